"""GPU: the one-barrier K loop of the Winograd convolution (csrc/conv3x3_wino.hip: Vs and Hs are doubled like Us; between barrier s-1 and
barrier s the MFMAs of slab s run on Vs / Us[s & 1] while the transform of slab s+1 goes Hs[(s+1) & 1] -> Vs[(s+1) & 1], the halo of slab
s+2 is stored into Hs[s & 1], the weights of slab s+1 stream into Us[(s+1) & 1] and the halo and coefficients of slab s+3 are loaded;
s+1 / s+2 / s+3 are clamped to the last slab) on the smallest shapes at which the buffers' parity, the look-ahead of three slabs and the
hand-over to the skip loop and the epilogue can go wrong: one slab (every look-ahead clamped to slab 0), two and three (each buffer used
once; an odd count), four (the load three ahead reaches exactly the last slab), five on two sources with the boundary after the second
(first seen by the load three ahead), seven on two sources and two images adjacent in memory with the full epilogue and statistics, the
other two instantiations of the normalisation (affine only, none), 32- and 64-column images (3 and 4 halo slots per thread; the
width-dependent halo and tile mapping in both Hs buffers), and skip slabs behind three and behind four K slabs (the hand-over from either
buffer parity, with the last slab's redundant transform and halo store behind it).

Case table format, reference and bounds are those of tests/test_hip_wino_pipe.py and tests/test_hip_wino_pipe2.py: an fp64 reference of
the layer and its epilogue, 2e-5 of its absmax; column sums 1e-5, GroupNorm statistics rtol 1e-4 / atol 1e-5; outputs and statistics
prefilled with NaN.  Every case is launched twice and must give equal bits.  One more test runs this file against the two race-stress
libraries (the transform's writes and the halo store into either Hs buffer are DS_RACE_SKEW sites)."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

TOL = 2e-5
SCALE = 0.7071
FULL = ('norm', 'bias', 'cbias', 'res', 'scale', 'silu')

# name -> (B, H, c0, c1, cout, ec0, ec1, features)
CASES = {
    'one_slab_every_look_ahead_clamped': (1, 16, 8, 0, 256, 0, 0, ('norm',)),
    'two_slabs_each_buffer_used_once': (1, 16, 16, 0, 256, 0, 0, ('norm',)),
    'three_slabs_odd_count': (1, 16, 24, 0, 256, 0, 0, ('norm',)),
    'four_slabs_load_three_ahead_reaches_the_last': (1, 16, 32, 0, 256, 0, 0, ('norm',)),
    'five_slabs_source_boundary_after_the_second': (1, 16, 16, 24, 256, 0, 0, ('norm',)),
    'seven_slabs_two_sources_two_adjacent_images_full_epilogue': (2, 16, 24, 32, 256, 0, 0, FULL),
    'three_slabs_normalisation_without_activation': (1, 16, 24, 0, 256, 0, 0, ('norm', 'noact')),
    'three_slabs_no_normalisation': (1, 16, 24, 0, 256, 0, 0, ()),
    'three_slabs_on_32_columns': (1, 32, 24, 0, 256, 0, 0, ('norm',)),
    'three_slabs_on_64_columns_two_sources': (1, 64, 16, 8, 256, 0, 0, ('norm',)),
    'two_skip_slabs_behind_three_k_slabs': (1, 16, 24, 0, 256, 64, 0, ('norm', 'bias')),
    'two_skip_slabs_two_sources_behind_four_k_slabs': (1, 16, 32, 0, 256, 32, 32, ('norm', 'bias')),
}


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


def _nhwc(x):      # [B,C,H,W] -> [B*H*W, C]
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


def _make(seed, B, H, c0, c1, cout, ec0, ec1, feats):
    g = torch.Generator().manual_seed(7200 + seed)
    cin = c0 + c1
    d = dict(x0=torch.randn(B, c0, H, H, generator=g), x1=torch.randn(B, c1, H, H, generator=g) if c1 else None,
             w=torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5)
    xin = torch.cat([t for t in (d['x0'], d['x1']) if t is not None], 1).double()
    if 'norm' in feats:          # planes {mu, A, B} per image; B != 0: an activated border pixel differs from a zero one
        d['coefs'] = torch.stack([torch.randn(B, cin, generator=g), 0.5 + torch.rand(B, cin, generator=g), 0.5 + torch.randn(B, cin, generator=g)], 1)
        mu, A_, B_ = (d['coefs'][:, i].double()[:, :, None, None] for i in range(3))
        xin = (xin - mu) * A_ + B_
        if 'noact' not in feats:
            xin = F.silu(xin)
    ref = F.conv2d(xin, d['w'].double(), padding=1)
    if ec0:
        d['e0'] = torch.randn(B, ec0, H, H, generator=g)
        d['e1'] = torch.randn(B, ec1, H, H, generator=g) if ec1 else None
        d['ws'] = torch.randn(cout, ec0 + ec1, 1, 1, generator=g) / (ec0 + ec1) ** 0.5
        ref = ref + F.conv2d(torch.cat([t for t in (d['e0'], d['e1']) if t is not None], 1).double(), d['ws'].double())
    if 'bias' in feats:
        d['bias'] = torch.randn(cout, generator=g)
        ref = ref + d['bias'].double()[None, :, None, None]
    if 'cbias' in feats:
        d['cb'] = torch.randn(B, cout, generator=g)
        ref = ref + d['cb'].double()[:, :, None, None]
    if 'res' in feats:
        d['res'] = torch.randn(B, cout, H, H, generator=g)
        ref = ref + d['res'].double()
    if 'scale' in feats:
        ref = ref * SCALE
    if 'silu' in feats:
        ref = F.silu(ref)
    d['ref'] = _nhwc(ref)
    return d


_DATA = {}


def _data(name):
    """Inputs and the fp64 reference of a case, computed once and never written to."""
    if name not in _DATA:
        _DATA[name] = _make(list(CASES).index(name), *CASES[name])
    return _DATA[name]


def conv_args(name, dev='cuda'):
    """(ConvArgs, out, stats, keep-alive) of a case; out and stats prefilled with NaN.  tools/wino_bits.py uses it too."""
    from diff_sampler_amd import _lib, ops
    B, H, c0, c1, cout, ec0, ec1, feats = CASES[name]
    d = _data(name)
    keep = {k: (_nhwc(v).to(dev) if isinstance(v, torch.Tensor) and v.dim() == 4 and k not in ('w', 'ws') else v) for k, v in d.items()}
    keep['wp'] = ops.pack_conv_weight_wino(d['w'].to(dev), extra=d['ws'].to(dev)) if ec0 else ops.pack_conv_weight_wino(d['w'].to(dev))
    for k in ('bias', 'cb', 'coefs'):
        if k in d:
            keep[k] = d[k].to(dev).contiguous()
    out = torch.full((B * H * H, cout), float('nan'), device=dev)
    stats = torch.full((B * H * H // 64 * 2 * cout,), float('nan'), device=dev)
    p = lambda k: keep[k].data_ptr() if keep.get(k) is not None else None
    norm_act = _lib.DS_ACT_SILU if 'norm' in feats and 'noact' not in feats else _lib.DS_ACT_NONE
    a = _lib.ConvArgs(p('x0'), p('x1'), c0, c1, c0, c1, B, H, H, 9, keep['wp'].data_ptr(), cout, p('bias'), p('cb'), cout if 'cb' in keep else 0,
                      B if 'cb' in keep else 1, p('res'), cout if 'res' in keep else 0, SCALE if 'scale' in feats else 1.0,
                      _lib.DS_ACT_SILU if 'silu' in feats else _lib.DS_ACT_NONE, out.data_ptr(), cout,
                      p('coefs'), norm_act, p('e0'), p('e1'), ec0, ec1, ec0, ec1)
    a.wino = 1
    a.stats_out = stats.data_ptr()
    a.tune.mode, a.tune.variant = 256, 6
    return a, out, stats, keep


def _launch(lib, name):
    from diff_sampler_amd import _lib
    a, out, stats, keep = conv_args(name)
    info = _lib.ConvRouteInfo()
    rc = lib.ds_conv_route(C.byref(a), C.byref(info))
    assert rc == 0 and info.wino == 1 and info.kernel_id == 2565 and info.splits == 1, (rc, info.wino, info.kernel_id, info.splits)
    rc = lib.ds_conv2d_nhwc(C.byref(a), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib.ds_error_string(rc)
    return out, stats


@pytest.mark.parametrize('name', list(CASES))
def test_one_barrier_k_loop_matches_fp64_and_repeats_its_bits(name):
    from diff_sampler_amd import _lib
    B, H, c0, c1, cout, ec0, ec1, feats = CASES[name]
    lib = _lib.load()
    out, stats = _launch(lib, name)
    want = _data(name)['ref']
    got = out.cpu()
    err = _rel(got.double(), want)
    print(f'wino kloop {name} {CASES[name][:7]}: {(c0 + c1) // 8} slabs + {(ec0 + ec1) // 32} skip slabs, rel err vs fp64 {err:.3e}')
    assert bool(torch.isfinite(got).all())
    assert err < TOL
    # column sums: an image's h w / 64 blocks are contiguous and add up to the image's own sums
    nb = H * H // 64
    st = stats.cpu().reshape(B, nb, 2, cout).double()
    img = got.double().reshape(B, H * H, cout)
    e_s, e_q = _rel(st[:, :, 0].sum(1), img.sum(1)), _rel(st[:, :, 1].sum(1), (img ** 2).sum(1))
    print(f'wino kloop {name}: column sums rel err {e_s:.3e} / {e_q:.3e}')
    assert e_s < 1e-5 and e_q < 1e-5
    # ... and ds_gn_finalize makes the consumer's GroupNorm statistics of them
    G_ = 32
    mean, rstd = torch.empty(B * G_, device='cuda'), torch.empty(B * G_, device='cuda')
    coefs = torch.empty(B * 3 * cout, device='cuda')
    gamma, beta = torch.ones(cout, device='cuda'), torch.zeros(cout, device='cuda')
    f = _lib.GnFinalizeArgs(stats.data_ptr(), None, cout, 0, B, H * H, G_, 1e-5, gamma.data_ptr(), beta.data_ptr(), None, None, 0, 1,
                            mean.data_ptr(), rstd.data_ptr(), coefs.data_ptr())
    assert lib.ds_gn_finalize(C.byref(f), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    r = want.reshape(B, H * H, G_, cout // G_).permute(0, 2, 1, 3).reshape(B, G_, -1)
    assert torch.allclose(mean.cpu(), r.mean(-1).float().reshape(-1), rtol=1e-4, atol=1e-5)
    assert torch.allclose(rstd.cpu(), (1.0 / (r.var(-1, unbiased=False) + 1e-5).sqrt()).float().reshape(-1), rtol=1e-4, atol=1e-5)
    # determinism: a second launch into fresh NaN-filled buffers gives the same bits
    out2, stats2 = _launch(lib, name)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32))
    assert torch.equal(stats.view(torch.int32), stats2.view(torch.int32))


@pytest.mark.parametrize('tag', ['stress_a', 'stress_b'])
def test_k_loop_cases_pass_against_the_race_stress_library(tag):
    """The cases above, unchanged, against a library whose LDS-producing waves are delayed (two complementary wave masks), each in a fresh
    child process with a timeout -- the way tests/test_hip_wino_pipe2.py runs the skip loop's cases."""
    from diff_sampler_amd import build
    lib = build.variant_lib(tag)
    assert os.path.exists(lib), f'{lib} is missing: __graft_entry__.build() / python -m diff_sampler_amd.build --variants builds it'
    assert C.CDLL(lib).ds_build_experiments() & 2, 'not a DS_RACE_STRESS build'
    env = dict(os.environ, DS_LIB_PATH=lib, DS_AUTOTUNE='0')
    cmd = [sys.executable, '-m', 'pytest', '-x', '-q', '-m', 'gpu', '-p', 'no:cacheprovider', 'tests/test_hip_wino_kloop.py', '-k', 'not race_stress']
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = (r.stdout or '')[-3000:] + (r.stderr or '')[-1500:]
    assert r.returncode == 0, f'{os.path.basename(lib)}\n{tail}'
    summary = r.stdout.strip().splitlines()[-1]
    assert 'passed' in summary and 'failed' not in summary and 'skipped' not in summary, summary
