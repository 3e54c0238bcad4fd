"""GPU: the Winograd F(2x2, 3x3) form of the exact-fp32 3x3 convolution (ds_conv_args.wino, csrc/conv3x3_wino.hip) against an fp64 reference of
the layer and its whole epilogue, on the smallest shapes at which the kernel can still go wrong; the refused shapes; and the full-size
CIFAR-10 network with the form on and off against the oracle's golden.

Tolerance: the per-kernel bound of tests/test_hip_kernels.py, 2e-5 of the reference absmax.  An all-fp32 CPU simulation of F(2x2, 3x3) (pad,
4x4 unfold, B^T d B, per-position channel sums, A^T m A) against an fp64 direct convolution measured 5.8e-7 ... 6.2e-7 at 256 / 512 input
channels (the direct fp32 form: 2.5e-7 ... 3.2e-7): the transforms have entries 0, +-1, +-1/2 only.  Column sums and the statistics
ds_gn_finalize makes of them use the bounds of tests/test_hip_upconv.py (1e-5 on the sums, rtol 1e-4 / atol 1e-5 on mean and rstd).
`tune.mode = 256, tune.variant = 6` forces the 256 x 256 class (kernel id 2565) at these sizes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

TOL = 2e-5
SCALE = 0.7071


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


def _nhwc(x):      # [B,C,H,W] -> [B*H*W, C]
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


# name -> (B, H, c0, c1, cout, ec0, ec1, features)
CASES = {
    'one_image_per_tile_full_epilogue': (3, 16, 32, 0, 256, 0, 0, ('bias', 'cbias', 'scale', 'silu', 'res')),
    'four_tiles_per_image_two_sources_norm': (2, 32, 64, 32, 256, 0, 0, ('norm',)),
    'appended_skip_slabs': (2, 16, 64, 0, 256, 64, 32, ('bias',)),
    'ffhq64_geometry': (1, 64, 32, 0, 256, 0, 0, ()),
}


def _make(B, H, c0, c1, cout, ec0, ec1, feats):
    g = torch.Generator().manual_seed(B * 1000 + H * 10 + c0 + c1 + cout + ec0)
    cin = c0 + c1
    d = dict(x0=torch.randn(B, c0, H, H, generator=g), x1=torch.randn(B, c1, H, H, generator=g) if c1 else None,
             w=torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5)
    xin = torch.cat([t for t in (d['x0'], d['x1']) if t is not None], 1).double()
    if 'norm' in feats:          # planes {mu, A, B} per image; B != 0: an activated border pixel differs from a zero one
        d['coefs'] = torch.stack([torch.randn(B, cin, generator=g), 0.5 + torch.rand(B, cin, generator=g), 0.5 + torch.randn(B, cin, generator=g)], 1)
        mu, A_, B_ = (d['coefs'][:, i].double()[:, :, None, None] for i in range(3))
        xin = F.silu((xin - mu) * A_ + B_)
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
        _DATA[name] = _make(*CASES[name])
    return _DATA[name]


def _args(name, dev='cuda'):
    from diff_sampler_amd import _lib, ops
    B, H, c0, c1, cout, ec0, ec1, feats = CASES[name]
    d = _data(name)
    t = {k: (_nhwc(v).to(dev) if isinstance(v, torch.Tensor) and v.dim() == 4 and k not in ('w', 'ws') else v) for k, v in d.items()}
    wp = ops.pack_conv_weight_wino(d['w'].to(dev))
    if ec0:
        wp = ops.pack_conv_weight_wino(d['w'].to(dev), extra=d['ws'].to(dev))
    keep = dict(t, wp=wp)
    for k in ('bias', 'cb', 'coefs'):
        if k in d:
            keep[k] = d[k].to(dev).contiguous()
    out = torch.full((B * H * H, cout), float('nan'), device=dev)
    stats = torch.full((B * H * H // 64 * 2 * cout,), float('nan'), device=dev)
    p = lambda k: keep[k].data_ptr() if keep.get(k) is not None else None
    a = _lib.ConvArgs(p('x0'), p('x1'), c0, c1, c0, c1, B, H, H, 9, wp.data_ptr(), cout, p('bias'), p('cb'), cout if 'cb' in keep else 0,
                      B if 'cb' in keep else 1, p('res'), cout if 'res' in keep else 0, SCALE if 'scale' in feats else 1.0,
                      _lib.DS_ACT_SILU if 'silu' in feats else _lib.DS_ACT_NONE, out.data_ptr(), cout,
                      p('coefs'), _lib.DS_ACT_SILU if 'norm' in feats else _lib.DS_ACT_NONE, p('e0'), p('e1'), ec0, ec1, ec0, ec1)
    a.wino = 1
    a.stats_out = stats.data_ptr()
    a.tune.mode, a.tune.variant = 256, 6
    return a, out, stats, keep


@pytest.mark.parametrize('name', list(CASES))
def test_winograd_conv_matches_fp64(name):
    from diff_sampler_amd import _lib
    B, H, c0, c1, cout, ec0, ec1, feats = CASES[name]
    lib = _lib.load()
    a, out, stats, keep = _args(name)
    info = _lib.ConvRouteInfo()
    rc = lib.ds_conv_route(C.byref(a), C.byref(info))
    assert rc == 0 and info.wino == 1 and info.kernel_id == 2565 and info.splits == 1, (rc, info.wino, info.kernel_id, info.splits)
    rc = lib.ds_conv2d_nhwc(C.byref(a), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib.ds_error_string(rc)
    want = _data(name)['ref']
    got = out.cpu()
    err = _rel(got.double(), want)
    print(f'wino {name} {CASES[name][:7]}: rel err vs fp64 {err:.3e}')
    assert err < TOL
    # column sums: an image's h w / 64 blocks are contiguous and add up to the image's own sums
    nb = H * H // 64
    st = stats.cpu().reshape(B, nb, 2, cout).double()
    img = got.double().reshape(B, H * H, cout)
    e_s, e_q = _rel(st[:, :, 0].sum(1), img.sum(1)), _rel(st[:, :, 1].sum(1), (img ** 2).sum(1))
    print(f'wino {name}: column sums rel err {e_s:.3e} / {e_q:.3e}')
    assert e_s < 1e-5 and e_q < 1e-5
    # ... and ds_gn_finalize makes the consumer's GroupNorm statistics of them
    G_ = 32
    dev = 'cuda'
    mean, rstd = torch.empty(B * G_, device=dev), torch.empty(B * G_, device=dev)
    coefs = torch.empty(B * 3 * cout, device=dev)
    gamma, beta = torch.ones(cout, device=dev), torch.zeros(cout, device=dev)
    f = _lib.GnFinalizeArgs(stats.data_ptr(), None, cout, 0, B, H * H, G_, 1e-5, gamma.data_ptr(), beta.data_ptr(), None, None, 0, 1,
                            mean.data_ptr(), rstd.data_ptr(), coefs.data_ptr())
    assert lib.ds_gn_finalize(C.byref(f), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    r = want.reshape(B, H * H, G_, cout // G_).permute(0, 2, 1, 3).reshape(B, G_, -1)
    assert torch.allclose(mean.cpu(), r.mean(-1).float().reshape(-1), rtol=1e-4, atol=1e-5)
    assert torch.allclose(rstd.cpu(), (1.0 / (r.var(-1, unbiased=False) + 1e-5).sqrt()).float().reshape(-1), rtol=1e-4, atol=1e-5)


def test_refused_call_launches_nothing():
    """cout = 320 leaves a 64-column tail behind the 256-column tile: the call returns the route's code and leaves the output alone.  (8 x 8
    images -- four per 256-pixel tile -- are not on the 256 x 256 tiles with a fused normalisation either: the route refuses them the same way.)"""
    from diff_sampler_amd import _lib, ops
    lib = _lib.load()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2 * 16 * 16, 64, generator=g).cuda()
    wp = ops.pack_conv_weight_wino(torch.randn(320, 64, 3, 3, generator=g).cuda())
    out = torch.full((2 * 16 * 16, 320), 7.0, device='cuda')
    a = _lib.ConvArgs(x.data_ptr(), None, 64, 0, 64, 0, 2, 16, 16, 9, wp.data_ptr(), 320, None, None, 0, 1, None, 0, 1.0, 0, out.data_ptr(), 320)
    a.wino = 1
    a.tune.mode, a.tune.variant = 256, 6
    assert lib.ds_conv_kernel_id(C.byref(a)) == -3           # DS_E_SHAPE
    assert lib.ds_conv2d_nhwc(C.byref(a), _lib.stream_ptr()) == -3
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # (5, 8, 64, 0, 256): several 8 x 8 images per tile
    x8 = torch.randn(5 * 64, 64, generator=g).cuda()
    w8 = ops.pack_conv_weight_wino(torch.randn(256, 64, 3, 3, generator=g).cuda())
    o8 = torch.full((5 * 64, 256), 7.0, device='cuda')
    b = _lib.ConvArgs(x8.data_ptr(), None, 64, 0, 64, 0, 5, 8, 8, 9, w8.data_ptr(), 256, None, None, 0, 1, None, 0, 1.0, 0, o8.data_ptr(), 256)
    b.wino = 1
    b.tune.mode, b.tune.variant = 256, 6
    assert lib.ds_conv2d_nhwc(C.byref(b), _lib.stream_ptr()) == -3
    torch.cuda.synchronize()
    assert bool((o8 == 7.0).all())


def test_full_size_cifar10_with_and_without_winograd_matches_the_golden():
    """The full-size CIFAR-10 network at B = 64 (the golden's two images, 32 times), one evaluation per engine: both within the golden's 2e-4.
    The flag-on plan runs in the Winograd form EXACTLY the launches the flag-off plan runs on the 256 x 256 tiles (kernel id 2565, no
    split-K) outside the upsampled-input mode, the flag-off plan none.  At this batch that is 19 launches, not the "at least 20" the issue
    of this change expected: the 32 x 32 level has 20 launches of kernel id 2565 and one of them is the up block's conv0 in the
    upsampled-input mode, which the Winograd route refuses by the same issue's rule; the 16 x 16 layers split K at B = 64 (kernel id 128).
    Hence: full coverage of the eligible launches, and at least 19."""
    from diff_sampler_amd import _lib
    from diff_sampler_amd.engine import EDMDenoiser
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'net_cifar10.npz'))
    reps = 64 // z['x'].shape[0]
    x = torch.from_numpy(z['x']).repeat(reps, 1, 1, 1).cuda()
    sig = torch.from_numpy(z['sigma']).repeat(reps).cuda()
    want = torch.from_numpy(z['out_vec']).repeat(reps, 1, 1, 1)
    lib = _lib.load()
    outs, taken, eligible = [], [], []
    for flag in (True, False):
        net = EDMDenoiser.from_config('cifar10', seed=int(z['seed']), winograd=flag)
        out = net(x, sig)
        torch.cuda.synchronize()
        P = net.engine.plan(64, 64)
        took = []
        for op in P.ops:
            if op.fn is lib.ds_conv2d_nhwc:
                info = _lib.ConvRouteInfo()
                assert lib.ds_conv_route(C.byref(op.keep[0]), C.byref(info)) == 0
                assert info.wino == op.keep[0].wino
                if info.wino:
                    took.append(op.name)
                elif not flag and info.kernel_id == 2565 and info.splits == 1 and not op.keep[0].in_up2:
                    eligible.append(op.name)
        n_w = len(took)
        if flag:
            taken = took
        else:
            assert n_w == 0 and taken == eligible and len(taken) >= 19, (n_w, len(taken), len(eligible))
        outs.append(out.cpu())
        err = _rel(outs[-1], want)
        print(f'cifar10 B=64 winograd={flag}: {n_w} Winograd launches, rel err vs golden {err:.3e}')
        assert err < 2e-4
        del net
    print(f'cifar10 B=64: winograd on vs off, rel diff {_rel(outs[0], outs[1]):.3e}')
