"""GPU: the Winograd convolution (csrc/conv3x3_wino.hip) on launches of MORE TILES THAN COMPUTE UNITS, the shapes that were sized for a
persistent form of the kernel (at most one workgroup per compute unit, workgroup b running the tiles b, b + G, ... of decode_tile's
order, the next tile's first slabs requested under the epilogue of the tile before).  That form was built and measured and is not the
kernel (profiles/wino_persist_ab.txt: it was slower than one workgroup per tile); its cases stay, because they are what the kept part of
that work needs: a workgroup holds a whole compute unit's LDS (156 KB of 160), so the workgroups of the second and third round start on
the LDS that another tile's workgroup left behind -- and the kernel now writes the zeros of a tile's out-of-image halo cells ONCE, in
front of the K loop, into both Hs buffers, where an earlier tile of another image row may have left in-image pixels.

One 16x16 image is one M tile and cout = 256 gives four N tiles, so n images are 4 n tiles, padded by grid_1d to a multiple of 32; a
32x32 image is four M tiles (its tiles have a top border, none, or a bottom border), a 64x64 image sixteen.  The image counts are
derived from the device's compute-unit count, and every case asserts the tile counts it is named after: tiles_per_workgroup() deals the
indices b, b + G, ... (G = the compute units, rounded down to a multiple of 8) as decode_tile / grid_1d would -- the tiles a persistent
workgroup would run, and with one workgroup per tile the number of workgroups that use a compute unit's LDS in turn.  With four N tiles
the padded indices all lie in the last group of 32, i.e. at the END of such a sequence, never in its middle.

Reference and bounds are those of tests/test_hip_wino_kloop.py (its _make): an fp64 reference of the layer and its epilogue, 2e-5 of its
absmax; column sums 1e-5.  `out` and `stats` lie inside larger NaN-filled buffers whose margins must stay NaN; every case is launched
twice into fresh buffers and must give equal bits.  One more test runs this file against the two race-stress libraries (the halo stores
and the transform's writes are DS_RACE_SKEW sites; the border zeros are written in front of the first of them)."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

TOL = 2e-5
GUARD = 4096          # floats of NaN in front of and behind `out` and `stats`


def _kloop():
    spec = importlib.util.spec_from_file_location('_wino_kloop_cases', os.path.join(ROOT, 'tests', 'test_hip_wino_kloop.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_K = _kloop()
FULL = _K.FULL


def _cus():
    """Compute units of device 0 (256 where there is no device: the case table is then only collected, never run)."""
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def _cases():
    cu = _cus()
    # name -> (B, H, c0, c1, cout, ec0, ec1, features), then what tiles_per_workgroup() must give: (max tiles of a workgroup, min)
    return {
        'one_slab_a_few_workgroups_run_two_tiles': ((cu // 4 + 1, 16, 8, 0, 256, 0, 0, ('norm',)), (2, 1)),
        'padded_grid_has_invalid_indices': ((cu // 4 + 2, 16, 8, 0, 256, 0, 0, ('norm',)), (2, 1)),
        'three_tiles_of_three_slabs': ((cu // 2 + 1, 16, 24, 0, 256, 0, 0, ('norm',)), (3, 2)),
        'two_sources_full_epilogue_second_tile_is_another_image': ((cu // 4 + 1, 16, 16, 8, 256, 0, 0, FULL), (2, 1)),
        'two_skip_slabs_behind_three_k_slabs_two_tiles': ((cu // 4 + 1, 16, 24, 0, 256, 64, 0, ('norm', 'bias')), (2, 1)),
        'two_tiles_on_32_columns': ((cu // 16 + 1, 32, 8, 0, 256, 0, 0, ('norm',)), (2, 1)),
        'two_tiles_on_64_columns_four_halo_slots': ((cu // 64 + 1, 64, 8, 0, 256, 0, 0, ('norm',)), (2, 1)),
    }


_TABLE = _cases()
CASES = {k: v[0] for k, v in _TABLE.items()}


def tiles_per_workgroup(B, H, cout, cus):
    """(valid tiles of every sequence b, b + G, ..., padded indices) of a launch: grid_1d and decode_tile in Python."""
    mtiles, ntiles = B * H * H // 256, cout // 64
    swapped = mtiles < 8 and ntiles > mtiles
    total = (ntiles + 7) // 8 * 8 * mtiles if swapped else (mtiles + 7) // 8 * 8 * ntiles
    nwg = min(total, cus // 8 * 8)

    def valid(b):
        if swapped:
            g, r = divmod(b, 8 * mtiles)
            return g * 8 + (r & 7) < ntiles
        g, r = divmod(b, 8 * ntiles)
        return g * 8 + (r & 7) < mtiles
    counts = [sum(valid(b) for b in range(w, total, nwg)) for w in range(nwg)]
    return counts, total - sum(counts)


_DATA = {}


def _data(name):
    """Inputs and the fp64 reference of a case, computed once and never written to."""
    if name not in _DATA:
        _DATA[name] = _K._make(100 + list(CASES).index(name), *CASES[name])
    return _DATA[name]


def conv_args(name, dev='cuda'):
    """(ConvArgs, out, stats, keep-alive) of a case; out and stats are the interiors of NaN-filled buffers (keep['out_buf'],
    keep['stats_buf']: GUARD floats on either side).  tools/wino_bits.py uses it too."""
    from diff_sampler_amd import _lib, ops
    B, H, c0, c1, cout, ec0, ec1, feats = CASES[name]
    d = _data(name)
    keep = {k: (_K._nhwc(v).to(dev) if isinstance(v, torch.Tensor) and v.dim() == 4 and k not in ('w', 'ws') else v) for k, v in d.items()}
    keep['wp'] = ops.pack_conv_weight_wino(d['w'].to(dev), extra=d['ws'].to(dev)) if ec0 else ops.pack_conv_weight_wino(d['w'].to(dev))
    for k in ('bias', 'cb', 'coefs'):
        if k in d:
            keep[k] = d[k].to(dev).contiguous()
    n_out, n_st = B * H * H * cout, B * H * H // 64 * 2 * cout
    keep['out_buf'] = torch.full((n_out + 2 * GUARD,), float('nan'), device=dev)
    keep['stats_buf'] = torch.full((n_st + 2 * GUARD,), float('nan'), device=dev)
    out = keep['out_buf'][GUARD:GUARD + n_out].view(B * H * H, cout)
    stats = keep['stats_buf'][GUARD:GUARD + n_st]
    p = lambda k: keep[k].data_ptr() if keep.get(k) is not None else None
    a = _lib.ConvArgs(p('x0'), p('x1'), c0, c1, c0, c1, B, H, H, 9, keep['wp'].data_ptr(), cout, p('bias'), p('cb'), cout if 'cb' in keep else 0,
                      B if 'cb' in keep else 1, p('res'), cout if 'res' in keep else 0, _K.SCALE if 'scale' in feats else 1.0,
                      _lib.DS_ACT_SILU if 'silu' in feats else _lib.DS_ACT_NONE, out.data_ptr(), cout,
                      p('coefs'), _lib.DS_ACT_SILU if 'norm' in feats else _lib.DS_ACT_NONE, p('e0'), p('e1'), ec0, ec1, ec0, ec1)
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
    for buf in (keep['out_buf'], keep['stats_buf']):        # nothing outside the tensors is written
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[-GUARD:]).all())
    return out, stats


@pytest.mark.parametrize('name', list(CASES))
def test_launches_of_several_tile_rounds_match_fp64_and_repeat_their_bits(name):
    from diff_sampler_amd import _lib
    B, H, c0, c1, cout, ec0, ec1, feats = CASES[name]
    counts, padded = tiles_per_workgroup(B, H, cout, _cus())
    print(f'wino persist {name} {CASES[name][:7]}: {len(counts)} sequences b, b + G, ..., tiles per sequence {min(counts)} .. {max(counts)} '
          f'({sum(c == max(counts) for c in counts)} run {max(counts)}), {padded} padded indices')
    assert (max(counts), min(counts)) == _TABLE[name][1]
    if name == 'padded_grid_has_invalid_indices':
        assert padded > 0
    lib = _lib.load()
    out, stats = _launch(lib, name)
    want = _data(name)['ref']
    got = out.cpu()
    err = _K._rel(got.double(), want)
    print(f'wino persist {name}: {(c0 + c1) // 8} slabs + {(ec0 + ec1) // 32} skip slabs, rel err vs fp64 {err:.3e}')
    assert bool(torch.isfinite(got).all())
    assert err < TOL
    # every image against its own reference: a tile that took another tile's image, coefficients or cbias row fails here by name
    per = ((got.double() - want).abs().reshape(B, -1).amax(1) / want.abs().max()).tolist()
    assert max(per) < TOL, f'image {per.index(max(per))}: {max(per):.3e}'
    # column sums: an image's h w / 64 blocks are contiguous and add up to the image's own sums
    nb = H * H // 64
    st = stats.cpu().reshape(B, nb, 2, cout).double()
    img = got.double().reshape(B, H * H, cout)
    e_s, e_q = _K._rel(st[:, :, 0].sum(1), img.sum(1)), _K._rel(st[:, :, 1].sum(1), (img ** 2).sum(1))
    print(f'wino persist {name}: column sums rel err {e_s:.3e} / {e_q:.3e}')
    assert e_s < 1e-5 and e_q < 1e-5
    # launch independence: the same call into fresh NaN-filled buffers gives the same bits
    out2, stats2 = _launch(lib, name)
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32))
    assert torch.equal(stats.view(torch.int32), stats2.view(torch.int32))


@pytest.mark.parametrize('tag', ['stress_a', 'stress_b'])
def test_several_round_cases_pass_against_the_race_stress_library(tag):
    """The cases above, unchanged, against a library whose LDS-producing waves are delayed (two complementary wave masks), each in a fresh
    child process with a timeout -- the way tests/test_hip_wino_kloop.py runs its cases."""
    from diff_sampler_amd import build
    lib = build.variant_lib(tag)
    assert os.path.exists(lib), f'{lib} is missing: __graft_entry__.build() / python -m diff_sampler_amd.build --variants builds it'
    assert C.CDLL(lib).ds_build_experiments() & 2, 'not a DS_RACE_STRESS build'
    env = dict(os.environ, DS_LIB_PATH=lib, DS_AUTOTUNE='0')
    cmd = [sys.executable, '-m', 'pytest', '-x', '-q', '-m', 'gpu', '-p', 'no:cacheprovider', 'tests/test_hip_wino_persist.py', '-k', 'not race_stress']
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    tail = (r.stdout or '')[-3000:] + (r.stderr or '')[-1500:]
    assert r.returncode == 0, f'{os.path.basename(lib)}\n{tail}'
    summary = r.stdout.strip().splitlines()[-1]
    assert 'passed' in summary and 'failed' not in summary and 'skipped' not in summary, summary
