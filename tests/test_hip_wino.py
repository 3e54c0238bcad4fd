"""GPU: the Winograd F(2x2, 3x3) form of the exact-fp32 3x3 convolution (ds_conv_args.wino, csrc/conv3x3_wino.hip) against an fp64 reference of
the layer and its whole epilogue, on the case table of tests/_conv_randn.py (WINO_GROUPS: the smallest shapes at which the kernel can
still go wrong, and which hazard each one guards); the refused shapes; and the full-size CIFAR-10 network with the form on and off
against the oracle's golden.  Reference, tolerances and the checks themselves are those of tests/_conv_randn.py.
tests/test_hip_race_stress.py runs this whole file against the two race-stress libraries (every producer of shared LDS contents in the
kernel is a DS_RACE_SKEW site)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _conv_randn as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _launch(lib, row):
    """Route assertion and one launch into fresh NaN-filled guarded buffers."""
    from diff_sampler_amd import _lib
    a, out, stats, keep = R.wino_args(row, 'cuda')
    info = _lib.ConvRouteInfo()
    rc = lib.ds_conv_route(C.byref(a), C.byref(info))
    assert rc == 0 and info.wino == 1 and info.kernel_id == 2565 and info.splits == 1, (rc, info.wino, info.kernel_id, info.splits)
    rc = lib.ds_conv2d_nhwc(C.byref(a), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib.ds_error_string(rc)
    return out, stats, keep['out_buf'], keep['stats_buf']


@pytest.mark.parametrize('group,name', [(g, n) for g, t in R.WINO_GROUPS.items() for n in t],
                         ids=[f'{g}-{n}' for g, t in R.WINO_GROUPS.items() for n in t])
def test_winograd_conv_matches_fp64_and_repeats_its_bits(group, name):
    from diff_sampler_amd import _lib
    row = R.WINO_GROUPS[group][name]
    seed, B, H, c0, c1, cout, ec0, ec1, feats = row
    lib = _lib.load()
    out, stats, out_buf, stats_buf = _launch(lib, row)
    err, per, e_s, e_q = R.compare(row, out.cpu(), stats.cpu(), out_buf.cpu(), stats_buf.cpu())
    print(f'wino {group} {name} {row[1:8]}: {(c0 + c1) // 8} slabs + {(ec0 + ec1) // 32} skip slabs, rel err vs fp64 {err:.3e} '
          f'(worst image {per.index(max(per))}), column sums rel err {e_s:.3e} / {e_q:.3e}')
    R.finalize_check(lib, stats, R.make_layer(*row)['ref'], B, H * H, cout)
    # launch independence: the same call into fresh buffers gives the same bits, interiors and NaN margins alike
    bufs2 = _launch(lib, row)[2:]
    assert torch.equal(out_buf.view(torch.int32), bufs2[0].view(torch.int32))
    assert torch.equal(stats_buf.view(torch.int32), bufs2[1].view(torch.int32))
    if group == 'persist':
        counts, padded = R.tiles_per_workgroup(B, H, cout, R.device_cus())
        print(f'wino persist {name}: {len(counts)} sequences b, b + G, ..., tiles per sequence {min(counts)} .. {max(counts)} '
              f'({sum(c == max(counts) for c in counts)} run {max(counts)}), {padded} padded indices')
        assert (max(counts), min(counts)) == R.PERSIST_TILES[name]
        if name == 'padded_grid_has_invalid_indices':
            assert padded > 0


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
        err = R.rel(outs[-1], want)
        print(f'cifar10 B=64 winograd={flag}: {n_w} Winograd launches, rel err vs golden {err:.3e}')
        assert err < 2e-4
        del net
    print(f'cifar10 B=64: winograd on vs off, rel diff {R.rel(outs[0], outs[1]):.3e}')
