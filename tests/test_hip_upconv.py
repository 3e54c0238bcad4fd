"""GPU: the upsampled-input 3x3 convolution (ds_conv_args.in_up2, conv3x3_halo_kernel<.., UP = 1>) against an fp64 reference of
conv3x3(nearest_x2(x)), on every tile shape that has the mode, with the whole epilogue (bias, per-image bias, scale, SiLU, GroupNorm column
sums); and an engine with and without it against the oracle's golden.

Tolerance: the bound of tests/test_hip_kernels.py (2e-5 relative to the output scale).  The folded form sums at most four fp32 weights before
the fp32 FMA chain of 4 cin terms; measured on the CPU at 256 -> 256 channels it is as close to the fp64 result (2.1e-7) as the direct 9-tap
form (2.5e-7)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _conv_randn as R  # noqa: E402

pytestmark = pytest.mark.gpu

TOL, SCALE, _rel, _nhwc = R.TOL, R.SCALE, R.rel, R.nhwc


_CASES = {}


def _case(B, Hin, cin, cout):
    """Inputs and the fp64 reference of one layer, computed once and shared by the tile shapes that run it (never written to)."""
    key = (B, Hin, cin, cout)
    if key not in _CASES:
        g = torch.Generator().manual_seed(B * 1000 + Hin * 10 + cin + cout)
        x = torch.randn(B, cin, Hin, Hin, generator=g)
        w = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
        bias, cb = torch.randn(cout, generator=g), torch.randn(B, cout, generator=g)
        ref = F.conv2d(F.interpolate(x.double(), scale_factor=2, mode='nearest'), w.double(), padding=1)
        ref = F.silu((ref + bias.double()[None, :, None, None] + cb.double()[:, :, None, None]) * SCALE)
        _CASES[key] = (x, w, bias, cb, _nhwc(ref))
    return _CASES[key]


# (B, Hin, cin, cout), tune.mode, tune.variant, kernel id
CASES = [
    ((3, 16, 64, 256), 256, 6, 2565),           # 256 x 256 tile, one image per tile
    ((2, 32, 32, 256), 256, 6, 2565),           # a tile is 8 rows of an image: halo rows cross tile boundaries
    ((5, 8, 64, 256), 256, 6, 2565),            # four 8x8 images per 256 x 256 tile, ragged last tile (the 8 -> 16 layer of the headline)
    ((3, 16, 64, 128), 0, 0, 1284),             # default route at this size: 128-pixel tiles on eight half-size waves
    ((3, 16, 64, 128), 128, 2048, 128),         # 128 x 128 tile on four waves
    ((3, 16, 64, 128), 256, 0, 256),            # 256 x 128 tile
    ((5, 8, 64, 128), 0, 0, 1284),              # two images per 128-pixel tile, ragged last tile
    ((5, 8, 64, 128), 256, 0, 256),             # four images per 256-pixel tile, ragged last tile
    ((2, 16, 64, 192), 256, 16384, 2568),       # 256 x 192 tile
    ((2, 16, 64, 384), 256, 6, 2565),           # 384 = 256 + 128: a second launch of 128-column tiles from column 256
]


@pytest.mark.parametrize('shape,mode,variant,want_kid', CASES)
def test_upsampled_input_conv_matches_fp64(shape, mode, variant, want_kid):
    from diff_sampler_amd import _lib, ops
    B, Hin, cin, cout = shape
    H = 2 * Hin
    x, w, bias, cb, want = _case(*shape)
    lib = _lib.load()
    dev = 'cuda'
    xn, wp, bd, cbd = _nhwc(x).to(dev), ops.pack_conv_weight_up2(w.to(dev)), bias.to(dev), cb.to(dev)
    out = torch.full((B * H * H, cout), float('nan'), device=dev)
    stats = torch.full((B * H * H // 64 * 2 * cout,), float('nan'), device=dev)
    a = _lib.ConvArgs(xn.data_ptr(), None, cin, 0, cin, 0, B, H, H, 9, wp.data_ptr(), cout, bd.data_ptr(), cbd.data_ptr(), cout, B, None, 0,
                      SCALE, _lib.DS_ACT_SILU, out.data_ptr(), cout)
    a.in_up2 = 1
    a.stats_out = stats.data_ptr()
    a.tune.mode, a.tune.variant = mode, variant
    kid = lib.ds_conv_kernel_id(C.byref(a))
    assert kid == want_kid, (kid, want_kid)
    rc = lib.ds_conv2d_nhwc(C.byref(a), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib.ds_error_string(rc)
    got = out.cpu()
    err = _rel(got.double(), want)
    print(f'in_up2 {shape} kernel {kid}: rel err vs fp64 {err:.3e}')
    assert err < TOL
    # column sums: an image's h w / 64 blocks are contiguous (phase-major inside the image) and add up to the image's own sums
    e_s, e_q = R.column_sum_errors(got, stats.cpu(), B, H * H, cout)
    assert e_s < 1e-5 and e_q < 1e-5
    # ... and ds_gn_finalize makes the consumer's GroupNorm statistics of them
    R.finalize_check(lib, stats, want, B, H * H, cout)


def test_refused_call_launches_nothing():
    """A 64-column tail (cout = 320) has no upsampled-input tile: the call returns the route's code and leaves the output alone."""
    from diff_sampler_amd import _lib, ops
    x, w, bias, cb, _ = _case(3, 16, 64, 128)
    lib = _lib.load()
    w320 = torch.cat([w, w, w[:64]], 0)
    xn, wp = _nhwc(x).cuda(), ops.pack_conv_weight_up2(w320.cuda())
    out = torch.full((3 * 32 * 32, 320), 7.0, device='cuda')
    a = _lib.ConvArgs(xn.data_ptr(), None, 64, 0, 64, 0, 3, 32, 32, 9, wp.data_ptr(), 320, None, None, 0, 1, None, 0, 1.0, 0, out.data_ptr(), 320)
    a.in_up2 = 1
    assert lib.ds_conv_kernel_id(C.byref(a)) == -3           # DS_E_SHAPE
    assert lib.ds_conv2d_nhwc(C.byref(a), _lib.stream_ptr()) == -3
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


def test_engine_with_and_without_the_mode_matches_the_golden():
    """tiny_adm is the smallest named net whose up block the route takes (128 channels, 8 -> 16; tiny_song's has 64): both engines within the
    golden's 2e-4 (tests/test_hip_denoiser.py), three images."""
    from diff_sampler_amd import _lib
    from diff_sampler_amd.engine import EDMDenoiser
    name = 'tiny_adm'
    z = np.load(os.path.join(ROOT, 'tests', 'golden', f'net_{name}.npz'))
    n = min(3, z['x'].shape[0])
    x = torch.from_numpy(z['x'][:n]).cuda()
    sig = torch.from_numpy(z['sigma'][:n]).cuda()
    lab = torch.from_numpy(z['labels'][:n]).cuda() if z['labels'].size else None
    want = torch.from_numpy(z['out_vec'][:n])
    outs = []
    for up_phase in (True, False):
        net = EDMDenoiser.from_config(name, seed=int(z['seed']), up_phase=up_phase)
        out = net(x, sig, class_labels=lab)
        torch.cuda.synchronize()
        P = net.engine.plan(n, n)
        used = [op.name for op in P.ops if op.fn is _lib.load().ds_conv2d_nhwc and op.keep[0].in_up2]
        assert (len(used) == 1 and used[0].endswith('_up.conv0')) if up_phase else not used, used
        outs.append(out.cpu())
        assert _rel(outs[-1], want) < 2e-4
    print(f'{name}: up_phase on vs off, rel diff {_rel(outs[0], outs[1]):.3e}; vs golden {_rel(outs[0], want):.3e} / {_rel(outs[1], want):.3e}')
