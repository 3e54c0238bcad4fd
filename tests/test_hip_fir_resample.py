"""GPU: dsm_fir_resample and dsm_zero_border (csrc/metrics/fir_resample.hip) element by element.

Every output buffer is prefilled with NaN and carries guard rows before and after the output rows and, where ld > c, padding columns: all
of that must still be NaN afterwards, and a second call must give the same bits.  The bound is per element against the fp64 depthwise
convolution written as the reference's ``Conv2d.forward`` writes it (tests/_ncsnpp_ref.py), derived by counting fp32 roundings as
tests/_norm_refs.py does: one per tap FMA (T = 16 down, 4 up) and one each for the bias add, the residual add and the scale,

    |got - ref| <= (T + 3) 2^-24 (sum |tap x| + |bias| + |res|) |out_scale|

(the 2-D weights of [1,3,3,1] are exact in fp32, so the reference and the kernel multiply by the same numbers).  dsm_zero_border is exact.
"""
import ctypes as C
import math
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _ncsnpp_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
TAPS = (1, 3, 3, 1)
GUARD = 3


@pytest.fixture(scope='module')
def mlib():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    from diff_sampler_amd import _metrics_lib
    return _metrics_lib.load()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _rows(rows, c, ld, gen, scale=1.0):
    """[rows, ld] on the device: N(0, scale^2) in the first c columns, NaN in the padding."""
    t = torch.full((rows, ld), float('nan'), dtype=torch.float32)
    t[:, :c] = torch.randn(rows, c, generator=gen) * scale
    return t.cuda()


def _run_fir(mlib, x, n, h, w, c, ld, up, pad, bias=None, res=None, res_ld=0, scale=1.0, out_ld=None, taps=TAPS):
    """Launch twice into a NaN-prefilled, guarded buffer; returns the [rows, c] result after checking guards, padding and repeatability."""
    from diff_sampler_amd import _lib, _metrics_lib as ML
    ho, wo = (2 * h, 2 * w) if up else ((h + 2 * pad - 4) // 2 + 1, (w + 2 * pad - 4) // 2 + 1)
    rows, out_ld = n * ho * wo, out_ld or ld
    outs = []
    for _ in range(2):
        buf = torch.full((rows + 2 * GUARD, out_ld), float('nan'), dtype=torch.float32, device='cuda')
        out = buf[GUARD:GUARD + rows]
        a = ML.DsmFirArgs(_ptr(x), ld, n, h, w, c, 1 if up else 0, pad, (C.c_float * 4)(*taps), _ptr(bias), _ptr(res), res_ld, scale, _ptr(out), out_ld)
        ML.check(mlib.dsm_fir_resample(C.byref(a), _lib.stream_ptr()), 'dsm_fir_resample')
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + rows:]).all()), 'guard rows were written'
        assert bool(torch.isnan(out[:, c:]).all()), 'padding columns were written'
        assert bool(torch.isfinite(out[:, :c]).all()), 'an output element was not written'
        outs.append(out[:, :c].clone())
    assert torch.equal(outs[0], outs[1]), 'two calls, different bits'
    return outs[0].cpu(), (ho, wo)


def _check(mlib, n, h, w, c, ld, up, pad, epilogue, seed):
    g = torch.Generator().manual_seed(seed)
    x = _rows(n * h * w, c, ld, g, 2.0)
    ho, wo = (2 * h, 2 * w) if up else ((h + 2 * pad - 4) // 2 + 1, (w + 2 * pad - 4) // 2 + 1)
    bias = res = None
    scale, res_ld = 1.0, 0
    if epilogue:
        bias, res_ld, scale = torch.randn(c, generator=g).cuda(), ld + 4, 1.0 / math.sqrt(2.0)
        res = _rows(n * ho * wo, c, res_ld, g, 1.5)
    got, size = _run_fir(mlib, x, n, h, w, c, ld, up, pad, bias, res, res_ld, scale)
    assert size == (ho, wo)
    ref, mag = R.fir_rows_ref(x.cpu(), n, h, w, c, TAPS, up, pad, None if bias is None else bias.cpu(), None if res is None else res.cpu(), scale)
    worst = R.assert_close_rows(got, ref, R.fir_bound(mag, up), (n, h, w, c, ld, up, pad))
    print(f'fir up={int(up)} pad={pad} {(n, h, w, c, ld)} -> {ho}x{wo}: worst error / bound = {worst:.3f}')


@pytest.mark.parametrize('shape', [(2, 8, 8, 4, 4), (1, 6, 10, 36, 40), (3, 2, 2, 8, 8)], ids=str)
def test_down_pad1(mlib, shape):
    """The stand-alone down form: h != w, a channel count that is no power of two, and 2x2 -> 1x1 where every tap row touches the border."""
    _check(mlib, *shape, up=False, pad=1, epilogue=False, seed=sum(shape))


@pytest.mark.parametrize('shape,size', [((3, 34, 34, 32, 32), (16, 16)), ((2, 10, 6, 8, 12), (4, 2))], ids=str)
def test_down_pad0_with_bias_residual_and_scale(mlib, shape, size):
    """The aux-residual launch: second half of fused_resample + bias + the down block's output, all times 1 / sqrt(2)."""
    n, h, w, c, ld = shape
    assert ((h - 4) // 2 + 1, (w - 4) // 2 + 1) == size
    _check(mlib, *shape, up=False, pad=0, epilogue=True, seed=sum(shape))


@pytest.mark.parametrize('shape', [(2, 4, 4, 4, 4), (1, 3, 5, 36, 40), (2, 1, 1, 8, 8)], ids=str)
@pytest.mark.parametrize('epilogue', [False, True], ids=['plain', 'epilogue'])
def test_up(mlib, shape, epilogue):
    """x2 up (two taps per axis): odd input sizes and the 1x1 image, whose four outputs each see one in-image tap."""
    _check(mlib, *shape, up=True, pad=1, epilogue=epilogue, seed=sum(shape) + 100)


def test_up_of_a_constant_is_the_constant_inside_and_the_phase_weights_at_the_border(mlib):
    """[1,3,3,1] up: 3/4 | 1/4 per axis -- interior outputs of a constant image are the constant, corners (3/4)^2 of it."""
    x = torch.ones(1 * 4 * 4, 4, device='cuda')
    got, _ = _run_fir(mlib, x, 1, 4, 4, 4, 4, True, 1)
    img = got.reshape(8, 8, 4)
    assert torch.equal(img[1:7, 1:7], torch.ones(6, 6, 4)) and float(img[0, 0, 0]) == 0.5625 and float(img[0, 3, 0]) == 0.75


def test_box_filter_taps_are_the_average_pool(mlib):
    """taps [0,1,1,0] = the reference's [1,1] filter embedded in four taps: 2x2 average pooling (pad 1) and nearest-neighbour x2 up."""
    g = torch.Generator().manual_seed(9)
    x = _rows(2 * 6 * 6, 8, 8, g)
    got, _ = _run_fir(mlib, x, 2, 6, 6, 8, 8, False, 1, taps=(0, 1, 1, 0))
    img = x.cpu().reshape(2, 6, 6, 8).permute(0, 3, 1, 2).double()
    want = torch.nn.functional.avg_pool2d(img, 2).permute(0, 2, 3, 1).reshape(-1, 8)
    assert float((got.double() - want).abs().max()) <= 4 * 2.0 ** -24 * float(img.abs().max())
    up, _ = _run_fir(mlib, x, 2, 6, 6, 8, 8, True, 1, taps=(0, 1, 1, 0))
    assert torch.equal(up.reshape(2, 12, 12, 8), x.cpu().reshape(2, 6, 6, 8).repeat_interleave(2, 1).repeat_interleave(2, 2))


def test_down_then_up_at_the_cifar_ve_sizes(mlib):
    """The buffers of the CIFAR-10 `ve` net at B = 2: 32 -> 16 at 256 channels (more than one workgroup), then 16 -> 32 of that result."""
    n, c = 2, 256
    g = torch.Generator().manual_seed(21)
    x = _rows(n * 32 * 32, c, c, g, 2.0)
    down, size = _run_fir(mlib, x, n, 32, 32, c, c, False, 1)
    assert size == (16, 16)
    ref, mag = R.fir_rows_ref(x.cpu(), n, 32, 32, c, TAPS, False, 1)
    R.assert_close_rows(down, ref, R.fir_bound(mag, False), 'down 32 -> 16')
    d = down.cuda().contiguous()
    up, size = _run_fir(mlib, d, n, 16, 16, c, c, True, 1)
    assert size == (32, 32)
    ref, mag = R.fir_rows_ref(down, n, 16, 16, c, TAPS, True, 1)
    R.assert_close_rows(up, ref, R.fir_bound(mag, True), 'up 16 -> 32')


@pytest.mark.parametrize('outer,h,w,inner', [(2, 5, 7, 12), (6, 32, 32, 1)], ids=['nhwc', 'nchw'])
def test_zero_border_is_exact(mlib, outer, h, w, inner):
    from diff_sampler_amd import _lib, _metrics_lib as ML
    x = torch.randn(outer, h, w, inner, generator=torch.Generator().manual_seed(5)).cuda()
    total = outer * (h + 2) * (w + 2) * inner
    outs = []
    for _ in range(2):
        buf = torch.full((total + 2 * 64,), float('nan'), dtype=torch.float32, device='cuda')
        out = buf[64:64 + total]
        ML.check(mlib.dsm_zero_border(_ptr(x), _ptr(out), outer, h, w, inner, 1, _lib.stream_ptr()), 'dsm_zero_border')
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[:64]).all()) and bool(torch.isnan(buf[64 + total:]).all()), 'guards were written'
        outs.append(out.clone().reshape(outer, h + 2, w + 2, inner))
    o = outs[0]
    assert torch.equal(o, outs[1])
    assert torch.equal(o[:, 1:-1, 1:-1], x), 'interior is not bit-equal'
    ring = o.clone()
    ring[:, 1:-1, 1:-1] = 0
    assert torch.equal(ring, torch.zeros_like(ring)) and not bool(torch.signbit(ring).any()), 'ring is not exactly +0'
