"""GPU: the solver-side kernels (csrc/solver.hip) and the glue kernels of csrc/norm_act.hip away from the bundled networks' geometry --
every kernel ds_solver_update can launch in every operand mode, both trips of the grid-stride loops, the quantile kernels at general
sample sizes up to the LDS cap, and the small copy / fill / select / quantise / im2col / mean / softmax kernels at odd sizes.

References and per-element bounds: tests/_kernel_refs.py (fp64 on the CPU; checked by tests/test_kernel_refs_cpu.py).  Every output buffer
is pre-filled with NaN and is longer than the kernel may write; what lies outside the result (guard floats, padding columns of a leading
dimension) must still be NaN afterwards."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

import _kernel_refs as R  # noqa: E402
from oracle import solvers_ref  # noqa: E402

DS_E_ARG, DS_E_ALIGN, DS_E_SHAPE = -1, -2, -3
TOL = 2e-5
NAN = float('nan')
GUARD = 4                # floats behind (and, for an offset view, in front of) every result


def _nan_out(numel, offset=0):
    """(whole NaN-filled device allocation, view of `numel` floats starting `offset` floats into it)."""
    buf = torch.full((offset + numel + GUARD,), NAN, device='cuda')
    return buf, buf[offset:offset + numel]


def _guards_nan(buf, numel, offset=0):
    return bool(torch.isnan(buf[:offset]).all()) and bool(torch.isnan(buf[offset + numel:]).all())


def _dev(t, offset=0):
    """A CPU fp32 tensor on the device, as a contiguous view starting `offset` floats into its allocation."""
    buf = torch.empty(offset + t.numel(), device='cuda')
    v = buf[offset:].view(t.shape)
    v.copy_(t)
    return v


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# =============================================================================================================== 1. ds_solver_update

def _run_update(case, d=None):
    """Launch one case of tests/_kernel_refs.UPDATE_CASES; returns (m, x') on the CPU (None where the case does not ask for it) after
    checking that nothing outside the results was written."""
    from diff_sampler_amd import ops
    d = R.update_inputs(case) if d is None else d
    n, c, h, w = case.n, case.c, case.h, case.w
    numel = n * c * h * w
    off = lambda name: 1 if case.misalign == name else 0
    xe = _dev(d['xe'], off('xe'))
    xb = _dev(d['xb'], 0) if case.xb_distinct else xe
    f_ld = R.update_f_ld(case)
    f = None if case.mode == 'afs' else _dev(R.nhwc_rows(d['f'], f_ld) if f_ld else d['f'], off('f'))
    hist = [_dev(t, 1 if (case.misalign == 'hist1' and i == 1) else 0) for i, t in enumerate(d['hist'])]
    mbuf, m_out = _nan_out(numel, off('m_out'))
    xbuf, x_out = _nan_out(numel, off('x_out'))
    want_m, want_x = case.outs in ('m', 'both'), case.outs in ('x', 'both')
    kw = dict(raw=case.mode in ('raw4', 'raw8', 'planar'), f_ld=f_ld, hist=hist, afs=case.mode == 'afs', sigma_data=d['sigma_data'],
              m_out=m_out if want_m else None, store_d=bool(case.store_d))
    if case.coef == 'host':
        kw['hcoefs'] = d['coefs'][0].tolist()
    else:
        rows = case.n if case.coef == 'devn' else 1
        kw.update(coefs=d['coefs'][:rows].contiguous().cuda(), coef_rows=rows)
    a = ops.make_update_args(xe, xb, f, n, c, h, w, x_out if want_x else None, **kw)
    ops.solver_update(a)
    torch.cuda.synchronize()
    assert _guards_nan(mbuf, numel if want_m else 0, off('m_out')), 'm_out: written outside the result'
    assert _guards_nan(xbuf, numel if want_x else 0, off('x_out')), 'x_out: written outside the result'
    shape = (n, c, h, w)
    return (m_out.cpu().view(shape) if want_m else None), (x_out.cpu().view(shape) if want_x else None)


def _check_update(case, m, x, d=None):
    d = R.update_inputs(case) if d is None else d
    m_ref, x_ref, m_bnd, x_bnd = R.solver_update_ref(d['xe'], d['xb'], d['f'], d['hist'], d['coefs'], d['sigma_data'], case.mode, case.store_d)
    if m is not None:
        err = (m.double() - m_ref).abs()
        print(f'{case.name}: m  worst {float((err / (m_bnd / 8).clamp_min(1e-300)).max()):.2f} units of 2^-24 M (bound 8)')
        assert bool((err <= m_bnd).all()), (case, int((~(err <= m_bnd)).sum()))
    if x is not None:
        err = (x.double() - x_ref).abs()
        print(f'{case.name}: x\' worst {float((err / (x_bnd / 16).clamp_min(1e-300)).max()):.2f} units (bound 16)')
        assert bool((err <= x_bnd).all()), (case, int((~(err <= x_bnd)).sum()))


@pytest.mark.parametrize('case', R.UPDATE_CASES, ids=[c.name for c in R.UPDATE_CASES])
def test_solver_update_every_kernel_against_fp64(case):
    """fast<3> / fast<4>, the generic 16-byte kernel, the scalar kernel (by shape) and the second trip of each grid-stride loop: m and x'
    within the per-element bounds of the fp64 reference, nothing written outside them."""
    m, x = _run_update(case)
    _check_update(case, m, x)


@pytest.mark.parametrize('operand', R.MISALIGNED_OPERANDS)
def test_solver_update_scalar_kernel_by_alignment_equals_the_aligned_run(operand):
    """One operand one float into its allocation sends the launch to the scalar kernel; outside AFS both kernels go through ds_upd_element,
    so the result equals the aligned (streaming-kernel) run bit for bit."""
    base = R.MISALIGN_BASE
    d = R.update_inputs(base)
    m0, x0 = _run_update(base, d)
    _check_update(base, m0, x0, d)
    m1, x1 = _run_update(base._replace(misalign=operand), d)
    assert _bits_equal(m1, m0) and _bits_equal(x1, x0)


@pytest.mark.parametrize('operand', ['xe', 'hist1', 'x_out'])
def test_solver_update_scalar_kernel_by_alignment_afs(operand):
    case = R.MISALIGN_AFS._replace(misalign=operand)
    m, x = _run_update(case)
    _check_update(case, m, x)


def test_solver_update_refuses_bad_arguments_and_writes_nothing():
    from diff_sampler_amd import _lib, ops
    lib = _lib.load()
    case = R._u('args', (3, 2, 2), 'raw4', 1, 0, 'both', 1, 'devn')
    d = R.update_inputs(case)
    xe, f, h0 = _dev(d['xe']), _dev(R.nhwc_rows(d['f'], 4)), _dev(d['hist'][0])
    coefs = d['coefs'].cuda()
    numel = d['xe'].numel()
    mbuf, m_out = _nan_out(numel)
    xbuf, x_out = _nan_out(numel)

    def rc(**over):
        kw = dict(raw=True, f_ld=4, hist=[h0], coefs=coefs, coef_rows=3, m_out=m_out, store_d=True)
        xo = over.pop('x_out', x_out)
        kw.update(over)
        a = ops.make_update_args(xe, xe, f, 3, 3, 2, 2, xo, **kw)
        code = lib.ds_solver_update(C.byref(a), _lib.stream_ptr())
        torch.cuda.synchronize()
        return code

    assert rc(f_ld=2) == DS_E_ARG                                  # raw rows shorter than the channel count
    assert rc(coef_rows=2) == DS_E_ARG and rc(coef_rows=0) == DS_E_ARG and rc(coef_rows=4) == DS_E_ARG
    assert rc(x_out=None, m_out=None) == DS_E_ARG                  # nothing to write
    assert bool(torch.isnan(mbuf).all()) and bool(torch.isnan(xbuf).all())
    with pytest.raises(_lib.DsError, match='code -1'):
        ops.solver_update(ops.make_update_args(xe, xe, f, 3, 3, 2, 2, None, raw=True, f_ld=4, coefs=coefs, coef_rows=3))
    assert rc() == 0                                               # the same call with valid arguments runs
    assert not bool(torch.isnan(m_out).any()) and not bool(torch.isnan(x_out).any())


# =============================================================================================================== 2. quantile kernels

_QREF = {}


def _threshold_ref(kind, per):
    """(input [4, per], torch.quantile thresholding of it on the CPU), computed once per (kind, per)."""
    if (kind, per) not in _QREF:
        x = R.quantile_inputs(kind, per)
        _QREF[kind, per] = (x, solvers_ref.threshold(x.reshape(4, per, 1, 1), R.QUANTILE_P).reshape(4, per))
    return _QREF[kind, per]


@pytest.mark.parametrize('per', R.QUANTILE_PERS)
def test_dynamic_threshold_general_sizes_bit_exact(per):
    """Fewer values than threads, sizes that are no multiple of the block, an integer rank (per = 201, 1001: hi == lo), the LDS cap."""
    from diff_sampler_amd import ops
    for kind in R.QUANTILE_KINDS:
        x, ref = _threshold_ref(kind, per)
        buf, out = _nan_out(4 * per)
        ops.dynamic_threshold(_dev(x), out, 4, per, R.QUANTILE_P)
        torch.cuda.synchronize()
        got = out.cpu().view(4, per)
        assert _bits_equal(got, ref), (kind, per, int((got.view(torch.int32) != ref.view(torch.int32)).sum()))
        assert _guards_nan(buf, 4 * per), (kind, per)


def test_dynamic_threshold_refuses_a_sample_beyond_the_lds_cap():
    from diff_sampler_amd import _lib, ops
    per = R.QUANTILE_LDS_CAP + 1
    x = _dev(R.quantile_inputs('gauss3', per))
    buf, out = _nan_out(4 * per)
    rc = _lib.load().ds_dynamic_threshold(C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), 4, per, R.QUANTILE_P, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == DS_E_SHAPE and bool(torch.isnan(buf).all())
    with pytest.raises(_lib.DsError, match='code -3'):
        ops.dynamic_threshold(x, out, 4, per, R.QUANTILE_P)


def _x0_step(shape, kind, variant, nhist, coef, lib_call=False, hist3=False):
    """ds_dpmpp_x0_step on a given denoised tensor (non-raw: D is the input itself, so m must equal torch.quantile thresholding to the bit).
    Returns (m, x', m_ref, x'_ref, bound on |x' - x'_ref|) or, with lib_call, (return code, whether both outputs are still all NaN)."""
    from diff_sampler_amd import _lib, ops
    c, h, w = shape
    per, n = c * h * w, 4
    f, m_ref = _threshold_ref(kind, per)
    g = torch.Generator().manual_seed(2500 + per)
    xb = torch.randn(n, per, generator=g) * 3
    hist = [torch.randn(n, per, generator=g) for _ in range(3 if hist3 else nhist)]
    case = R._u('x0', shape, 'nonraw', nhist, 1, 'both', 0, coef, n=n)
    coefs = R.update_inputs(case, seed=per)['coefs']
    mbuf, m_out = _nan_out(n * per)
    xbuf, x_out = _nan_out(n * per)
    kw = dict(hcoefs=coefs[0].tolist()) if coef == 'host' else dict(coefs=coefs[:n if coef == 'devn' else 1].contiguous().cuda(),
                                                                    coef_rows=n if coef == 'devn' else 1)
    fd = _dev(f)
    a = ops.make_update_args(fd, _dev(xb), fd, n, c, h, w, x_out, raw=False, f_ld=0, hist=[_dev(t) for t in hist], m_out=m_out,
                             store_d=False, **kw)
    a.variant = variant
    if lib_call:
        rc = _lib.load().ds_dpmpp_x0_step(C.byref(a), R.QUANTILE_P, _lib.stream_ptr())
        torch.cuda.synchronize()
        return rc, bool(torch.isnan(mbuf).all()) and bool(torch.isnan(xbuf).all())
    ops.dpmpp_x0_step(a, R.QUANTILE_P)
    torch.cuda.synchronize()
    assert _guards_nan(mbuf, n * per) and _guards_nan(xbuf, n * per)
    k = coefs.double()
    x_ref = k[:, 0:1] * xb.double() + k[:, 1:2] * m_ref.double()
    mag = (k[:, 0:1] * xb.double()).abs() + (k[:, 1:2] * m_ref.double()).abs()
    for j, t in enumerate(hist[:nhist]):
        x_ref = x_ref + k[:, 2 + j:3 + j] * t.double()
        mag = mag + (k[:, 2 + j:3 + j] * t.double()).abs()
    return m_out.cpu().view(n, per), x_out.cpu().view(n, per), m_ref, x_ref, 16 * R.U * mag


@pytest.mark.parametrize('shape,nhist,coef', [((5, 3, 7), 2, 'devn'), ((1, 1, 2), 0, 'host'), ((3, 5, 5), 1, 'dev1'),
                                              ((1, 2, R.QUANTILE_LDS_CAP // 2), 2, 'devn')])
def test_dpmpp_x0_step_lds_kernel_general_sizes(shape, nhist, coef):
    for kind in R.QUANTILE_KINDS:
        m, x, m_ref, x_ref, x_bnd = _x0_step(shape, kind, 1, nhist, coef)
        assert _bits_equal(m, m_ref), (shape, kind)
        assert bool(((x.double() - x_ref).abs() <= x_bnd).all()), (shape, kind)


def test_dpmpp_x0_step_register_kernel_with_per_sample_coefficients():
    from diff_sampler_amd import _lib
    shape = R.X0_STEP_REG_SHAPE
    assert _lib.load().ds_dpmpp_x0_step_in_registers(shape[0] * shape[1] * shape[2]) == 1
    for kind in R.QUANTILE_KINDS:
        m, x, m_ref, x_ref, x_bnd = _x0_step(shape, kind, 0, 2, 'devn')
        assert _bits_equal(m, m_ref), kind
        assert bool(((x.double() - x_ref).abs() <= x_bnd).all()), kind


def test_dpmpp_x0_step_refuses_a_third_history_tensor_and_oversized_samples():
    """x' combines m0 with hist[0] and hist[1] only: a third history tensor is an argument error (it used to be dropped silently, on the
    LDS kernel it forced).  A sample beyond the LDS cap is a shape error.  Neither writes anything."""
    for shape, variant in (((3, 16, 16), 0), ((3, 16, 16), 1), ((5, 3, 7), 0)):
        rc, untouched = _x0_step(shape, 'gauss3', variant, 2, 'host', lib_call=True, hist3=True)
        assert rc == DS_E_ARG and untouched, (shape, variant)
    rc, untouched = _x0_step((1, 1, R.QUANTILE_LDS_CAP + 1), 'gauss3', 1, 1, 'host', lib_call=True)
    assert rc == DS_E_SHAPE and untouched


# =============================================================================================================== 4. glue kernels

@pytest.mark.parametrize('count', [1, 2, 3, 5, 1023, 4 * 256 * 4096 + 7])
def test_scale_counts_and_tail(count):
    from diff_sampler_amd import ops
    x = torch.randn(count, generator=torch.Generator().manual_seed(count)) * 3
    xd = _dev(x)
    buf, y = _nan_out(count)
    ops.scale(xd, 1.7, y)
    torch.cuda.synchronize()
    assert _bits_equal(y.cpu(), x * torch.tensor(1.7)) and _guards_nan(buf, count)


def test_scale_refuses_misaligned_views():
    from diff_sampler_amd import _lib, ops
    x = _dev(torch.randn(64))
    buf, y = _nan_out(64, offset=1)
    with pytest.raises(_lib.DsError, match='code -2'):
        ops.scale(x, 2.0, y)
    with pytest.raises(_lib.DsError, match='code -2'):
        ops.scale(_dev(torch.randn(64), 1), 2.0, buf[:64])
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())


@pytest.mark.parametrize('count', [1, 255, 257, 256 * 4096 + 3])
def test_fill_counts(count):
    from diff_sampler_amd import ops
    buf, dst = _nan_out(count + 5)
    ops.fill(dst, -2.75, count)
    torch.cuda.synchronize()
    assert bool((dst[:count] == -2.75).all()) and bool(torch.isnan(buf[count:]).all())


@pytest.mark.parametrize('rows,cols,src_ld,dst_ld', [(1, 1, 1, 1), (5, 7, 9, 8), (3, 64, 64, 70), (1031, 1021, 1021, 1024)])
def test_copy_rows(rows, cols, src_ld, dst_ld):
    from diff_sampler_amd import ops
    assert rows != 1031 or rows * cols > 256 * 4096
    src = torch.randn(rows, src_ld, generator=torch.Generator().manual_seed(rows))
    buf, dst = _nan_out(rows * dst_ld)
    ops.copy_rows(_dev(src), src_ld, dst, dst_ld, rows, cols)
    torch.cuda.synchronize()
    got = dst.cpu().view(rows, dst_ld)
    assert _bits_equal(got[:, :cols], src[:, :cols])
    assert bool(torch.isnan(got[:, cols:]).all()) and _guards_nan(buf, rows * dst_ld)


def test_table_select_steps_and_repeats():
    from diff_sampler_amd import ops
    table = torch.randn(5, 70, generator=torch.Generator().manual_seed(5))
    td = _dev(table)
    step = torch.zeros(1, dtype=torch.int32, device='cuda')
    for s in range(5):
        buf, dst = _nan_out(70)
        ops.table_select(td, 70, step, 1, dst)
        torch.cuda.synchronize()
        assert _bits_equal(dst.cpu(), table[s]) and _guards_nan(buf, 70) and int(step) == s + 1
    assert int(step) == 5
    step.fill_(3)
    for _ in range(2):
        buf, dst = _nan_out(70)
        ops.table_select(td, 70, step, 0, dst)
        torch.cuda.synchronize()
        assert _bits_equal(dst.cpu(), table[3]) and _guards_nan(buf, 70) and int(step) == 3


@pytest.mark.parametrize('n,c,h,w', [(2, 1, 31, 35), (2, 3, 31, 35), (1, 4, 33, 35), (1, 1, 1025, 1025)])
def test_quantize_u8_nhwc_edges(n, c, h, w):
    """Inputs on and next to every quantisation step, below -1 and above 1, odd H*W; (1, 1, 1025, 1025): the second trip.  The reference
    rounds the product and the sum separately (ATen), which decides the inputs that land exactly on an integer."""
    from diff_sampler_amd import ops
    assert (h * w) % 2 == 1 and (n != 1 or c != 1 or n * h * w > 256 * 4096)
    x = R.quantize_inputs(n, c, h, w)
    out = torch.full((n * h * w * c + 16,), 77, dtype=torch.uint8, device='cuda')
    ops.quantize_u8_nhwc(_dev(x), out, n, c, h, w)
    torch.cuda.synchronize()
    got = out.cpu()
    ref = R.quantize_ref(x)
    assert torch.equal(got[:ref.numel()].view(ref.shape), ref), int((got[:ref.numel()].view(ref.shape) != ref).sum())
    assert bool((got[ref.numel():] == 77).all())


@pytest.mark.parametrize('n,c,h,w,kpad,per_sample', [(2, 3, 5, 7, 32, True), (1, 4, 4, 4, 64, False), (3, 3, 1, 1, 32, True),
                                                     (2, 7, 3, 2, 64, False), (9, 3, 86, 86, 32, True)])
def test_stem_im2col(n, c, h, w, kpad, per_sample):
    from diff_sampler_amd import ops
    assert n != 9 or n * h * w * kpad > 8192 * 256
    g = torch.Generator().manual_seed(n * 100 + c)
    x = torch.randn(n, c, h, w, generator=g) * 2
    sigma = torch.exp(torch.rand(n if per_sample else 1, generator=g) * 6 - 3)
    buf, out = _nan_out(n * h * w * kpad)
    ops.stem_im2col(_dev(x), _dev(sigma), sigma.numel(), 0.5, n, c, h, w, out, kpad)
    torch.cuda.synchronize()
    got = out.cpu().view(n * h * w, kpad)
    ref = R.stem_im2col_ref(x, sigma, 0.5, kpad)
    zero = ref == 0
    assert bool(zero[:, 9 * c:].all()) and int(zero[:, :9 * c].sum()) > 0            # pad columns and border taps
    assert bool((got[zero].view(torch.int32) == 0).all())                            # exactly +0.0
    assert bool(((got.double() - ref).abs() <= 4 * R.U * ref.abs()).all())
    assert _guards_nan(buf, n * h * w * kpad)


@pytest.mark.parametrize('c', [1, 63, 64, 65, 320])
def test_channel_mean_fp32(c):
    from diff_sampler_amd import ops
    for ld in (c, c + 4):
        for rows in (1, 5, 4097):
            g = torch.Generator().manual_seed(c * 7 + rows)
            x = torch.full((rows, ld), NAN)                       # padding columns hold NaN: reading one poisons the row's mean
            x[:, :c] = torch.randn(rows, c, generator=g) * 3 + 0.5
            buf, out = _nan_out(rows)
            ops.channel_mean(_dev(x), ld, c, rows, out)
            torch.cuda.synchronize()
            ref = x[:, :c].double().mean(-1)
            err = (out.cpu().double() - ref).abs()
            assert bool((err <= R.channel_mean_bound(x[:, :c], c)).all()), (c, ld, rows)
            assert _guards_nan(buf, rows)


@pytest.mark.parametrize('in_place', [False, True])
@pytest.mark.parametrize('rows,cols,ld', R.SOFTMAX_SHAPES)
def test_softmax_rows(rows, cols, ld, in_place):
    from diff_sampler_amd import ops
    x = torch.full((rows, ld), NAN)
    x[:, :cols] = R.softmax_inputs(rows, cols)
    xd = _dev(x)
    if in_place:
        buf, y = None, xd
    else:
        buf, y = _nan_out(rows * ld)
    ops.softmax_rows(xd, y, rows, cols, ld)
    torch.cuda.synchronize()
    got = y.cpu().view(rows, ld)
    ref = x[:, :cols].double().softmax(-1)
    err = (got[:, :cols].double() - ref).abs().amax(-1) / ref.amax(-1)
    assert bool((err < TOL).all()), err
    assert bool(((got[:, :cols].double().sum(-1) - 1).abs() < 1e-5).all())
    assert bool(torch.isnan(got[:, cols:]).all())
    assert buf is None or _guards_nan(buf, rows * ld)
