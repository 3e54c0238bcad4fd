"""GPU: every kernel behind ds_conv2d_nhwc and ds_gemm_nt_batched, element by element, on the case table of tests/_conv_refs.py.

Family A (integer operands): the output EQUALS the fp64 reference whatever the kernel's order of summation, its tile shape, its split-K
factor or its Winograd transform; fp16 rows equal rne16 of the exact value; stats_out is exact.  Family B (selector weights, randn inputs,
fused normalisation + SiLU, output SiLU): every element inside the derived bound.  Every launch runs on guarded buffers: NaN padding columns
in the sources, and NaN behind everything it may write -- output padding columns, rows beyond M, the block behind stats_out, the workspace
behind the planes it needs -- which must still be NaN afterwards.  The route is asserted before the launch.
tests/test_conv_refs_cpu.py proves the table's coverage and that these criteria bite."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _conv_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu


def _all_nan(t):
    return bool(torch.isnan(t).all())


def _launch(case, d):
    """Route check, launch, guard check -> (out [M, cout] fp64, stats [blocks, 2, cout] fp64 or None, raw fp32 / fp16 output tensor)."""
    from diff_sampler_amd import _lib
    lib = _lib.load()
    a, b = R.build(case, d, R.TorchAlloc('cuda'))
    assert R.route(a) == R.expected_route(case), (case.name, R.route(a))
    rc = lib.ds_conv2d_nhwc(C.byref(a), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, (case.name, lib.ds_error_string(rc))
    m = case.n * case.h * case.w
    out = b['out']
    if case.nchw:
        live = case.n * case.cout * case.h * case.w
        assert _all_nan(out[live:]), f'{case.name}: wrote behind the planar output'
        rows = out[:live].reshape(case.n, case.cout, case.h * case.w).permute(0, 2, 1).reshape(m, case.cout)
    else:
        assert _all_nan(out[:m, case.cout:]), f'{case.name}: wrote into the output padding columns'
        assert _all_nan(out[m:]), f'{case.name}: wrote rows beyond M'
        rows = out[:m, :case.cout]
    stats = None
    if case.stats:
        nblk = -(-m // 64)
        st = b['stats'].reshape(nblk + 1, 2, case.cout)
        assert _all_nan(st[nblk]), f'{case.name}: wrote behind the last statistics block'
        stats = st[:nblk].double().cpu().numpy()
    if case.ws:
        used = case.ws * m * case.cout
        assert _all_nan(b['ws'][used:]), f'{case.name}: wrote behind the workspace it was given'
        assert bool(torch.isfinite(b['ws'][:used]).all()), f'{case.name}: {case.splits} planes expected'
    for key, width in (('x', case.c0 + case.c1), ('e', case.ec0 + case.ec1)):          # the sources' NaN padding columns are still there
        if key in b:
            assert _all_nan(b[key][:, width:])
    rows = rows.contiguous()
    return rows.double().cpu().numpy(), stats, rows


def _check_stats(case, got, want):
    if R.stats_per_image(case):
        got, want = R.image_sums(got, case), R.image_sums(want, case)
    assert np.array_equal(got[:, 0], want[:, 0]), f'{case.name}: column sums differ in {int((got[:, 0] != want[:, 0]).sum())} places'
    if case.stats == 1:
        assert np.array_equal(got[:, 1], want[:, 1]), f'{case.name}: sums of squares differ in {int((got[:, 1] != want[:, 1]).sum())} places'
    else:
        assert (np.abs(got[:, 1] - want[:, 1]) <= R.squares_bound(want[:, 1])).all(), case.name


@pytest.mark.parametrize('name,fam,role', R.RUNS, ids=lambda v: str(v))
def test_conv_case(name, fam, role):
    case = R.CASE_BY_NAME[name]
    d = R.make_data(case, fam, role)
    if fam == 'A':
        want, bound, wstats = R.a_reference(case, d)
        got, gstats, _ = _launch(case, d)
        ok = R.a_inside(case, got, want, bound)
        if not ok.all():
            i = np.argwhere(~ok)[0]
            pytest.fail(f'{name}: {int((~ok).sum())} of {ok.size} elements differ from the exact result; first at row {i[0]} column {i[1]}: '
                        f'got {got[tuple(i)]!r} want {want[tuple(i)]!r}')
        if wstats is not None:
            _check_stats(case, gstats, wstats)
    else:
        ref = R.b_reference(case, d)
        got, _, _ = _launch(case, d)
        ok = R.b_inside(case, got, ref)
        if not ok.all():
            i = tuple(np.argwhere(~ok)[0])
            pytest.fail(f'{name}: {int((~ok).sum())} of {ok.size} elements outside the bound; first at {i}: got {got[i]!r} '
                        f'ref [{ref[0][i]!r}, {ref[1][i]!r}] bound {ref[2][i]!r}')


def test_every_kernel_that_can_run_one_layer_returns_the_same_bits():
    """One family-A layer on the generic, 128 / 1284 / 256 / 2565 tiles, the Winograd form and the split-fp16 kernel: each equals the
    reference, so all agree; stated separately because a failure here names the pair."""
    cases = R.agree_cases()
    wino = [c for c in cases if c.wino][0]
    d = R.make_data(wino, 'A')                   # weights multiples of 4, every slab of 8 channels with 13-bit activations
    want = R.a_reference(wino, d)[0]
    outs = {}
    for c in cases:
        got, _, raw = _launch(c, d)
        outs[c.name] = raw.cpu()
        assert np.array_equal(got, want), f'{c.name} differs from the exact result in {int((got != want).sum())} places'
    names = list(outs)
    for i, p in enumerate(names):
        for q in names[i + 1:]:
            assert torch.equal(outs[p], outs[q]), (p, q)


@pytest.mark.parametrize('case', R.GEMM_CASES, ids=lambda c: c.name)
def test_gemm_nt_batched_case(case):
    """ds_gemm_nt_batched with the attention strides (heads side by side in a row), ragged m and n, ldc > n, NaN guards."""
    from diff_sampler_amd import ops
    d = R.gemm_data(case)
    want, bound, _ = R.gemm_reference(case, d)
    dev = 'cuda'
    ld = case.heads * case.k + 8
    ldc = R.ceil_to(case.n, 4) + 4

    def rows(v, r):
        t = torch.full((case.batch, r, ld), float('nan'), device=dev)
        t[:, :, :case.heads * case.k] = torch.from_numpy(v.reshape(case.batch, r, -1)).float().to(dev)
        return t
    a, b = rows(d['a'], case.m), rows(d['b'], case.n)
    c = torch.full((case.batch * case.heads * case.m + R.SPARE_ROWS, ldc), float('nan'), device=dev)
    rb = torch.from_numpy(d['rowbias']).float().to(dev) if case.rowbias else None
    cb = torch.from_numpy(d['colbias']).float().to(dev) if case.colbias else None
    ops.gemm_nt_batched(a, ld, b, ld, c, ldc, case.m, case.n, case.k, batch=case.batch, heads=case.heads, a_bs=case.m * ld, a_hs=case.k,
                        b_bs=case.n * ld, b_hs=case.k, c_bs=case.heads * case.m * ldc, c_hs=case.m * ldc, alpha=case.alpha, rowbias=rb,
                        colbias=cb, act=case.act)
    torch.cuda.synchronize()
    live = case.batch * case.heads * case.m
    assert _all_nan(c[:live, case.n:]) and _all_nan(c[live:]), f'{case.name}: wrote outside C'
    got = c[:live, :case.n].reshape(case.batch, case.heads, case.m, case.n).double().cpu().numpy()
    ok = (got == want) if bound is None else R.inside(got, want, bound)
    assert ok.all(), f'{case.name}: {int((~ok).sum())} of {ok.size} elements; {R.worst(got, want, 0.0 if bound is None else bound)}'
