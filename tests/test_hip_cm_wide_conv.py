"""GPU: the U-Net block forms of the wide fp16-activation 3x3 kernel (csrc/conv3x3_f16wide.hip: appended 1x1 columns, kernel id 2576, and
the per-image bias row), element by element on the case table of tests/_cm_wide_cases.py.  Family A: equality with the fp64 evaluation
(statistics too); family B: the per-element bound of tests/_conv_refs.py.  Guards around every buffer as in tests/test_hip_conv_kernels.py."""
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
import _cm_wide_cases as W  # noqa: E402

pytestmark = pytest.mark.gpu


def _all_nan(t):
    return bool(torch.isnan(t).all())


def _launch(case, d):
    from diff_sampler_amd import _lib
    lib = _lib.load()
    a, b = R.build(case, d, R.TorchAlloc('cuda'))
    assert R.route(a) == R.expected_route(case), (case.name, R.route(a))
    rc = lib.ds_conv2d_nhwc(C.byref(a), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, (case.name, lib.ds_error_string(rc))
    m = case.n * case.h * case.w
    out = b['out']
    assert _all_nan(out[:m, case.cout:]), f'{case.name}: wrote into the output padding columns'
    assert _all_nan(out[m:]), f'{case.name}: wrote rows beyond M'
    stats = None
    if case.stats:
        nblk = m // 64
        st = b['stats'].reshape(nblk + 1, 2, case.cout)
        assert _all_nan(st[nblk]), f'{case.name}: wrote behind the last statistics block'
        stats = st[:nblk].double().cpu().numpy()
    for key, width in (('x', case.c0), ('e', case.ec0)):
        if key in b:
            assert _all_nan(b[key][:, width:])
    return out[:m, :case.cout].contiguous().double().cpu().numpy(), stats


@pytest.mark.parametrize('name,fam', W.RUNS, ids=lambda v: str(v))
def test_wide_block_conv_case(name, fam):
    case = W.CASE_BY_NAME[name]
    d = R.make_data(case, fam)
    if fam == 'A':
        want, bound, wstats = R.a_reference(case, d)
        assert bound is None
        got, gstats = _launch(case, d)
        ok = got == want
        if not ok.all():
            i = np.argwhere(~ok)[0]
            pytest.fail(f'{name}: {int((~ok).sum())} of {ok.size} elements differ from the exact result; first at row {i[0]} column {i[1]}: '
                        f'got {got[tuple(i)]!r} want {want[tuple(i)]!r}')
        if wstats is not None:
            assert np.array_equal(gstats[:, 0], wstats[:, 0]), f'{name}: column sums differ'
            assert np.array_equal(gstats[:, 1], wstats[:, 1]), f'{name}: sums of squares differ'
    else:
        ref = R.b_reference(case, d)
        got, _ = _launch(case, d)
        ok = R.b_inside(case, got, ref)
        if not ok.all():
            i = tuple(np.argwhere(~ok)[0])
            pytest.fail(f'{name}: {int((~ok).sum())} of {ok.size} elements outside the bound; first at {i}: got {got[i]!r} '
                        f'ref [{ref[0][i]!r}, {ref[1][i]!r}] bound {ref[2][i]!r}')
