"""CPU: the case table of tests/_cm_wide_cases.py routes to the forms of the wide fp16-activation kernel it names (asked of the library's
host-only ds_conv_route), covers what its docstring claims, and its data meets the exactness conditions of family A (tests/_conv_refs.py), as
tests/test_conv_refs_cpu.py asserts them for the main table."""
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


@pytest.mark.parametrize('case', W.CASES, ids=lambda c: c.name)
def test_case_takes_the_route_it_names(case):
    a, _ = R.build(case)
    assert R.route(a) == R.expected_route(case), (case.name, R.route(a))
    assert case.kid == (2576 if case.ec0 else 2575) and case.w >= 128


def test_table_covers_what_it_claims():
    has = lambda pred: any(pred(c) for c in W.CASES)
    for h in (4, 8):
        for n in (1, 2):
            assert has(lambda c: c.w == 128 and c.h == h and c.n == n and c.ec0)
    for c0 in (64, 128):
        for ec0 in (64, 128):
            assert has(lambda c: c.c0 == c0 and c.ec0 == ec0)
    for cout, width in ((64, 1), (128, 2), (192, 3)):
        assert has(lambda c: c.cout == cout and c.widths == (width,) and c.ec0)
        assert has(lambda c: c.cout == cout and c.widths == (width,) and not c.ec0 and c.cbias)
    for out16 in (0, 1):
        for res in (0, 1):
            assert has(lambda c: c.ec0 and c.out16 == out16 and bool(c.res) == bool(res))
    assert has(lambda c: c.ec0 and c.cbias == 2 and c.n == 2) and has(lambda c: not c.ec0 and c.cbias == 2 and c.n == 2)
    assert has(lambda c: c.cbias == 1 and c.n == 2)                               # one row for two images
    assert has(lambda c: c.ec0 and c.stats and c.out16) and has(lambda c: c.ec0 and c.stats and not c.out16)
    assert has(lambda c: (c.n, c.h, c.w, c.c0, c.ec0, c.cout) == (1, 256, 256, 64, 64, 64))
    assert has(lambda c: 'B' in c.fam and c.ec0 and c.act and c.scale == R.B_SCALE)
    assert has(lambda c: c.res16 and c.ec0)


@pytest.mark.parametrize('case', [c for c in W.CASES if 'B' in c.fam], ids=lambda c: c.name)
def test_selectors_visit_every_tap_channel_position_and_the_appended_columns(case):
    v = R.selector_visits(case)
    assert v['taps'] == set(range(9)) and v['cpos'] == set(range(64)) and v['src'] == {0}
    assert v['esrc'] == ({0} if case.ec0 else set())


@pytest.mark.parametrize('case', [c for c in W.CASES if 'A' in c.fam and c.h < 256], ids=lambda c: c.name)
def test_family_a_data_meets_the_exactness_conditions(case):
    d = R.make_data(case, 'A')
    want, bound, stats = R.a_reference(case, d)
    assert bound is None
    c = R.conditions(case, d)
    assert c['units'] < 2 ** 24 and c['operands_fit'], c
    if case.mag == 'wide':
        assert c['every_slab_wide']
        if not case.out16:
            assert np.abs(want).max() > 4 * 2048                 # an fp16 accumulator would show
        else:
            exact = R.evaluate(case._replace(out16=0, stats=0), d)['out'].numpy()
            assert (exact != want).mean() > 0.05 and np.isfinite(want).all()
    if case.stats:
        s = R.block_sums(torch.from_numpy(np.abs(want)), want.shape[0], case.cout).numpy()
        assert s[:, 0].max() / case.scale < 2 ** 24 and s[:, 1].max() / case.scale ** 2 < 2 ** 24
    # a plain fp32 evaluation meets the criterion, and one that drops the appended columns does not
    assert np.array_equal(R.evaluate(case, d, torch.float32)['out'].double().numpy(), want)
    if case.ec0:
        assert not np.array_equal(R.evaluate(case, dict(d, we=np.zeros_like(d['we'])))['out'].numpy(), want)
    if case.cbias == 2:
        assert not np.array_equal(R.evaluate(case, d, mut=('cbias_neighbour',))['out'].numpy(), want)
