"""CPU: the case table of tests/_conv_refs.py reaches every kernel, reduce kernel, column-range form and operand form it names (asked of the
library's own host-only ds_conv_route), the data of every case meets the conditions that make equality the criterion, a plain fp32 torch
evaluation of every case passes the criterion, and each of a list of deliberate defects of that evaluation fails it on a named case."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _conv_refs as R  # noqa: E402

CASES = R.CASES
BY = R.CASE_BY_NAME
_CACHE = {}


def _run(name, fam, role=0):
    """(case, data, reference) of a run, computed once and never written to."""
    key = (name, fam, role)
    if key not in _CACHE:
        case = BY[name]
        d = R.make_data(case, fam, role)
        ref = R.a_reference(case, d) if fam == 'A' else R.b_reference(case, d)
        _CACHE[key] = (case, d, ref)
    return _CACHE[key]


def _passes(case, fam, ref, r):
    """The criterion on an evaluation r = dict(out, stats) -> (output ok, statistics ok)."""
    got = r['out'].double().numpy()
    if fam == 'B':
        return bool(R.b_inside(case, got, ref).all()), True
    want, bound, stats = ref
    ok = bool((R.a_inside(case, got, want, bound)).all())
    sok = True
    if stats is not None:
        gs = r['stats'].double().numpy()
        sok = bool((gs[:, 0] == stats[:, 0]).all())
        sok = sok and (bool((gs[:, 1] == stats[:, 1]).all()) if case.stats == 1 else
                       bool((np.abs(gs[:, 1] - stats[:, 1]) <= R.squares_bound(stats[:, 1])).all()))
    return ok, sok


# ------------------------------------------------------------------------------------------------------------------------------
# routes and coverage

@pytest.mark.parametrize('case', list(CASES) + R.agree_cases(), ids=lambda c: c.name)
def test_case_takes_the_route_it_names(case):
    a, _ = R.build(case)
    assert R.route(a) == R.expected_route(case), case.name


def _where(pred):
    return [c for c in CASES if pred(c)]


def test_every_kernel_id_and_the_winograd_form():
    assert {c.kid for c in CASES} == set(R.KERNEL_IDS)
    assert _where(lambda c: c.wino)
    for kid in R.KERNEL_IDS:
        fams = ''.join(c.fam for c in CASES if c.kid == kid)
        assert 'A' in fams, kid
        assert 'B' in fams, kid


def test_split_k_on_each_reduce_path_with_and_without_statistics():
    for kid in (0, 128, 256, 1284, 2566):
        sk = _where(lambda c: c.kid == kid and c.splits > 1 and not c.up2)
        assert sk and any(c.stats for c in sk) and any(not c.stats for c in sk), kid
        assert all(c.ws == c.splits for c in sk)                    # the workspace is exactly the planes the launch needs
    assert _where(lambda c: c.kid == 128 and c.splits > 1 and c.cout % 4)                          # ragged cout: scalar partial store
    assert any(c.out16 for c in _where(lambda c: c.kid == 2566 and c.splits > 1))                  # splitk_reduce_f16, fp16 rows


def test_column_ranges():
    assert _where(lambda c: c.kid == 128 and c.cout > 128 and 0 < c.cout % 128 <= 64)               # 128 + 64-column tail
    assert _where(lambda c: c.kid == 256 and c.cout > 128 and 0 < c.cout % 128 <= 64)
    assert _where(lambda c: c.kid == 2565 and c.cout == 320 and not c.wino)                        # 256 + 64
    assert _where(lambda c: c.kid == 2575 and len(set(c.widths)) == 2)                             # two tile widths
    assert _where(lambda c: c.kid == 2566 and len(set(c.widths)) == 2)
    assert _where(lambda c: c.kid == 2568) and _where(lambda c: c.kid == 1284)                     # 192-column tiles, half-size waves


def test_pixel_tiles():
    tile = {128: 128, 1284: 128, 256: 256, 2565: 256, 2568: 256, 2566: 256, 2572: 256}
    halo = _where(lambda c: c.kid in tile and not c.up2)
    assert [c for c in halo if c.h * c.w < tile[c.kid] and c.n > 1]                                 # several images per tile
    assert [c for c in halo if (c.n * c.h * c.w) % tile[c.kid]]                                    # ragged last tile
    assert [c for c in halo if c.h != c.w]
    assert [c for c in halo if c.w == 4] and [c for c in halo if c.w == 64]
    assert _where(lambda c: c.kid == 2566 and c.h * c.w == 64 and c.n % 4 == 1)                    # last tile holds one image
    assert _where(lambda c: c.kid == 2561 and (c.n * c.h * c.w) % 256 and c.cout % 128)            # ragged M and N


def test_operand_forms():
    assert _where(lambda c: c.c1 and c.kind == 'f32' and c.taps == 9) and _where(lambda c: c.c1 and c.taps == 1)
    assert _where(lambda c: c.ec0 and not c.ec1) and _where(lambda c: c.ec1)
    for kid in (128, 1284, 2565, 2568):
        assert _where(lambda c: c.up2 and c.kid == kid), kid
    assert _where(lambda c: c.stride == 2 and c.kind == 'f32') and _where(lambda c: c.stride == 2 and c.kind == 'f16')
    assert _where(lambda c: c.nchw and c.kid == 0) and _where(lambda c: c.nchw and c.kid == 2570) and _where(lambda c: not c.nchw and c.kid == 2570)
    assert _where(lambda c: c.kid == 2570 and c.norm) and _where(lambda c: c.kid == 2570 and not c.norm)
    assert {R.scalar_epilogue(c) for c in CASES} >= {'out_ld', 'res_ld', 'bias'}
    assert _where(lambda c: c.kind == 'split' and 'A' in c.fam)
    assert [r for r in R.RUNS if r[2] == 1]                                                         # split-fp16: the run with wide weights


OPTIONS = dict(bias=dict(bias=1), cbias1=dict(cbias=1), cbiasn=dict(cbias=2), res=dict(res=1), scale=dict(scale=0.5), act=dict(act=1),
               res16=dict(res=1, res16=1), out16=dict(out16=1))


@pytest.mark.parametrize('kid,wino', [(k, 0) for k in R.KERNEL_IDS] + [(2565, 1)])
def test_each_optional_operand_a_kernel_accepts_is_once_present_and_once_absent(kid, wino):
    """What a kernel accepts is asked of the route: a bare case of the kernel with ONE option switched on must keep its kernel id; an option
    the route refuses (or sends to another kernel) needs no case -- the refusal is what is asserted."""
    mine = [c for c in CASES if c.kid == kid and c.wino == wino]
    bare = mine[0]._replace(bias=0, cbias=0, res=0, scale=1.0, act=0, res16=0, out16=0, stats=0, fam='A')
    for opt, kw in OPTIONS.items():
        rc, got_kid, _, got_wino, _ = R.route(R.build(bare._replace(**kw))[0])
        accepted = rc == 0 and got_kid == kid and got_wino == wino
        present = [c for c in mine if opt in R.options(c)]
        if not accepted:
            assert not present, (kid, opt)
            continue
        if opt == 'cbiasn':
            present = [c for c in present if c.n > 1]          # n rows of one image are the one-row form
        assert present, f'kernel {kid}: no case with {opt}'
        assert [c for c in mine if opt not in R.options(c)], f'kernel {kid}: no case without {opt}'


@pytest.mark.parametrize('case', [c for c in CASES if 'B' in c.fam], ids=lambda c: c.name)
def test_selectors_visit_every_tap_channel_position_and_source(case):
    g = R.geo(case)
    v = R.selector_visits(case)
    assert v['taps'] == set(range(case.taps)), case.name
    assert v['cpos'] == set(range(g['slab'])), case.name
    assert v['src'] == ({0, 1} if case.c1 else {0})
    assert v['esrc'] == ({0, 1} if case.ec1 else ({0} if case.ec0 else set()))
    for rnd in range(case.rounds):
        d = R.make_data(case, 'B', rnd)
        nz = (d['w'].reshape(case.cout, -1) != 0).sum(1) + ((d['we'] != 0).sum(1) if d['we'] is not None else 0)
        assert (nz == 1).all()                                    # exactly one non-zero weight per column


# ------------------------------------------------------------------------------------------------------------------------------
# family A: the conditions, on the data of every run

A_RUNS = [r for r in R.RUNS if r[1] == 'A']
B_RUNS = [r for r in R.RUNS if r[1] == 'B']


@pytest.mark.parametrize('name,fam,role', A_RUNS, ids=lambda v: str(v))
def test_family_a_data_meets_the_exactness_conditions(name, fam, role):
    case, d, (want, bound, stats) = _run(name, fam, role)
    c = R.conditions(case, d, role)
    assert c['units'] < 2 ** 24, c
    assert c['operands_fit'], name
    if case.wino:
        assert c['wino_u_integer']
    if case.mag == 'wide':
        assert c['every_slab_wide'], name
        if case.kind in ('f16', 'f16w') and not case.out16:
            assert np.abs(want).max() > 4 * 2048                 # an fp16 accumulator would show
    if case.stats:
        q = 1.0 / 64 if case.mag == 'mid' else float(case.scale)          # small magnitudes are whole numbers
        s = R.block_sums(torch.from_numpy(np.abs(want)), want.shape[0], case.cout).numpy()
        assert s[:, 0].max() / q < 2 ** 24
        if case.stats == 1:
            assert s[:, 1].max() / (q * q) < 2 ** 24
        if case.out16 and case.stats == 2:                       # the rounding is not trivial
            exact = R.evaluate(case._replace(out16=0, stats=0), d)['out'].numpy()
            assert (exact != want).mean() > 0.05
    if case.out16 and case.mag == 'wide':
        exact = R.evaluate(case._replace(out16=0, stats=0), d)['out'].numpy()
        assert (exact != want).mean() > 0.05 and np.isfinite(want).all()


def test_the_layer_every_kernel_runs_is_exact_for_each_of_them():
    cases = R.agree_cases()
    assert {(c.kid, c.wino) for c in cases} == {(0, 0), (128, 0), (1284, 0), (256, 0), (2565, 0), (2565, 1), (2563, 0)}
    wino = [c for c in cases if c.wino][0]
    d = R.make_data(wino, 'A')
    want = R.a_reference(wino, d)[0]
    for c in cases:
        cond = R.conditions(c, d)
        assert cond['units'] < 2 ** 24 and cond['operands_fit'] and cond['every_slab_wide'], (c.name, cond)
        assert np.array_equal(R.evaluate(c, d, torch.float32)['out'].double().numpy(), want)


def test_every_kernel_id_has_a_wide_mantissa_case():
    for kid in R.KERNEL_IDS:
        assert [c for c in CASES if c.kid == kid and 'A' in c.fam and c.mag == 'wide'], kid


# ------------------------------------------------------------------------------------------------------------------------------
# the plain fp32 evaluation is inside the criterion; its mutants are outside

@pytest.mark.parametrize('name,fam,role', [r for r in R.RUNS], ids=lambda v: str(v))
def test_plain_fp32_evaluation_passes_the_criterion(name, fam, role):
    case, d, ref = _run(name, fam, role)
    r = R.evaluate(case, d, torch.float32)
    assert _passes(case, fam, ref, r) == (True, True), name


MUTANTS = [
    # (defect, case, family, which part of the criterion must fail: 0 output, 1 statistics)
    ('slab_f16', 'h1284', 'A', 0),                     # one 32-channel operand slab rounded to fp16, exact-fp32 case
    ('acc_f16', 'f16c', 'A', 0),                       # the accumulator rounded to fp16 once, fp16 case
    ('rtz16', 'f16c_full', 'A', 0),                    # out_f16 rounded toward zero
    ('cbias_neighbour', 'h128_multi_image', 'A', 0),   # per-image bias of the neighbouring image, multi-image tile
    ('cbias_rows', 'h1284_nonsquare', 'A', 0),         # cbias_rows = 1 treated as n
    ('pad_raw', 'h128_full', 'A', 0),                  # zero padding applied to the raw tensor, B != 0
    ('halo_cell', 'h1284', 'A', 0),                    # one out-of-image halo cell non-zero
    ('res_after_scale', 'h256_full', 'A', 0),          # the residual added after out_scale
    ('stats_unrounded', 'f16c_stats16_rounding', 'A', 1),   # statistics of the unrounded values under out_f16
    ('tap_shift', 'h128_b', 'B', 0),                   # one selected tap shifted by one pixel
    ('one_element', 'h1284', 'A', 0),                  # one element off by 1e-5 of the absmax
    ('one_element', 'h128_b', 'B', 0),
]


@pytest.mark.parametrize('mut,name,fam,part', MUTANTS, ids=lambda v: str(v))
def test_mutant_of_the_fp32_evaluation_fails_the_criterion(mut, name, fam, part):
    case, d, ref = _run(name, fam)
    r = R.evaluate(case, d, torch.float32, mut=(mut,))
    ok = _passes(case, fam, ref, r)
    assert not ok[part], (mut, name)
    if mut == 'one_element':          # ... which the comparison this family had until now lets through
        want = ref[0]
        got = r['out'].double().numpy()
        assert np.abs(got - want).max() / np.abs(want).max() < 2e-5


# ------------------------------------------------------------------------------------------------------------------------------
# ds_gemm_nt_batched

def test_gemm_table_covers_what_it_names():
    cs = R.GEMM_CASES
    assert {c.m for c in cs} >= {1, 64, 100, 129} and {c.n for c in cs} >= {1, 64, 100, 129} and {c.k for c in cs} == {32, 96}
    for f in ('rowbias', 'colbias', 'act'):
        assert {getattr(c, f) for c in cs} == {0, 1}
    assert [c for c in cs if c.alpha != 1.0] and [c for c in cs if c.alpha == 1.0] and all(np.log2(c.alpha) % 1 == 0 for c in cs)
    assert [c for c in cs if c.batch > 1 and c.heads > 1]


@pytest.mark.parametrize('case', R.GEMM_CASES, ids=lambda c: c.name)
def test_gemm_data_is_exact_and_the_fp32_evaluation_passes(case):
    d = R.gemm_data(case)
    ref, bound, units = R.gemm_reference(case, d)
    assert units < 2 ** 24
    a, b = torch.from_numpy(d['a']).float(), torch.from_numpy(d['b']).float()
    assert np.array_equal(a.double().numpy(), d['a']) and np.array_equal(b.double().numpy(), d['b'])
    v = torch.einsum('bmhk,bnhk->bhmn', a, b) * case.alpha
    if d['colbias'] is not None:
        v = v + torch.from_numpy(d['colbias']).float()[None, None, None, :]
    if d['rowbias'] is not None:
        v = v + torch.from_numpy(d['rowbias']).float()[None, None, :, None]
    if case.act:
        v = v * torch.sigmoid(v)
    got = v.double().numpy()
    assert (got == ref).all() if bound is None else R.inside(got, ref, bound).all()
