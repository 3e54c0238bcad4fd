"""CPU: the fp64 references and error bounds of tests/_kernel_refs.py, checked without a GPU -- an fp32 evaluation of the solver update
stays inside the per-element bounds on the very inputs the GPU test uses, the case table reaches every update kernel in every mode, the
'dev' closed form agrees with the cost's definition, and the special inputs of the quantile and quantisation tests are what they claim."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, ROOT)

import _kernel_refs as R  # noqa: E402

ALL_UPDATE = R.UPDATE_CASES + [R.MISALIGN_BASE._replace(misalign=op) for op in R.MISALIGNED_OPERANDS] + [R.MISALIGN_AFS._replace(misalign='xe')]
SMALL_UPDATE = [c for c in ALL_UPDATE if not c.name.startswith('trip2')]


def test_update_case_table_reaches_every_kernel_in_every_mode():
    seen = {(R.expected_update_kernel(c), c.mode) for c in ALL_UPDATE}
    for kernel in ('fast', 'generic', 'scalar'):
        for mode in ('raw4', 'raw8', 'planar', 'nonraw', 'afs'):
            if (kernel, mode) == ('fast', 'raw8'):
                assert (kernel, mode) not in seen               # rows of 8 floats never take the streaming kernel
                continue
            assert (kernel, mode) in seen, (kernel, mode)
        mine = [c for c in ALL_UPDATE if R.expected_update_kernel(c) == kernel]
        assert {c.nhist for c in mine} == {0, 1, 2, 3}, kernel
        assert {c.xb_distinct for c in mine} == {False, True}, kernel
        assert {c.outs for c in mine} == {'x', 'm', 'both'}, kernel
        assert {c.store_d for c in mine} == {0, 1}, kernel
        assert {c.coef for c in mine} == {'host', 'dev1', 'devn'}, kernel
    # the shapes the kernels are selected by
    by = lambda k: {(c.c, c.h, c.w) for c in ALL_UPDATE if R.expected_update_kernel(c) == k and c.misalign is None and not c.name.startswith('trip2')}
    assert by('fast') == {(3, 2, 2), (4, 2, 2), (3, 4, 6)}
    assert {c for c, _, _ in by('generic')} == {1, 2, 4, 5, 8} and {h * w for _, h, w in by('generic')} == {4, 24}
    assert by('scalar') == {(3, 5, 5), (4, 3, 3), (5, 1, 1)}
    assert all(R.expected_update_kernel(R.MISALIGN_BASE._replace(misalign=op)) == 'scalar' for op in R.MISALIGNED_OPERANDS)
    assert R.expected_update_kernel(R.MISALIGN_BASE) == 'fast'
    # the second trip: more work items than 4096 blocks x 256 threads, one case per kernel
    trips = {R.expected_update_kernel(c): c for c in ALL_UPDATE if c.name.startswith('trip2')}
    assert set(trips) == {'fast', 'generic', 'scalar'}
    for k, c in trips.items():
        work = c.n * c.h * c.w // (1 if k == 'scalar' else 4)
        assert 4096 * 256 < work < 4096 * 256 + 64, (k, work)
    assert (trips['scalar'].n, trips['scalar'].c, trips['scalar'].h * trips['scalar'].w) == (3, 1, 349527)
    assert (trips['generic'].n, trips['generic'].c, trips['generic'].h * trips['generic'].w) == (2, 1, 2097156)
    assert (trips['fast'].n, trips['fast'].c, trips['fast'].h * trips['fast'].w) == (2, 3, 2097156)
    # 'devn' really gives every sample its own t, sigma and coefficients
    k = R.update_inputs(R.MISALIGN_BASE)['coefs']
    assert all(len(set(k[:, j].tolist())) == k.shape[0] for j in range(7))
    assert float(k[:, 5:7].min()) >= 0.002 and float(k[:, 5:7].max()) <= 80.0


@pytest.mark.parametrize('case', SMALL_UPDATE, ids=[c.name + ('' if c.misalign is None else '_' + c.misalign) for c in SMALL_UPDATE])
def test_fp32_update_stays_inside_the_bounds_on_the_gpu_tests_inputs(case):
    d = R.update_inputs(case)
    args = (d['xe'], d['xb'], d['f'], d['hist'], d['coefs'], d['sigma_data'], case.mode, case.store_d)
    m_ref, x_ref, m_bnd, x_bnd = R.solver_update_ref(*args)
    m32, x32 = R.solver_update_fp32(*args)
    assert bool(((m32.double() - m_ref).abs() <= m_bnd).all()), float(((m32.double() - m_ref).abs() / m_bnd.clamp_min(1e-300)).max())
    assert bool(((x32.double() - x_ref).abs() <= x_bnd).all()), float(((x32.double() - x_ref).abs() / x_bnd.clamp_min(1e-300)).max())
    # the bounds are tight enough to notice a wrong operand: shifting F (or x under AFS) by one element breaks them
    wrong = list(args)
    wrong[0 if case.mode == 'afs' else 2] = torch.roll(args[0 if case.mode == 'afs' else 2], 1, dims=-1 if case.w > 1 else 1)
    mw, _ = R.solver_update_fp32(*wrong)
    assert not bool(((mw.double() - m_ref).abs() <= m_bnd).all())


def test_fp32_update_error_in_units_of_the_bound_over_random_draws():
    """400 random draws (t, sigma in [0.002, 80], per-sample coefficients, both values of raw and store_d): the fp32 evaluation stays
    well inside 8 units for m and 16 units for x'."""
    worst_m = worst_x = 0.0
    for s in range(400):
        case = R._u('draw', (3, 2, 2), ('planar', 'nonraw', 'afs', 'raw4')[s % 4], s % 3 + 1, s % 2, 'both', (s // 4) % 2, 'devn')
        d = R.update_inputs(case, seed=7000 + s)
        args = (d['xe'], d['xb'], d['f'], d['hist'], d['coefs'], d['sigma_data'], case.mode, case.store_d)
        m_ref, x_ref, m_bnd, x_bnd = R.solver_update_ref(*args)
        m32, x32 = R.solver_update_fp32(*args)
        worst_m = max(worst_m, float(((m32.double() - m_ref).abs() / (m_bnd / 8)).max()))
        worst_x = max(worst_x, float(((x32.double() - x_ref).abs() / (x_bnd / 16)).max()))
    assert worst_m < 8 and worst_x < 16, (worst_m, worst_x)


def test_nhwc_rows_layout():
    f = torch.arange(2 * 3 * 2 * 2, dtype=torch.float32).reshape(2, 3, 2, 2)
    rows = R.nhwc_rows(f, 4)
    assert rows.shape == (8, 4) and bool(torch.isnan(rows[:, 3]).all())
    assert rows[5, 1] == f[1, 1, 0, 1]


# ---------------------------------------------------------------------------------------------------------------- quantile inputs

def test_quantile_rank_of_201_values_is_an_integer_in_fp32():
    rank, lo, hi = R.fp32_rank(201)
    assert rank == 199.0 and lo == hi == 199
    assert R.fp32_rank(1001)[1:] == (995, 995)                  # 0.995f * 1000 rounds to 995 as well
    for per in R.QUANTILE_PERS:
        if per not in (201, 1001):
            rank, lo, hi = R.fp32_rank(per)
            assert hi == lo + 1 and hi <= per - 1, per
    assert (R.QUANTILE_LDS_CAP + 256) * 4 <= 150 * 1024 < (R.QUANTILE_LDS_CAP + 1 + 256) * 4


@pytest.mark.parametrize('per', R.QUANTILE_PERS)
def test_quantile_inputs_are_what_they_claim(per):
    for kind in R.QUANTILE_KINDS:
        x = R.quantile_inputs(kind, per)
        assert x.shape == (4, per) and x.dtype == torch.float32 and bool(torch.isfinite(x).all()), kind
    assert float(R.quantile_inputs('below1', per).abs().max()) < 1
    assert float(R.quantile_inputs('huge', per).abs().max()) == float(np.float32(1e30))
    x = R.quantile_inputs('ties', per)
    _, lo, hi = R.fp32_rank(per)
    for b in range(4):
        mag, order = x[b].abs().sort()
        assert mag[lo] == mag[hi], b                                       # the tie straddles both order statistics
        tied = x[b][x[b].abs() == mag[lo]]
        assert per < 4 or (bool((torch.signbit(tied)).any()) and bool((~torch.signbit(tied)).any())), b
    assert bool(torch.signbit(x[0]).any()) and bool((~torch.signbit(x[0])).any()) and float(x[0].abs().max()) == 0.0       # signed zeros
    tiny = float(torch.finfo(torch.float32).tiny)
    assert 0.0 < float(x[1].abs().max()) < tiny                            # fp32 denormals
    if per >= 200:
        assert bool(((x[2].abs() > 0) & (x[2].abs() < tiny)).any()) and bool((x[2] == 0).any())


# ---------------------------------------------------------------------------------------------------------------- GITS costs

@pytest.mark.parametrize('shape', R.TRAJ_SHAPES)
def test_dev_closed_form_from_numpy_moments_matches_the_definition(shape):
    traj, eps, t = R.synthetic_trajectory(*shape)
    m, _ = R.traj_moments_ref(traj, eps)
    direct, tol = R.pair_costs_ref(traj, eps, t, 'dev')
    closed = R.dev_closed_form(m, t)
    iu = np.triu_indices(shape[0], 1)
    if shape[2] == 1:
        tol = tol * 1e5         # one value per sample: every point lies on the chord, the degenerate bound 1e-7 * s applies
    assert np.all(np.abs(closed - direct)[iu] <= tol[iu]), float((np.abs(closed - direct)[iu] / tol[iu]).max())
    assert np.all(closed[np.tril_indices(shape[0])] == 0)


def test_dev_closed_form_on_the_degenerate_trajectory():
    traj, eps, t = R.degenerate_trajectory()
    m, _ = R.traj_moments_ref(traj, eps)
    direct, tol = R.pair_costs_ref(traj, eps, t, 'dev')
    iu = np.triu_indices(len(t), 1)
    assert np.all(np.abs(direct[iu]) <= tol[iu] * 1e3)            # on the chord: 0 up to fp64 rounding of the projection
    closed = R.dev_closed_form(m, t)
    assert np.all(np.abs(closed - direct)[iu] <= 1e5 * tol[iu]), float((np.abs(closed - direct)[iu] / tol[iu]).max())


@pytest.mark.parametrize('shape', R.TRAJ_SHAPES[1:])
def test_library_cost_matrix_on_numpy_moments_matches_the_definition(shape, monkeypatch):
    """gits_utils._cost_matrix_round('dev') itself, fed the numpy moments instead of the kernel's: its closed form against the definition
    (the pair costs are means over the batch)."""
    from diff_sampler_amd import gits_utils
    traj, eps, t = R.synthetic_trajectory(*shape)
    monkeypatch.setattr(gits_utils, 'trajectory_moments', lambda tr, e=None: R.traj_moments_ref(tr, e)[0])
    cost = gits_utils._cost_matrix_round(traj, eps, t, 'dev')
    direct, tol = R.pair_costs_ref(traj, eps, t, 'dev')
    assert np.all(np.abs(cost - direct) <= tol), float((np.abs(cost - direct)[tol > 0] / tol[tol > 0]).max())
    dev = gits_utils.cal_deviation(traj)
    dref, Rj = R.deviation_ref(traj)
    assert dev.shape == dref.shape and np.all(np.abs(dev.double().numpy() - dref) <= 2 * R.U * dref + 1e-12 * np.sqrt(Rj))


def test_l1_l2_reference_against_a_plain_loop():
    traj, eps, t = R.synthetic_trajectory(4, 2, 5)
    x, d = traj.double().numpy(), eps.double().numpy()
    for metric, p in (('l1', 1), ('l2', 2)):
        cost, tol = R.pair_costs_ref(traj, eps, t, metric)
        for i in range(4):
            for j in range(4):
                want = 0.0
                if i < j:
                    want = np.mean([np.linalg.norm(x[i, b] + (t[j] - t[i]) * d[i, b] - x[j, b], p) for b in range(2)])
                assert abs(cost[i, j] - want) <= 1e-13 * max(want, 1.0) and (tol[i, j] > 0) == (i < j)


def test_moment_reference_against_einsum():
    traj, eps, _ = R.synthetic_trajectory(7, 3, 75)
    m, mabs = R.traj_moments_ref(traj, eps)
    x, d = traj.double().numpy(), np.concatenate([eps.double().numpy(), np.zeros((1, 3, 75))])
    cx, bc = x[-1] - x, np.broadcast_to(x[-1] - x[0], x.shape)
    for k, (a, b) in enumerate([(cx, bc), (d, bc), (cx, cx), (cx, d), (d, d), (bc, bc)]):
        assert np.allclose(m[:, :, k], np.einsum('ibe,ibe->ib', a, b), rtol=1e-13, atol=0)
    assert np.all(mabs >= np.abs(m)) and np.all(R.traj_moments_ref(traj)[0][:, :, [1, 3, 4]] == 0)


# ---------------------------------------------------------------------------------------------------------------- glue references

def test_quantize_edge_values_separate_a_fused_multiply_add_from_two_roundings():
    e = R.quantize_edge_values().reshape(1, 1, 1, -1)
    two, one = R.quantize_ref(e), R.quantize_fma_ref(e)
    assert int((two != one).sum()) > 0                          # some inputs land exactly on an integer only with both roundings
    v = (e * 127.5 + 128).flatten()
    on_int = (v == v.round()) & (v > 0) & (v < 255)
    assert int(on_int.sum()) >= 256
    assert float(e.min()) < -1 and float(e.max()) > 1
    assert set(two.flatten().tolist()) == set(range(256))
    x = R.quantize_inputs(2, 3, 5, 7)
    assert x.shape == (2, 3, 5, 7)


def test_stem_im2col_reference_layout():
    g = torch.Generator().manual_seed(0)
    n, c, h, w, kpad = 2, 3, 4, 5, 32
    x = torch.randn(n, c, h, w, generator=g)
    sigma = torch.tensor([0.7, 3.0])
    ref = R.stem_im2col_ref(x, sigma, 0.5, kpad)
    cin = R.c_in64(sigma, 0.5)
    for (img, oh, ow, tap, ch) in [(0, 0, 0, 0, 1), (1, 3, 4, 8, 2), (1, 2, 2, 4, 0), (0, 1, 0, 3, 2), (1, 0, 4, 2, 1)]:
        ih, iw = oh + tap // 3 - 1, ow + tap % 3 - 1
        want = float(cin[img]) * float(x[img, ch, ih, iw]) if 0 <= ih < h and 0 <= iw < w else 0.0
        assert float(ref[(img * h + oh) * w + ow, tap * c + ch]) == want
    assert bool((ref[:, 9 * c:] == 0).all())


def test_softmax_inputs_carry_the_special_rows():
    x = R.softmax_inputs(7, 130)
    assert float(x[1].max()) == float(x[1].min()) and float(x[2].min()) > 9900 and int(x[3].argmax()) == 129
    assert R.softmax_inputs(1, 1).shape == (1, 1)
