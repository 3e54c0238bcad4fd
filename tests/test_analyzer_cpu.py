"""Trajectory analysis without a GPU: the host paths of diff_sampler_amd/analyzer.py against the direct restatement (_analyzer_ref.py) and
against results recorded from the reference (tests/golden/analyzer_small.npz, tools/gen_analyzer_golden.py), the library surface of the two
new entry points, and the argument rules of the samplers' return_denoised."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _analyzer_ref as R  # noqa: E402
from diff_sampler_amd import analyzer  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'analyzer_small.npz')


def _rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


# ------------------------------------------------------------------------------------------------------------------ projection
@pytest.mark.parametrize('name', sorted(R.PROJECTION_CASES))
def test_projection_cases_meet_their_conditions(name):
    gap, probe = R.conditions(name)
    assert gap >= R.MIN_GAP and probe >= R.MIN_PROBE, (name, gap, probe)


@pytest.mark.parametrize('name', sorted(R.PROJECTION_CASES))
def test_project_trajectories_host_path_equals_the_direct_route(name):
    """Gram form (fp64, eigh of a T x T matrix) against projector + SVD on the D-dimensional points.  Observed: 3e-13 absolute at
    magnitude ~60; the bound is the 1e-9 of the GPU test, whose derivation (gap conditions amplify the Gram's relative perturbation of
    about per 2^-53 by less than 1e3) does not depend on where the Gram matrix was formed."""
    traj, ref = R.projection_case(name)
    got = analyzer.project_trajectories(traj)
    T, B = traj.shape[0], traj.shape[1]
    for k in ('xs', 'ys', 'zs'):
        assert got[k].shape == (T, B) and got[k].dtype == np.float64
        scale = np.abs(ref[k]).max()
        err = np.abs(got[k] - ref[k]).max()
        print(name, k, 'max abs err %.3e at scale %.3e' % (err, scale))
        assert err <= 1e-9 * scale, (name, k, err, scale)
    assert got['singular_values'].shape == (B, min(T, 8))
    assert _rel(got['singular_values'][:, :3], ref['singular_values'][:, :3]) <= 1e-9
    mid = T // 2
    assert (got['xs'][mid] < 0).all() and (got['ys'][mid] > 0).all() and (got['zs'][mid] < 0).all()     # the cell's sign rules
    assert np.abs(got['xs'][-1]).max() == 0 and np.abs(got['ys'][-1]).max() <= 1e-9 * np.abs(ref['ys']).max()      # the end is the origin


def test_trajectory_gram_host_is_the_definition_and_symmetric():
    traj = R.lattice(5, (6, 3, 37))
    g = analyzer.trajectory_gram(torch.from_numpy(traj).reshape(6, 3, 37, 1, 1))
    assert g.dtype == torch.float64 and tuple(g.shape) == (3, 6, 6)
    assert np.array_equal(g.numpy(), R.gram_int(traj).astype(np.float64))
    assert torch.equal(g, g.transpose(1, 2))
    with pytest.raises(ValueError):
        analyzer.trajectory_gram(torch.zeros(1, 2, 5))
    with pytest.raises(ValueError):
        analyzer.trajectory_gram(torch.zeros(4, 5))


def test_two_point_trajectory_projects_onto_the_chord_only():
    traj = R.random_walk(7, (2, 3, 11))
    got = analyzer.project_trajectories(traj)
    chord = (traj[0].to(torch.float64) - traj[1].to(torch.float64)).reshape(3, -1).norm(dim=1).numpy()
    # row T // 2 = 1 is the end point, xs = 0 there: "keep u1 where the probe is < 0" flips, as the reference's rule does
    assert np.allclose(got['xs'][0], chord, rtol=1e-14) and not got['xs'][1].any()
    # nothing is left beside the chord: M = G - g0 g0^T / G00 is zero up to the rounding of one product and one quotient
    for k in ('ys', 'zs'):
        assert np.isfinite(got[k]).all() and np.abs(got[k]).max() <= 1e-6 * chord.max()
    assert np.isfinite(got['singular_values']).all() and got['singular_values'].shape == (3, 2)


def test_drop_outliers_keeps_the_middle_of_the_order():
    B = 10
    ys = np.arange(B, dtype=np.float64)[None, ::-1].repeat(4, 0)          # energy falls with the index
    xs, zs = np.zeros_like(ys), np.zeros_like(ys)
    kx, ky, kz, keep = analyzer.drop_outliers(xs, ys, zs, ratio_to_keep=0.8)
    assert keep.tolist() == [8, 7, 6, 5, 4, 3, 2, 1]                       # ascending energy, one dropped at either end
    assert ky.shape == (4, 8) and np.array_equal(ky, ys[:, keep])


# ------------------------------------------------------------------------------------------------------------------ alignment
def _rot3(a, b, c):
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    return (np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]]) @ np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
            @ np.array([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]]))


@pytest.mark.parametrize('proj_dim', [2, 3])
def test_align_trajectories(proj_dim):
    g = np.random.RandomState(4)
    T = 12
    base = np.cumsum(g.randn(T, 3), axis=0)
    rot = _rot3(0.7, 0.0, 0.0) if proj_dim == 2 else _rot3(0.7, -0.4, 1.1)      # proj_dim 2 rotates (ys, zs) about the xs axis
    other = np.cumsum(g.randn(T, 3), axis=0)
    pts = np.stack([base, base @ rot, other], axis=2)                            # [T, 3, B]: base, its rotated copy, an unrelated one
    out = analyzer.align_trajectories(pts[:, 0], pts[:, 1], pts[:, 2], base_idx=0, proj_dim=proj_dim)
    got = np.stack([out['xs'], out['ys'], out['zs']], axis=1)
    O = out['rotations']
    assert O.shape == (3, proj_dim, proj_dim)
    assert np.abs(O @ O.transpose(0, 2, 1) - np.eye(proj_dim)).max() <= 1e-14                  # orthogonal
    assert np.abs(got[:, :, 0] - base).max() <= 1e-13 * np.abs(base).max()                       # the base maps to itself
    assert np.abs(got[:, :, 1] - base).max() <= 1e-13 * np.abs(base).max()                       # its rotated copy lands on it
    before, after = np.linalg.norm(pts[:, :, 2] - base), np.linalg.norm(got[:, :, 2] - base)
    assert after <= before * (1 + 1e-14)                                                         # and nothing moves away from the base
    if proj_dim == 2:
        assert np.array_equal(got[:, 0], pts[:, 0])                                              # xs is kept
    with pytest.raises(ValueError):
        analyzer.align_trajectories(pts[:, 0], pts[:, 1], pts[:, 2], proj_dim=4)


# ------------------------------------------------------------------------------------------------------------------ golden: recorded from the reference
def test_arc_length_and_cal_curv_tors_match_the_recorded_reference():
    z = np.load(GOLDEN)
    xs, ys, zs = z['curv_xs'], z['curv_ys'], z['curv_zs']
    s = analyzer.arc_length(xs, ys, zs)
    assert s.shape == xs.shape and _rel(s, z['curv_s']) <= 1e-12
    curv, tors = analyzer.cal_curv_tors(xs, ys, zs, z['curv_s'], int(z['curv_window']))
    assert curv.shape == z['curv_curvatures'].shape == xs.shape
    print('curvature %.3e torsion %.3e relative' % (_rel(curv, z['curv_curvatures']), _rel(tors, z['curv_torsions'])))
    assert _rel(curv, z['curv_curvatures']) <= 1e-12 and _rel(tors, z['curv_torsions']) <= 1e-12
    with pytest.raises(ValueError):
        analyzer.cal_curv_tors(xs, ys, zs, s, 10)


def test_trajectory_stats_deviation_matches_the_recorded_reference():
    z = np.load(GOLDEN)
    traj = torch.from_numpy(z['dev_traj'])
    st = analyzer.trajectory_stats(traj)
    dev = st['dev_xt']                                               # [n - 2, B]; the reference returns [B, n - 2]
    assert dev.shape == z['dev_f32'].T.shape and dev.dtype == np.float64
    print('vs fp32 reference %.3e, vs fp64 reference %.3e' % (_rel(dev, z['dev_f32'].T), _rel(dev, z['dev_f64'].T)))
    assert _rel(dev, z['dev_f32'].T) <= 2e-6
    assert _rel(dev, z['dev_f64'].T) <= 1e-12


def test_trajectory_stats_keys_shapes_and_definitions():
    n, B = 6, 4
    xt = R.random_walk(11, (n, B, 2, 3, 3))
    dn = R.random_walk(12, (n - 1, B, 2, 3, 3))
    ep = R.random_walk(13, (n - 1, B, 2, 3, 3), scale=1.0)
    st = analyzer.trajectory_stats(xt, dn, ep)
    assert sorted(st) == sorted(['mag_xt', 'mag_denoised', 'mag_eps', 'dev_xt', 'dev_denoised', 'dist_xt', 'dist_denoised', 'cos_xt'])
    want = dict(mag_xt=n, mag_denoised=n - 1, mag_eps=n - 1, dev_xt=n - 2, dev_denoised=n - 3, dist_xt=n, dist_denoised=n - 1, cos_xt=n - 1)
    for k, rows in want.items():
        assert st[k].shape == (rows, B) and st[k].dtype == np.float64, k
    x64, d64, e64 = (t.to(torch.float64) for t in (xt, dn, ep))
    assert _rel(st['mag_xt'], x64.flatten(2).norm(dim=2).numpy()) <= 1e-14
    assert _rel(st['mag_eps'], e64.flatten(2).norm(dim=2).numpy()) <= 1e-14
    assert _rel(st['dist_denoised'], (d64 - d64[-1:]).flatten(2).norm(dim=2).numpy()) <= 1e-14
    cos = torch.nn.functional.cosine_similarity(e64.flatten(2), (x64[:-1] - x64[-1:]).flatten(2), dim=2).numpy()
    assert np.abs(st['cos_xt'] - cos).max() <= 1e-14
    assert sorted(analyzer.trajectory_stats(xt)) == ['dev_xt', 'dist_xt', 'mag_xt']
    assert _rel(analyzer.trajectory_distance(xt, xt.flip(0)), (x64 - x64.flip(0)).flatten(2).norm(dim=2).numpy()) <= 1e-14
    with pytest.raises(ValueError):
        analyzer.trajectory_stats(xt, None, ep[:-1])                  # eps has one row per step
    with pytest.raises(ValueError):
        analyzer.trajectory_distance(xt, xt[:-1])


# ------------------------------------------------------------------------------------------------------------------ library surface
@pytest.fixture(scope='module')
def lib():
    from diff_sampler_amd import build, _metrics_lib
    build.build_metrics_lib(verbose=False)
    return _metrics_lib.load()


def test_abi_rows_and_version(lib):
    from diff_sampler_amd import _metrics_lib as M
    assert lib.dsm_version() == M.DSM_VERSION == 2
    rows = M._SIGNATURES
    assert rows['dsm_traj_gram'] == (C.c_int, [M.vp, C.c_int, C.c_int, C.c_longlong, C.c_int, C.c_int, M.vp, M.vp, C.c_longlong, M.vp])
    assert rows['dsm_traj_gram_workspace_bytes'] == (C.c_longlong, [C.c_int, C.c_longlong, C.c_int])
    assert rows['dsm_row_sqdist'] == (C.c_int, [M.vp, M.vp, C.c_longlong, C.c_longlong, M.vp, M.vp])
    header = open(os.path.join(ROOT, 'diff_sampler_amd', 'csrc', 'metrics', 'ds_metrics.h')).read()
    for name in ('dsm_traj_gram', 'dsm_traj_gram_workspace_bytes', 'dsm_traj_gram_splits', 'dsm_row_sqdist'):
        assert name in M.EXPORTS and hasattr(lib, name) and ('DSM_API int %s(' % name in header or 'DSM_API long long %s(' % name in header)


def test_argument_errors_are_answered_on_the_host(lib):
    """Every rejection comes back before any launch: no GPU is needed (or touched) for them."""
    from diff_sampler_amd._metrics_lib import DS_E_ARG, DS_E_SHAPE, DS_E_ALIGN
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 4)
    big = 1 << 40

    def gram(traj=p, n_pts=21, batch=3, per=3072, b0=0, nb=3, out=p, ws=p, nbytes=big):
        return lib.dsm_traj_gram(traj, n_pts, batch, per, b0, nb, out, ws, nbytes, None)

    assert gram(traj=None) == gram(out=None) == gram(ws=None) == DS_E_ARG
    assert gram(n_pts=1) == gram(batch=0) == gram(per=0) == gram(nb=0) == gram(b0=-1) == DS_E_ARG
    assert gram(b0=1, nb=3) == gram(b0=3, nb=1) == DS_E_ARG                       # the window leaves the batch
    need = lib.dsm_traj_gram_workspace_bytes(21, 3072, 3)
    assert need == 3 * lib.dsm_traj_gram_splits(21, 3072) * 21 * 21 * 8 and gram(nbytes=need - 1) == DS_E_ARG
    assert gram(ws=odd) == DS_E_ALIGN
    assert gram(n_pts=32769) == DS_E_SHAPE and gram(batch=70000, nb=65536) == DS_E_SHAPE
    assert lib.dsm_traj_gram_workspace_bytes(1, 8, 1) == DS_E_ARG and lib.dsm_traj_gram_workspace_bytes(5, 0, 1) == DS_E_ARG
    assert lib.dsm_traj_gram_workspace_bytes(5, 8, 0) == DS_E_ARG and lib.dsm_traj_gram_workspace_bytes(40000, 8, 1) == DS_E_SHAPE
    # the split is a function of (n_pts, per) alone: one tile of a long contraction is split, a short one or many tiles are not
    assert lib.dsm_traj_gram_splits(21, 3072) > 1 and lib.dsm_traj_gram_splits(21, 48) == 1 and lib.dsm_traj_gram_splits(1001, 3072) == 1
    assert lib.dsm_traj_gram_splits(130, 4099) > 1 and lib.dsm_traj_gram_splits(1, 8) == DS_E_ARG
    assert lib.dsm_traj_gram_workspace_bytes(1001, 3072, 100) == 0                 # no split, no workspace

    def rows(a=p, b=None, n=5, per=7, out=p):
        return lib.dsm_row_sqdist(a, b, n, per, out, None)

    assert rows(a=None) == rows(out=None) == rows(n=0) == rows(per=0) == DS_E_ARG
    assert rows(n=1 << 31) == DS_E_SHAPE


def test_cuda_path_has_no_fallback(monkeypatch, tmp_path):
    """A device tensor never takes the host route: without the library the device route raises before any work."""
    from diff_sampler_amd import _metrics_lib
    monkeypatch.setattr(_metrics_lib, '_lib', None)
    monkeypatch.setattr(_metrics_lib, 'LIB_PATH', str(tmp_path / 'nope.so'))

    class FakeCuda:                                   # _gram_device loads the library before it looks at the tensor
        is_cuda, shape = True, (4, 2, 8)

    with pytest.raises(_metrics_lib.DsMetricsError, match='no CPU fallback'):
        analyzer._gram_device(FakeCuda())


# ------------------------------------------------------------------------------------------------------------------ return_denoised: the rules
SAMPLERS = ['euler_sampler', 'heun_sampler', 'dpm_2_sampler', 'ipndm_sampler', 'ipndm_v_sampler', 'deis_sampler', 'dpm_pp_sampler']


@pytest.mark.parametrize('fn', SAMPLERS)
def test_return_denoised_rules_need_no_device(fn):
    import inspect
    from diff_sampler_amd import solvers
    f = getattr(solvers, fn)
    assert inspect.signature(f).parameters['return_denoised'].default is False
    lat = torch.zeros(2, 3, 8, 8)
    kw = dict(num_steps=4, coeff_list=[[]] * 4)
    with pytest.raises(ValueError, match='return_inters'):
        f(None, lat, return_denoised=True, **kw)
    # afs: the reference's dpm_pp records x - t d, heun / dpm_2 record their second evaluation; the single-evaluation solvers read an unbound name
    if fn in ('heun_sampler', 'dpm_2_sampler', 'dpm_pp_sampler'):
        with pytest.raises(RuntimeError, match='no CPU fallback'):          # the rules pass; CPU latents are refused as always
            f(None, lat, return_inters=True, return_denoised=True, afs=True, t_steps=torch.linspace(80, 0.002, 4), **kw)
    else:
        with pytest.raises(ValueError, match='afs'):
            f(None, lat, return_inters=True, return_denoised=True, afs=True, **kw)
    with pytest.raises(RuntimeError, match='no CPU fallback'):              # default: nothing new in the way
        f(None, lat, t_steps=torch.linspace(80, 0.002, 4), **kw)
