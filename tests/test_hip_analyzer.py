"""Trajectory analysis on the GPU: dsm_traj_gram and dsm_row_sqdist (csrc/metrics/traj.hip) through the C ABI, the device paths of
diff_sampler_amd/analyzer.py, and the samplers' return_denoised.

Bounds:
  * an integer lattice (values in [-512, 512]: differences to 1024, products to 2^20, sums of 4099 of them below 2^33) is EXACT: the
    Gram matrix must equal the int64 one bit for bit, in any summation order;
  * random data against numpy fp64, element by element:  2 per 2^-53 sum_e |y_te y_se|  -- the bound of a sum of `per` products in any
    order, doubled for the reference's own rounding (dsm_row_sqdist: the same with sum_e d_e^2);
  * symmetry, batch invariance (sample 1 of a batch of 3 against the b0 = 1, nb = 1 window and against a batch of 1) and run-to-run: bits;
  * project_trajectories on the device against the host finalisation of the numpy fp64 Gram: 1e-9 max|coordinate| -- under the gap
    conditions of _analyzer_ref.conditions the Gram's relative perturbation of about per 2^-53 is amplified by less than 1e3;
  * trajectory_stats on the device against the host path: 1e-12 relative."""
import ctypes as C
import functools
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

pytestmark = pytest.mark.gpu

GUARD = 777.0
U = 2.0 ** -53


def _lib():
    from diff_sampler_amd import _metrics_lib
    return _metrics_lib.load()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    from diff_sampler_amd import _lib as engine_lib
    return engine_lib.stream_ptr()


def _gram(x, b0=0, nb=None):
    """dsm_traj_gram through the C ABI on a host array [n_pts][batch][per]; one guard element behind the output."""
    lib = _lib()
    n, B, per = x.shape
    nb = B - b0 if nb is None else nb
    xd = torch.from_numpy(np.array(x)).cuda()                      # (a writable copy: the cached cases are read-only)
    out = torch.full((nb * n * n + 1,), GUARD, dtype=torch.float64, device='cuda')
    need = lib.dsm_traj_gram_workspace_bytes(n, per, nb)
    assert need >= 0
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device='cuda')
    rc = lib.dsm_traj_gram(_ptr(xd), n, B, per, b0, nb, _ptr(out), _ptr(ws), need, _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.dsm_error_string(rc)
    got = out.cpu().numpy()
    assert got[-1] == GUARD, 'the guard element was overwritten'
    return got[:-1].reshape(nb, n, n)


@functools.lru_cache(maxsize=None)
def _random_case(n_pts, per, batch):
    x = np.random.RandomState(1000 * n_pts + 10 * per + batch).randn(n_pts, batch, per).astype(np.float32)
    x += np.float32(0.5) * x[:1]                                   # a common component: the chord dominates, as on real trajectories
    ref, scale = R.gram_f64(x)
    for a in (x, ref, scale):
        a.setflags(write=False)
    return x, ref, scale


@pytest.mark.parametrize('batch', [1, 3])
@pytest.mark.parametrize('per', [1, 7, 48, 4099])
@pytest.mark.parametrize('n_pts', [2, 5, 17, 130])
def test_traj_gram_lattice_exact_and_random_within_the_summation_bound(n_pts, per, batch):
    """n_pts 130 crosses a 128-row tile (three lower tiles), per 4099 forces the split with a ragged last chunk, per 1 and 7 are less
    than one chunk."""
    lat = R.lattice(7 * n_pts + per + batch, (n_pts, batch, per))
    got = _gram(lat)
    want = R.gram_int(lat)
    assert np.array_equal(got, want.astype(np.float64)), float(np.abs(got - want).max())
    assert np.array_equal(got, got.transpose(0, 2, 1))
    x, ref, scale = _random_case(n_pts, per, batch)
    got = _gram(x)
    bound = 2.0 * per * U * scale
    worst = float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max())
    print('n_pts %d per %d batch %d: worst error / bound %.3f' % (n_pts, per, batch, worst))
    assert (np.abs(got - ref) <= bound).all(), worst
    assert np.array_equal(got, got.transpose(0, 2, 1)), 'gram[t][s] and gram[s][t] differ in bits'


@pytest.mark.parametrize('n_pts,per', [(17, 4099), (130, 4099), (130, 48), (5, 7)])
def test_traj_gram_batch_invariant_and_reproducible(n_pts, per):
    """Split and unsplit, one tile and three: a sample's matrix is the same bits in the whole batch, in a b0 = 1, nb = 1 window, as a
    batch of 1, and in a second run."""
    x, _, _ = _random_case(n_pts, per, 3)
    whole = _gram(x)
    again = _gram(x)
    window = _gram(x, b0=1, nb=1)
    alone = _gram(np.ascontiguousarray(x[:, 1:2]))
    assert np.array_equal(whole, again)
    assert np.array_equal(whole[1:2], window) and np.array_equal(whole[1:2], alone)
    split = _lib().dsm_traj_gram_splits(n_pts, per)
    assert (split > 1) == (per == 4099), split


def test_traj_gram_error_codes_on_device_pointers():
    from diff_sampler_amd._metrics_lib import DS_E_ARG, DS_E_SHAPE
    lib = _lib()
    x = torch.zeros(5, 3, 4099, device='cuda')
    out = torch.full((3 * 25 + 1,), GUARD, dtype=torch.float64, device='cuda')
    need = lib.dsm_traj_gram_workspace_bytes(5, 4099, 3)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    assert need > 0

    def call(traj=x, n_pts=5, batch=3, per=4099, b0=0, nb=3, gram=out, w=ws, nbytes=need):
        return lib.dsm_traj_gram(_ptr(traj), n_pts, batch, per, b0, nb, _ptr(gram), _ptr(w), nbytes, _stream())

    assert call(traj=None) == call(gram=None) == call(w=None) == DS_E_ARG
    assert call(n_pts=1) == call(per=0) == call(batch=0) == call(nb=0) == DS_E_ARG
    assert call(b0=2, nb=2) == call(b0=-1) == DS_E_ARG and call(nbytes=need - 1) == DS_E_ARG
    assert call(n_pts=40000) == DS_E_SHAPE
    torch.cuda.synchronize()
    assert float(out[-1]) == GUARD and float(out[0]) == GUARD          # a rejected call wrote nothing
    assert call() == 0
    torch.cuda.synchronize()
    assert float(out[0]) == 0.0 and float(out[-1]) == GUARD


@pytest.mark.parametrize('with_b', [False, True])
@pytest.mark.parametrize('per', [1, 4099])
@pytest.mark.parametrize('rows', [1, 5])
def test_row_sqdist(rows, per, with_b):
    lib = _lib()

    def run(a, b):
        ad, bd = torch.from_numpy(a).cuda(), (torch.from_numpy(b).cuda() if b is not None else None)
        out = torch.full((rows + 1,), GUARD, dtype=torch.float64, device='cuda')
        rc = lib.dsm_row_sqdist(_ptr(ad), _ptr(bd), rows, per, _ptr(out), _stream())
        torch.cuda.synchronize()
        assert rc == 0, lib.dsm_error_string(rc)
        got = out.cpu().numpy()
        assert got[-1] == GUARD
        return got[:-1]

    a = R.lattice(rows + per, (rows, per))
    b = R.lattice(rows + per + 1, (rows, per)) if with_b else None
    d = a.astype(np.int64) - (b.astype(np.int64) if with_b else 0)
    assert np.array_equal(run(a, b), (d * d).sum(1).astype(np.float64))
    g = np.random.RandomState(rows * 10 + per)
    a = g.randn(rows, per).astype(np.float32)
    b = g.randn(rows, per).astype(np.float32) if with_b else None
    d = a.astype(np.float64) - (b.astype(np.float64) if with_b else 0.0)
    ref = (d * d).sum(1)
    got = run(a, b)
    assert (np.abs(got - ref) <= 2.0 * per * U * ref).all(), (got, ref)
    assert np.array_equal(got, run(a, b))


# ------------------------------------------------------------------------------------------------------------------ analyzer.py on the device
@pytest.mark.parametrize('name', sorted(R.PROJECTION_CASES))
def test_project_trajectories_on_the_device(name):
    traj, direct = R.projection_case(name)
    T, B = traj.shape[0], traj.shape[1]
    ref_gram, _ = R.gram_f64(traj.reshape(T, B, -1).numpy())
    want = analyzer.project_from_gram(ref_gram)
    got = analyzer.project_trajectories(traj.cuda())
    for k in ('xs', 'ys', 'zs'):
        scale = np.abs(want[k]).max()
        err = np.abs(got[k] - want[k]).max()
        print(name, k, 'max abs err %.3e at scale %.3e' % (err, scale))
        assert got[k].shape == (T, B) and err <= 1e-9 * scale, (name, k, err, scale)
        assert np.abs(got[k] - direct[k]).max() <= 1e-9 * scale          # and with it the direct route's
    assert np.abs(got['singular_values'] - want['singular_values']).max() <= 1e-9 * want['singular_values'].max()


def test_trajectory_gram_on_the_device_chunks_the_batch(monkeypatch):
    """trajectory_gram splits the samples over several calls so that one call's output stays below its byte limit: same bits."""
    x, ref, scale = _random_case(17, 4099, 3)
    t = torch.from_numpy(np.array(x)).cuda()
    whole = analyzer.trajectory_gram(t)
    assert whole.is_cuda and whole.dtype == torch.float64 and tuple(whole.shape) == (3, 17, 17)
    monkeypatch.setattr(analyzer, '_GRAM_BYTES', 17 * 17 * 8)            # one sample per call even without the workspace
    assert torch.equal(analyzer.trajectory_gram(t), whole)
    assert (np.abs(whole.cpu().numpy() - ref) <= 2.0 * 4099 * U * scale).all()


def test_trajectory_stats_on_the_device_equal_the_host_path():
    n, B = 7, 3
    xt = R.random_walk(21, (n, B, 3, 8, 8))
    dn = R.random_walk(22, (n - 1, B, 3, 8, 8))
    ep = R.random_walk(23, (n - 1, B, 3, 8, 8), scale=1.0)
    host = analyzer.trajectory_stats(xt, dn, ep)
    dev = analyzer.trajectory_stats(xt.cuda(), dn.cuda(), ep.cuda())
    assert sorted(dev) == sorted(host) and len(dev) == 8
    for k in host:
        rel = float(np.abs(dev[k] - host[k]).max() / np.abs(host[k]).max())
        print(k, 'device vs host %.3e' % rel)
        assert dev[k].shape == host[k].shape and rel <= 1e-12, (k, rel)
    d = analyzer.trajectory_distance(xt.cuda(), xt.flip(0).cuda())
    h = analyzer.trajectory_distance(xt, xt.flip(0))
    assert np.abs(d - h).max() <= 1e-12 * np.abs(h).max()


# ------------------------------------------------------------------------------------------------------------------ return_denoised
SOLVERS = [('euler_sampler', {}), ('heun_sampler', {}), ('dpm_2_sampler', {}), ('ipndm_sampler', dict(max_order=3)),
           ('ipndm_v_sampler', dict(max_order=3)), ('deis_sampler', dict(max_order=3)), ('dpm_pp_sampler', dict(max_order=2))]
NUM_POINTS = 5           # 4 steps


@pytest.fixture(scope='module')
def tiny():
    from diff_sampler_amd import solver_utils
    from diff_sampler_amd.engine import EDMDenoiser
    net = EDMDenoiser.from_config('tiny_song', seed=3)
    lat = torch.randn(3, net.img_channels, net.img_resolution, net.img_resolution, generator=torch.Generator().manual_seed(5)).cuda()
    ts = solver_utils.get_schedule(NUM_POINTS, 0.002, 80, device=lat.device, schedule_type='polynomial', schedule_rho=7, net=net)
    return net, lat, ts


def _direct_denoised(net, lat, ts, points):
    """D(x; sigma) for a list of (x, sigma): the evaluation a sampler's own `run.denoised` makes."""
    from diff_sampler_amd import solvers
    run = solvers._Run(net, lat, None, None, None, ts, False, False)
    return [run.denoised(x.contiguous(), s).clone() for x, s in points]


def _axpy(net, lat, ts, x, c, d):
    """x + c d with the update kernel's arithmetic (the predictor of heun / dpm_2)."""
    from diff_sampler_amd import solvers
    run = solvers._Run(net, lat, None, None, None, ts, False, False)
    out = run.new()
    run.update(xe=x.contiguous(), xb=x.contiguous(), t=1.0, sigma=1.0, cx=1.0, cm=c, x_out=out, f=d.contiguous(), raw=False, store_d=False)
    return out


@pytest.mark.parametrize('fn,extra', SOLVERS, ids=[s[0] for s in SOLVERS])
def test_return_denoised_records_the_reference_s_evaluation(fn, extra, tiny):
    from diff_sampler_amd import solvers, solver_utils
    net, lat, ts = tiny
    kw = dict(num_steps=NUM_POINTS, t_steps=ts, return_inters=True, return_eps=True, **extra)
    if fn == 'deis_sampler':
        kw['coeff_list'] = solver_utils.get_deis_coeff_list(ts, extra['max_order'], deis_mode='tab')
    f = getattr(solvers, fn)
    xt0, eps0 = f(net, lat, **kw)
    xt, den, eps = f(net, lat, return_denoised=True, **kw)
    torch.cuda.synchronize()
    assert torch.equal(xt, xt0) and torch.equal(eps, eps0), fn                   # capturing changes no bit of the trajectory
    assert tuple(den.shape) == (NUM_POINTS - 1,) + tuple(lat.shape) and den.dtype == torch.float32
    t = solver_utils.host_times(ts)
    points = []
    for i in range(NUM_POINTS - 1):
        if fn == 'heun_sampler':                                                   # the corrector's evaluation: Euler predictor at t_{i+1}
            points.append((_axpy(net, lat, ts, xt[i], t[i + 1] - t[i], eps[i]), t[i + 1]))
        elif fn == 'dpm_2_sampler':                                                # the midpoint evaluation (r = 0.5)
            tm = (t[i + 1] ** 0.5) * (t[i] ** 0.5)
            points.append((_axpy(net, lat, ts, xt[i], tm - t[i], eps[i]), tm))
        else:
            points.append((xt[i], t[i]))
    if fn in ('heun_sampler', 'dpm_2_sampler'):                                    # the kernel's predictor is the plain fp32 x + c d
        c = torch.tensor(points[0][1] - t[0], dtype=torch.float32, device=lat.device)
        assert torch.allclose(points[0][0], xt[0] + c * eps[0], rtol=1e-6, atol=1e-6 * float(xt[0].abs().max()))
    want = _direct_denoised(net, lat, ts, points)
    for i, w in enumerate(want):
        assert torch.equal(den[i], w), (fn, i, float((den[i] - w).abs().max()))
    assert float(den.abs().max()) > 0 and not torch.equal(den[0], den[1])


def test_return_denoised_with_denoise_to_zero_and_dpm_pp_afs(tiny):
    from diff_sampler_amd import solvers, solver_utils
    net, lat, ts = tiny
    t = solver_utils.host_times(ts)
    kw = dict(num_steps=NUM_POINTS, t_steps=ts, return_inters=True, return_eps=True)
    xt0, eps0 = solvers.euler_sampler(net, lat, denoise_to_zero=True, **kw)
    xt, den, eps = solvers.euler_sampler(net, lat, denoise_to_zero=True, return_denoised=True, **kw)
    assert torch.equal(xt, xt0) and torch.equal(eps, eps0)
    assert xt.shape[0] == NUM_POINTS + 1 and den.shape[0] == NUM_POINTS            # one more of each
    assert torch.equal(den[-1], xt[-1])                                            # the final denoised output is the last point
    assert torch.equal(den[-1], _direct_denoised(net, lat, ts, [(xt[-2], t[-1])])[0])
    xt, den, eps = solvers.dpm_pp_sampler(net, lat, afs=True, return_denoised=True, max_order=2, **kw)
    xt0, eps0 = solvers.dpm_pp_sampler(net, lat, afs=True, max_order=2, **kw)
    assert torch.equal(xt, xt0) and torch.equal(eps, eps0)
    x0 = xt[0]
    afs_d = x0 - t[0] * (x0 / (1 + t[0] ** 2) ** 0.5)                              # the reference's x - t d of the analytical first step
    assert torch.allclose(den[0], afs_d, rtol=1e-5, atol=1e-5 * float(x0.abs().max()))
    assert torch.equal(den[1], _direct_denoised(net, lat, ts, [(xt[1], t[1])])[0])
    third = solvers.euler_sampler(net, lat, num_steps=NUM_POINTS, t_steps=ts, return_inters=True, return_denoised=True)
    assert len(third) == 3 and third[2] is None                                    # no eps asked for, none returned
