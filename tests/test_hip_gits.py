"""GPU: GITS schedule search (cost matrix from trajectory moments, DP, AFS slot search) against the real reference's
outputs on the same seeded warm-up latents (tests/golden/gits.npz, made by oracle/gen_golden.py --part gits), and the cost
kernels themselves (moments, closed-form 'dev' cost, 'l1' / 'l2' pair kernel) against fp64 restatements of the definition."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

from oracle import cases  # noqa: E402

G = os.path.join(ROOT, 'tests', 'golden')


def test_cal_deviation_matches_reference():
    from diff_sampler_amd import gits_utils
    z = np.load(os.path.join(G, 'gits.npz'))
    dev = gits_utils.cal_deviation(torch.from_numpy(z['dev_traj']).cuda(), 3, 16, bs=3)
    assert np.allclose(dev.cpu().numpy(), z['dev_out'], rtol=2e-5, atol=1e-5)


@pytest.mark.parametrize('tag', [c[0] for c in cases.GITS_CASES])
def test_get_dp_list_matches_reference(tag):
    from diff_sampler_amd import gits_utils
    from diff_sampler_amd.engine import EDMDenoiser
    z = np.load(os.path.join(G, 'gits.npz'))
    net = EDMDenoiser.from_config('tiny_song', seed=int(z['seed']))
    gk = dict(cases.GITS_CASES)[tag]
    kwargs = dict(cases.GITS_COMMON); kwargs.update(gk)
    rounds = kwargs['num_warmup'] // (kwargs['max_batch_size'] + 1) + 1
    lat = cases.gits_warmup_latents(1000 + len(tag), rounds, kwargs['max_batch_size'], (3, 16, 16))
    dp_list = gits_utils.get_dp_list(net, torch.device('cuda'), warmup_latents=lat, **kwargs)
    assert list(dp_list) == list(z[f'{tag}_dp_list']), (tag, dp_list, z[f'{tag}_dp_list'])
    # the searched schedule is consumed exactly like the reference does (gits-main/solver_utils.py:52-53)
    from diff_sampler_amd import solver_utils
    ts = solver_utils.get_schedule(kwargs['num_steps_tea'], 0.002, 80., device='cuda', schedule_type=kwargs['schedule_type'],
                                   schedule_rho=kwargs['schedule_rho'], dp_list=dp_list)
    assert ts.shape[0] == len(dp_list) and float(ts[0]) > float(ts[-1])


def test_get_dp_list_on_the_full_size_cifar10_net_matches_reference():
    """The schedule search itself (gits-main/gits_utils.py:42-255) on the FULL-size CIFAR-10 net against the real reference
    (oracle/gen_golden.py --part fullgits): 21-step iPNDM-4 teacher on 8 warm-up latents, 'dev' cost, 6-step student."""
    from diff_sampler_amd import gits_utils
    from diff_sampler_amd.engine import EDMDenoiser
    z = np.load(os.path.join(G, 'gits_cifar10.npz'))
    net = EDMDenoiser.from_config('cifar10', seed=int(z['seed']))
    tag, gk = cases.GITS_FULL_CASE
    kwargs = dict(cases.GITS_COMMON); kwargs.update(gk)
    rounds = kwargs['num_warmup'] // (kwargs['max_batch_size'] + 1) + 1
    lat = cases.gits_warmup_latents(int(z['warmup_seed']), rounds, kwargs['max_batch_size'], (3, 32, 32))
    dp_list = gits_utils.get_dp_list(net, torch.device('cuda'), warmup_latents=lat, **kwargs)
    assert list(dp_list) == list(z['dp_list']), (dp_list, z['dp_list'])


def test_get_dp_list_on_a_latent_diffusion_denoiser_matches_reference():
    """model_source == 'ldm' (gits-main/gits_utils.py:86-108): text conditions instead of labels, classifier-free guidance inside the
    denoiser, 'discrete' schedule from the net's own sigma(t).  Golden = the REAL reference's get_dp_list on the tiny LDM U-Net with a
    shimmed text encoder (oracle/gen_golden.py --part gitsldm); here the same latents and conditions go through the HIP CFGDenoiser."""
    from diff_sampler_amd import gits_utils
    from diff_sampler_amd.ldm_engine import CFGDenoiser
    import diff_sampler_amd.ldm_arch as la
    z = np.load(os.path.join(G, 'gits_ldm.npz'))
    net = CFGDenoiser.from_config('tiny_ldm', seed=int(z['seed']), guidance_rate=7.5)
    assert abs(net.sigma_min - float(z['sigma_min'])) < 1e-6 and abs(net.sigma_max - float(z['sigma_max'])) < 1e-4
    tag, gk = cases.GITS_LDM_CASE
    kwargs = dict(cases.GITS_COMMON); kwargs.update(gk)
    kwargs['sigma_min'], kwargs['sigma_max'] = net.sigma_min, net.sigma_max
    kw = la.NAMED_LDM_CONFIGS['tiny_ldm']
    rounds = kwargs['num_warmup'] // (kwargs['max_batch_size'] + 1) + 1
    lat = cases.gits_warmup_latents(int(z['warmup_seed']), rounds, kwargs['max_batch_size'], (kw['in_channels'], kw['img_resolution'], kw['img_resolution']))
    conds = cases.gits_ldm_conditions(int(z['cond_seed']), rounds, kwargs['max_batch_size'], kw['context_dim'])
    dp_list = gits_utils.get_dp_list(net, torch.device('cuda'), warmup_latents=lat, warmup_conditions=conds, **kwargs)
    assert list(dp_list) == list(z['dp_list']), (dp_list, z['dp_list'])
    # without the test hooks the search draws its own conditions (seeded N(0,1) CLIP-shaped states for an engine net) and still returns a path
    dp2 = gits_utils.get_dp_list(net, torch.device('cuda'), **kwargs)
    assert dp2[0] == 0 and dp2[-1] == kwargs['num_steps_tea'] - 1 and len(dp2) == kwargs['num_steps']


# ------------------------------------------------------------------------------------------------------------------------------
# The cost kernels against the cost's definition (tests/_kernel_refs.py: fp64 on the CPU, synthetic trajectories, no network).  The
# dp_list tests above see the cost matrix only through the argmin path of the dynamic programme.

sys.path.insert(0, os.path.join(ROOT, 'tests'))
import _kernel_refs as R  # noqa: E402

_TRAJ = {}


def _traj(shape):
    """(traj, eps, t) of one synthetic trajectory on the CPU and (traj, eps) on the device, made once per shape."""
    if shape not in _TRAJ:
        traj, eps, t = R.degenerate_trajectory() if shape == 'degenerate' else R.synthetic_trajectory(*shape)
        _TRAJ[shape] = (traj, eps, t, traj.cuda(), eps.cuda())
    return _TRAJ[shape]


@pytest.mark.parametrize('shape', R.TRAJ_SHAPES)
@pytest.mark.parametrize('with_eps', [False, True])
def test_trajectory_moments_match_fp64_dot_products(shape, with_eps):
    from diff_sampler_amd import gits_utils
    traj, eps, _, traj_d, eps_d = _traj(shape)
    got = gits_utils.trajectory_moments(traj_d, eps_d if with_eps else None)
    ref, ref_abs = R.traj_moments_ref(traj, eps if with_eps else None)
    assert got.shape == ref.shape == (shape[0], shape[1], 6)
    assert np.all(np.abs(got - ref) <= 1e-12 * ref_abs), float((np.abs(got - ref) / np.maximum(ref_abs, 1e-300)).max())
    if not with_eps:
        assert np.all(got[:, :, [1, 3, 4]] == 0)                 # Q, S, T: no direction tensor


@pytest.mark.parametrize('shape', R.TRAJ_SHAPES)
@pytest.mark.parametrize('metric', ['dev', 'l1', 'l2'])
def test_cost_matrix_matches_the_definition(shape, metric):
    """Every pair i < j: 'dev' (closed form from the six moments) within 1e-12 * s, 'l1' / 'l2' (fp32 jump and difference, fp64 sums and
    atomicAdd over the batch) within the fp32 bound of the jump's three operands.  One value per sample puts every point on the chord:
    there the closed form cancels to the square root of its rounding noise and the degenerate bound 1e-7 * s holds instead."""
    from diff_sampler_amd import gits_utils
    traj, eps, t, traj_d, eps_d = _traj(shape)
    cost = gits_utils._cost_matrix_round(traj_d, eps_d, t, metric)
    ref, tol = R.pair_costs_ref(traj, eps, t, metric)
    if metric == 'dev' and shape[2] == 1:
        tol = tol * 1e5
    n = shape[0]
    iu = np.triu_indices(n, 1)
    print(metric, shape, 'worst error / bound', float((np.abs(cost - ref)[iu] / tol[iu]).max()))
    assert cost.shape == (n, n) and np.all(np.abs(cost - ref)[iu] <= tol[iu])
    assert np.all(cost[np.tril_indices(n)] == 0)


def test_dev_cost_on_a_trajectory_that_lies_on_its_chord():
    from diff_sampler_amd import gits_utils
    traj, eps, t, traj_d, eps_d = _traj('degenerate')
    cost = gits_utils._cost_matrix_round(traj_d, eps_d, t, 'dev')
    ref, tol = R.pair_costs_ref(traj, eps, t, 'dev')
    iu = np.triu_indices(len(t), 1)
    assert np.all(np.abs(cost - ref)[iu] <= 1e5 * tol[iu]), float((np.abs(cost - ref)[iu] / tol[iu]).max())       # 1e-7 * s


@pytest.mark.parametrize('shape', R.TRAJ_SHAPES)
def test_cal_deviation_matches_the_definition(shape):
    """fp32 result of the fp64 closed form sqrt(R - P^2 / N): one fp32 rounding plus 1e-12 of its scale sqrt(R) = |c - x_j|."""
    from diff_sampler_amd import gits_utils
    traj, _, _, traj_d, _ = _traj(shape)
    dev = gits_utils.cal_deviation(traj_d)
    ref, Rj = R.deviation_ref(traj)
    assert tuple(dev.shape) == ref.shape == (shape[1], shape[0] - 2) and dev.dtype == torch.float32 and dev.is_cuda
    assert np.all(np.abs(dev.cpu().double().numpy() - ref) <= R.U * ref + 1e-12 * np.sqrt(Rj))


@pytest.mark.parametrize('shape', R.TRAJ_SHAPES)
@pytest.mark.parametrize('p_norm', [1, 2])
def test_traj_pair_cost_accumulates_and_leaves_the_lower_triangle_zero(shape, p_norm):
    """ds_traj_pair_cost adds into `cost`: a second call on the same buffer doubles it.  With one sample per pair that is exact (v + v);
    with B samples the second round's B atomicAdds each round once in fp64, in any order, onto partial sums that stay below twice the
    first result (every term is a norm, >= 0): |second - 2 first| <= B * 2^-52 * 2 first."""
    import ctypes as C
    from diff_sampler_amd import _lib
    _, _, t, traj_d, eps_d = _traj(shape)
    n, B, per = shape
    cost = torch.zeros(n, n, dtype=torch.float64, device='cuda')
    td = torch.tensor(t, dtype=torch.float32, device='cuda')
    call = lambda: _lib.load().ds_traj_pair_cost(C.c_void_p(traj_d.data_ptr()), C.c_void_p(eps_d.data_ptr()), C.c_void_p(td.data_ptr()), n, B,
                                                 per, p_norm, C.c_void_p(cost.data_ptr()), _lib.stream_ptr())
    assert call() == 0
    first = cost.cpu().numpy().copy()
    assert call() == 0
    second = cost.cpu().numpy()
    assert np.all(first[np.tril_indices(n)] == 0) and np.all(second[np.tril_indices(n)] == 0)
    assert np.all(first[np.triu_indices(n, 1)] > 0)
    if B == 1:
        assert np.array_equal(second, 2 * first)
    else:
        assert np.all(np.abs(second - 2 * first) <= B * 2.0 ** -52 * 2 * first)
