"""GPU: the AMED samplers on the latent-diffusion denoiser under classifier-free guidance (``ldm_engine.CFGDenoiser``; the reference's
Stable Diffusion recipe is AMED-Plugin on DPM-Solver++(2M), amed-solver-main/launch.sh:55-62) against what the REAL reference recorded
(tests/golden/amed_ldm_tiny.npz, tools/gen_golden_amed_ldm.py), and the two kernels the route adds, both plan operations of the library: ``DS_OP_CHANNEL_MEAN_F16``
(the tap's channel mean over fp16 rows) and ``DS_OP_CFG_SIGMA_ROWS`` (sigma -> c_noise rows on the device).

Tolerances: 1e-3 of the trajectory scale (tests/test_hip_ldm.py, tests/test_hip_amed.py; the generator's issue measured that rounding is
amplified < 3x along these trajectories while a wrong tap half moves them by >= 0.8 %), 2e-4 per evaluation, 1e-5 for the channel means
(fp32 accumulation of <= 1280 terms: ~sqrt(c) * 6e-8 of the row scale)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
G = os.path.join(ROOT, 'tests', 'golden')
TOL = 1e-3


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda')


@pytest.fixture(scope='module')
def gold():
    z = np.load(os.path.join(G, 'amed_ldm_tiny.npz'))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope='module')
def net(gold, dev):
    from diff_sampler_amd.ldm_engine import CFGDenoiser
    return CFGDenoiser.from_config(str(gold['config']), seed=int(gold['seed']), guidance_rate=7.5)


def _inputs(gold, dev):
    return tuple(torch.from_numpy(gold[k]).to(dev) for k in ('latents', 'cond', 'uncond'))


def _fns():
    from diff_sampler_amd import solvers_amed
    return dict(amed=solvers_amed.amed_sampler, euler=solvers_amed.euler_sampler, ipndm=solvers_amed.ipndm_sampler,
                dpm=solvers_amed.dpm_2_sampler, dpmpp=solvers_amed.dpm_pp_sampler)


def _predictor(gold, dev, case, common):
    from diff_sampler_amd import solvers_amed
    from oracle import cases
    pp = cases.amed_predictor_params(int(gold['pred_seed']), case['scale_dir'], case['scale_time'])
    return solvers_amed.AMEDPredictor(pp, device=dev, num_steps=common['num_steps'], sampler_stu=case['student'],
                                      schedule_type=common['schedule_type'], schedule_rho=common['schedule_rho'], afs=case['afs'],
                                      scale_dir=case['scale_dir'], scale_time=case['scale_time'], **case['kwargs'])


def _sample(net, gold, dev, tag, num_steps=None, **over):
    spec = json.loads(str(gold['cases_json']))
    common, case = spec['common'], spec['cases'][tag]
    lat, cond, uncond = _inputs(gold, dev)
    pred = _predictor(gold, dev, case, common)
    kw = dict(condition=cond, unconditional_condition=uncond, num_steps=(num_steps or common['num_steps']), sigma_min=net.sigma_min,
              sigma_max=net.sigma_max, schedule_type=common['schedule_type'], schedule_rho=common['schedule_rho'], afs=case['afs'],
              AMED_predictor=pred, **case['kwargs'])
    kw.update(over)
    out = _fns()[case['student']](net, lat, **kw)
    torch.cuda.synchronize()
    return out


def test_amed_ldm_trajectories_match_reference(net, gold, dev):
    """All six recorded cases -- the five samplers, both predict_x0 settings, AFS on and off -- against the reference's trajectories."""
    spec = json.loads(str(gold['cases_json']))
    assert abs(net.sigma_min - float(gold['sigma_min'])) < 1e-6 and abs(net.sigma_max - float(gold['sigma_max'])) < 1e-4
    checked = 0
    for tag in spec['cases']:
        want = torch.from_numpy(gold[f'{tag}_inters'])
        inters = _sample(net, gold, dev, tag, return_inters=True)
        assert tuple(inters.shape) == tuple(want.shape) == (4, 2, 4, 32, 32), (tag, inters.shape)
        err = _rel(inters.cpu(), want)
        print(f'{tag}: trajectory rel err {err:.3e}')
        assert err < TOL, (tag, err)
        out = _sample(net, gold, dev, tag)
        assert tuple(out.shape) == (2, 4, 32, 32) and _rel(out.cpu(), want[-1]) < TOL, tag
        checked += 1
    assert checked == 6


def test_amed_ldm_tap_and_prediction_shims(net, gold, dev):
    """`block_output('middle_block.2')` is what the reference's forward hook on `...diffusion_model.middle_block` recorded ([2B, C, 8, 8],
    unconditional half first); `bottleneck_mean` is the channel mean of its conditional half; `init_hook` / `get_amed_prediction` give the
    reference's r, scale_dir, scale_time -- from the tap, under AFS (zeros) and from a plain list of [2B, C, h, w] tensors."""
    from diff_sampler_amd import solvers_amed
    from oracle import cases
    B = 2
    x, (_, cond, uncond) = torch.from_numpy(gold['tap_x']).to(dev), _inputs(gold, dev)
    tap, hook = solvers_amed.init_hook(net)
    d = net(x, float(gold['tap_sigma']), condition=cond, unconditional_condition=uncond)
    torch.cuda.synchronize()
    assert _rel(d.cpu(), torch.from_numpy(gold['tap_denoised'])) < 2e-4
    got = net.block_output('middle_block.2')
    want = torch.from_numpy(gold['tap_out'])
    assert tuple(got.shape) == tuple(want.shape) == (2 * B, 128, 8, 8) and got.is_contiguous() and got.dtype == torch.float32
    assert _rel(got.cpu(), want) < 2e-4
    assert len(tap) == 1 and torch.equal(tap[-1], got)
    plan, b_, doubled = net._last
    assert b_ == B and doubled
    bm = net.bottleneck_mean(plan, B, doubled)
    assert tuple(bm.shape) == (B, 8, 8) and _rel(bm.cpu(), got[B:].mean(1).cpu()) < 1e-5
    assert _rel(bm.cpu(), got[:B].mean(1).cpu()) > 1e-3           # ... and not the unconditional half

    sd, st = float(gold['tap_scale_dir_setting']), float(gold['tap_scale_time_setting'])
    pred = solvers_amed.AMEDPredictor(cases.amed_predictor_params(int(gold['pred_seed']), sd, st), device=dev, scale_dir=sd, scale_time=st)
    t_cur, t_next = torch.tensor(float(gold['tap_sigma'])), torch.tensor(float(gold['tap_t_next']))
    for use_afs, pre in ((False, 'tap_'), (True, 'tap_afs_')):
        res = solvers_amed.get_amed_prediction(pred, t_cur, t_next, net, tap, use_afs, B)
        for got_, key in zip(res, ('r', 'scale_dir', 'scale_time')):
            assert got_.shape == (B, 1, 1, 1)
            assert torch.allclose(got_.cpu().flatten(), torch.from_numpy(gold[pre + key]).flatten(), rtol=2e-4, atol=1e-5), (pre, key)
    a = solvers_amed.get_amed_prediction(pred, t_cur, t_next, net, tap, False, B)
    b = solvers_amed.get_amed_prediction(pred, t_cur, t_next, net, [tap[-1]], False, B)       # the reference's own list form: sliced [B:]
    assert all(torch.allclose(p, q, rtol=1e-5, atol=1e-6) for p, q in zip(a, b))

    # an evaluation that is not doubled has no conditional half to read
    net(x, float(gold['tap_sigma']), condition=cond, unconditional_condition=None)
    with pytest.raises(ValueError, match='not doubled'):
        solvers_amed.get_amed_prediction(pred, t_cur, t_next, net, tap, False, B)
    with pytest.raises(ValueError, match='not doubled'):
        solvers_amed.get_amed_prediction(pred, t_cur, t_next, net, [got[:B]], False, B)
    hook.remove()
    with pytest.raises(RuntimeError):
        tap[-1]


def test_amed_ldm_refuses_what_it_cannot_run(net, gold, dev):
    """No unconditional condition / guidance_rate == 1 (the reference would slice an empty tensor) and a predictor whose input width is not
    the tap's h * w: ValueError, before any launch."""
    from diff_sampler_amd import solvers_amed
    from oracle import cases
    with pytest.raises(ValueError, match='not doubled'):
        _sample(net, gold, dev, 'amed', unconditional_condition=None)
    rate = net.guidance_rate                        # an attribute read at every evaluation, as in the reference's CFGPrecond
    try:
        net.guidance_rate = 1.0
        with pytest.raises(ValueError, match='guidance_rate'):
            _sample(net, gold, dev, 'dpmpp2_eps_afs')
    finally:
        net.guidance_rate = rate
    pp = cases.amed_predictor_params(3, 0.01, 0)
    pp['enc_layer0.weight'] = pp['enc_layer0.weight'][:, :16].contiguous()         # a predictor for a 4x4 tap
    bad = solvers_amed.AMEDPredictor(pp, device=dev, scale_dir=0.01)
    last = net._last
    with pytest.raises(ValueError, match='enc_layer0'):
        _sample(net, gold, dev, 'amed', AMED_predictor=bad)
    assert net._last is last                                                        # nothing was evaluated


@pytest.mark.parametrize('rows,c,ld', [(128, 128, 128), (130, 96, 160), (64 * 3, 1280, 1280), (1, 8, 8), (3, 10, 12)])
def test_channel_mean_f16_kernel(rows, c, ld, dev):
    """DS_OP_CHANNEL_MEAN_F16 on synthetic fp16 rows: SD-1.5's tap (1280 channels, 8x8, three images), a ragged row count with ld > c, one
    row of one 16-byte chunk, and (3, 10, 12), which takes the kernel's unvectorised path; whole and from a pointer offset by half the rows;
    nothing is written outside `rows`."""
    from diff_sampler_amd import ops
    g = torch.Generator().manual_seed(rows * 7 + c)
    x = (torch.randn(rows, ld, generator=g) + 0.5).to(torch.float16).to(dev)
    want = x[:, :c].float().mean(1)
    scale = x[:, :c].float().abs().max(1).values
    for first in sorted({0, rows // 2}):
        n = rows - first
        out = torch.full((rows + 5,), -77.0, device=dev)
        ops.channel_mean_f16(x[first:], ld, c, n, out)
        torch.cuda.synchronize()
        err = ((out[:n] - want[first:]).abs() / scale[first:]).max().item()
        assert err < 1e-5, (first, err)
        assert bool((out[n:] == -77.0).all())


def _c_noise_f64(log_alpha, sigma):
    """float64 evaluation of CFGPrecond's formulas (networks_edm.py:677, :713-759) on the fp32 log_alpha table."""
    la = log_alpha.double().cpu()
    M = la.numel()
    x = -0.5 * torch.log1p(sigma.double().cpu() ** 2)
    xp, yp = torch.flip(la, [0]), torch.flip(torch.arange(1, M + 1, dtype=torch.float64) / M, [0])
    i = torch.searchsorted(xp, x.contiguous()).clamp(1, M - 1) - 1
    t = yp[i] + (x - xp[i]) * (yp[i + 1] - yp[i]) / (xp[i + 1] - xp[i])
    return M * t - 1.


def test_cfg_sigma_rows_kernel(net, gold, dev):
    """DS_OP_CFG_SIGMA_ROWS at the golden's 64 probe sigmas (log-uniform over [sigma_min / 2, 2 sigma_max]: both linear extensions are hit).
    The bound is measured: twice the largest distance of the HOST path (CFGSchedule.sigma_inv, an fp32 evaluation pinned to the real
    reference by tests/test_hip_ldm.py) from a float64 evaluation of the same formulas on the same fp32 table."""
    from diff_sampler_amd import ops
    probe = torch.from_numpy(gold['probe_sigma'])
    table = net.log_alpha_array.to(dev, torch.float32).contiguous()
    want = _c_noise_f64(net.log_alpha_array, probe)
    assert float(want.min()) < 0 and float(want.max()) > net.M - 1
    host = (net.M * net.sigma_inv(probe) - 1.).double()
    d_host = float((host - want).abs().max())
    d_ref = float((torch.from_numpy(gold['probe_c_noise']).double() - want).abs().max())
    worst = 0.0
    for n, idx in ((1, [0]), (5, [0, 1, 31, 62, 63]), (64, list(range(64)))):
        sg = probe[idx].to(dev).contiguous()
        for copies in (1, 2):
            s_out = torch.full((copies * n + 3,), -5.0, device=dev)
            c_out = torch.full((copies * n + 3,), -5.0, device=dev)
            ops.cfg_sigma_rows(sg, n, table, copies, s_out, c_out)
            torch.cuda.synchronize()
            assert bool((s_out[copies * n:] == -5.0).all()) and bool((c_out[copies * n:] == -5.0).all())
            for k in range(copies):
                assert torch.equal(s_out[k * n:(k + 1) * n], sg)                                    # sigma copied exactly
                assert torch.equal(c_out[k * n:(k + 1) * n], c_out[:n])                             # both halves equal
            d = float((c_out[:n].double().cpu() - want[idx]).abs().max())
            worst = max(worst, d)
            assert d <= 2 * d_host, (n, copies, d, d_host)
    print(f'c_noise distance from float64: device {worst:.3e}, host path {d_host:.3e}, recorded reference {d_ref:.3e}')


def test_amed_ldm_no_host_round_trip_per_step(net, gold, dev, monkeypatch):
    """The per-sample sigma of every evaluation stays on the device: `sigma_inv` (a D2H copy, CPU interpolation, an H2D copy) is called by
    get_schedule only, so the count does not depend on the number of steps.  With the device route switched off it does -- which shows
    that the counter sees the host route."""
    from diff_sampler_amd import solvers_amed
    calls = [0]
    real = net.sigma_inv

    def counting(sigma):
        calls[0] += 1
        return real(sigma)
    monkeypatch.setattr(net, 'sigma_inv', counting, raising=False)

    def count(num_steps):
        calls[0] = 0
        _sample(net, gold, dev, 'dpmpp2_x0', num_steps=num_steps)
        return calls[0]
    n4, n6 = count(4), count(6)
    assert n4 == n6 == 2, (n4, n6)                        # the two end points of the discrete schedule (solver_utils.get_schedule)
    monkeypatch.setattr(solvers_amed, 'DEVICE_SIGMA', False)
    h4, h6 = count(4), count(6)
    assert h4 > n4 and h6 > h4, (h4, h6)


def test_amed_ldm_fp16_mode(net, gold, dev):
    """`use_fp16=True`: the tap of this geometry lives on the fp16 stream (the plan's `middle_block.2` rows are float16), so the sampler
    reads it through DS_OP_CHANNEL_MEAN_F16.  The reference's SD recipe (`dpmpp2_eps_afs`) against the fp32 golden; the bound is measured
    here from code the AMED route does not touch: the distance of the fp16-mode PLAIN DPM-Solver++(2M) trajectory from the fp32-mode one
    (same net, inputs, num_steps = 4), times 3 -- the amplification of rounding measured on the reference's AMED trajectories."""
    from diff_sampler_amd import solvers
    from diff_sampler_amd.ldm_engine import CFGDenoiser
    net16 = CFGDenoiser.from_config(str(gold['config']), seed=int(gold['seed']), guidance_rate=7.5, use_fp16=True)
    lat, cond, uncond = _inputs(gold, dev)
    kw = dict(condition=cond, unconditional_condition=uncond, num_steps=4, sigma_min=net.sigma_min, sigma_max=net.sigma_max,
              schedule_type='discrete', schedule_rho=1, return_inters=True, max_order=2, predict_x0=False, lower_order_final=True)
    plain32 = solvers.dpm_pp_sampler(net, lat, **kw)
    plain16 = solvers.dpm_pp_sampler(net16, lat, **kw)
    torch.cuda.synchronize()
    d_plain = _rel(plain16.cpu(), plain32.cpu())
    got = _sample(net16, gold, dev, 'dpmpp2_eps_afs', return_inters=True)
    assert net16._last[0].bufs['middle_block.2'].dtype == torch.float16
    err = _rel(got.cpu(), torch.from_numpy(gold['dpmpp2_eps_afs_inters']))
    print(f'fp16 mode: AMED dpmpp2_eps_afs vs fp32 golden {err:.3e}; plain DPM-Solver++(2M) fp16 vs fp32 {d_plain:.3e} (bound = 3x)')
    assert d_plain > 0 and err < 3 * d_plain, (err, d_plain)


def test_sample_run_ms_coco_amed_predictor(tmp_path, monkeypatch):
    """The reference's B.1 form on the full-size SD-1.5 U-Net (random init): `--predictor_path random:7 --random_init True` builds the
    predictor from the CLI's options, the samplers run AMED-Plugin on DPM-Solver++(2M) under classifier-free guidance, one latent per seed in
    a directory named with NFE = 2 * (2 * 2 - 1) = 6."""
    from diff_sampler_amd import sample
    monkeypatch.chdir(tmp_path)
    out, n = sample.run('ms_coco', predictor_path='random:7', random_init=True, solver='dpmpp', num_steps=3, afs=True, max_order=2,
                        predict_x0=False, lower_order_final=True, schedule_type='discrete', schedule_rho=1, guidance_type='cfg',
                        guidance_rate=7.5, scale_dir=0, scale_time=0.2, max_batch_size=2, seeds='0-1')
    assert n == 2 and os.path.basename(os.path.normpath(out)) == 'dpmpp_nfe6'
    for seed in (0, 1):
        z = np.load(os.path.join(out, '000000', f'{seed:06d}.npy'))
        assert z.shape == (4, 64, 64) and np.isfinite(z).all()
