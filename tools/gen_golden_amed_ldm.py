#!/usr/bin/env python
"""Record tests/golden/amed_ldm_tiny.npz: the AMED samplers on a latent-diffusion denoiser under classifier-free guidance, from the REAL
reference (amed-solver-main/solvers_amed.py, training/networks.py AMED_predictor, models/networks_edm.py CFGPrecond around the ldm
UNetModel), on the CPU.

    python tools/gen_golden_amed_ldm.py                 # write the file
    python tools/gen_golden_amed_ldm.py --check TAG     # run CASES[TAG] again: exit status 0 when it equals the stored trajectory bit for bit

Development machine only: it imports the reference tree (oracle.gen_golden.REF); the tests read the recorded file.  The net is
``ldm_arch.NAMED_LDM_CONFIGS['tiny_ldm_amed']`` with ``init_ldm_params(spec, NET_SEED)`` (middle block [2B, 128, 8, 8]: the reference
hard-codes an 8x8 tap, solvers_amed.py:24), built by ``oracle.gen_golden._ref_cfg_net``; ``net.model.model.diffusion_model`` is pointed at the
U-Net so that the reference's own ``init_hook`` finds ``middle_block`` (solvers_amed.py:11-12).  Predictor weights:
``oracle.cases.amed_predictor_params(PRED_SEED, scale_dir, scale_time)``.  Weights are not stored, inputs and outputs are.

  <tag>_inters     the trajectory [num_steps, B, 4, 32, 32] of CASES[tag] (return_inters=True)
  tap_*            one evaluation net(tap_x, tap_sigma): the hooked middle-block output [2B, 128, 8, 8] and what get_amed_prediction makes of
                   it (r, scale_dir, scale_time), with and without AFS, for the predictor of TAP_PRED
  probe_sigma      64 sigmas: log-uniform over [sigma_min / 2, 2 sigma_max] with both end points (both linear extensions of
  probe_c_noise    CFGPrecond.interpolate_fn are hit), and M * sigma_inv(sigma) - 1 of the reference for them
"""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'amed_ldm_tiny.npz')
sys.path.insert(0, ROOT)

CONFIG, NET_SEED, PRED_SEED, INPUT_SEED, B, CTX_LEN = 'tiny_ldm_amed', 61, 900, 161, 2, 7
COMMON = dict(num_steps=4, schedule_type='discrete', schedule_rho=1, guidance_rate=7.5)
# tag -> (student sampler, afs, scale_dir, scale_time, sampler kwargs); 'dpmpp2_eps_afs' is the reference's Stable Diffusion recipe
# (amed-solver-main/launch.sh:55-62)
CASES = {
    'dpmpp2_eps_afs': ('dpmpp', True, 0, 0.2, dict(max_order=2, predict_x0=False, lower_order_final=True)),
    'dpmpp2_x0': ('dpmpp', False, 0.05, 0.2, dict(max_order=2, predict_x0=True, lower_order_final=True)),
    'amed': ('amed', False, 0.01, 0.1, {}),
    'ipndm3': ('ipndm', True, 0.05, 0.05, dict(max_order=3)),
    'euler': ('euler', False, 0.01, 0, {}),
    'dpm2': ('dpm', False, 0.01, 0.1, {}),
}
TAP_PRED = dict(scale_dir=0.05, scale_time=0.2)
TAP_SIGMA, TAP_T_NEXT = 2.0, 0.7
SAMPLER_FNS = dict(amed='amed_sampler', euler='euler_sampler', ipndm='ipndm_sampler', dpm='dpm_2_sampler', dpmpp='dpm_pp_sampler')


def inputs(context_dim):
    """Latents and text-encoder-shaped states of the cases (seeded CPU generator): (latents, cond, uncond)."""
    g = torch.Generator().manual_seed(INPUT_SEED)
    latents = torch.randn(B, 4, 32, 32, generator=g)
    cond = torch.randn(B, CTX_LEN, context_dim, generator=g)
    uncond = torch.randn(B, CTX_LEN, context_dim, generator=g)
    return latents, cond, uncond


def reference_modules():
    """(solvers_amed module, AMED_predictor class, net, kw) of the real reference, net = CFGPrecond around the tiny U-Net."""
    from oracle import gen_golden
    sys.path.insert(0, os.path.join(gen_golden.REF, 'amed-solver-main'))
    import solvers_amed
    from training.networks import AMED_predictor
    net, unet, kw, _ = gen_golden._ref_cfg_net(CONFIG, NET_SEED, guidance_rate=COMMON['guidance_rate'])
    net.model.model = types.SimpleNamespace(diffusion_model=unet)       # what init_hook walks: net.model.model.diffusion_model.middle_block
    return solvers_amed, AMED_predictor, net, kw


def reference_predictor(AMED_predictor, stu, afs, scale_dir, scale_time, sk):
    from oracle.cases import amed_predictor_params
    pred = AMED_predictor(num_steps=COMMON['num_steps'], sampler_stu=stu, sampler_tea='heun', M=1, guidance_type='cfg',
                          guidance_rate=COMMON['guidance_rate'], schedule_type=COMMON['schedule_type'], schedule_rho=COMMON['schedule_rho'],
                          afs=afs, scale_dir=scale_dir, scale_time=scale_time, dataset_name='ms_coco',
                          **{k: v for k, v in sk.items() if k in ('max_order', 'predict_x0', 'lower_order_final')}).eval()
    pred.load_state_dict(amed_predictor_params(PRED_SEED, scale_dir, scale_time), strict=True)
    return pred


def run_case(mods, tag):
    """The reference's trajectory of CASES[tag]: [num_steps, B, 4, 32, 32]."""
    solvers_amed, AMED_predictor, net, kw = mods
    stu, afs, sd, st, sk = CASES[tag]
    latents, cond, uncond = inputs(kw['context_dim'])
    pred = reference_predictor(AMED_predictor, stu, afs, sd, st, sk)
    with torch.no_grad():
        return getattr(solvers_amed, SAMPLER_FNS[stu])(net, latents, condition=cond, unconditional_condition=uncond,
                                                       num_steps=COMMON['num_steps'], sigma_min=net.sigma_min, sigma_max=net.sigma_max,
                                                       schedule_type=COMMON['schedule_type'], schedule_rho=COMMON['schedule_rho'], afs=afs,
                                                       return_inters=True, AMED_predictor=pred, **sk)


def main():
    mods = reference_modules()
    solvers_amed, AMED_predictor, net, kw = mods
    latents, cond, uncond = inputs(kw['context_dim'])
    d = dict(config=CONFIG, seed=NET_SEED, pred_seed=PRED_SEED, latents=latents.numpy(), cond=cond.numpy(), uncond=uncond.numpy(),
             sigma_min=np.float64(net.sigma_min), sigma_max=np.float64(net.sigma_max),
             cases_json=json.dumps(dict(common=COMMON, cases={t: dict(student=c[0], afs=c[1], scale_dir=c[2], scale_time=c[3], kwargs=c[4])
                                                             for t, c in CASES.items()})))
    for tag in CASES:
        inters = run_case(mods, tag)
        d[f'{tag}_inters'] = inters.numpy()
        print(tag, tuple(inters.shape), 'absmax %.4f' % float(inters[-1].abs().max()))

    # one evaluation with the reference's own hook, and its predictor outputs
    pred = reference_predictor(AMED_predictor, 'dpmpp', False, TAP_PRED['scale_dir'], TAP_PRED['scale_time'], dict(max_order=2))
    x = latents * TAP_SIGMA
    with torch.no_grad():
        tap, hook = solvers_amed.init_hook(net)
        den = net(x, torch.tensor(TAP_SIGMA), condition=cond, unconditional_condition=uncond)
        hook.remove()
        t_cur, t_next = torch.tensor(TAP_SIGMA).reshape(-1, 1, 1, 1), torch.tensor(TAP_T_NEXT).reshape(-1, 1, 1, 1)
        r, sd, st = solvers_amed.get_amed_prediction(pred, t_cur, t_next, net, tap, False, B)
        ra, sda, sta = solvers_amed.get_amed_prediction(pred, t_cur, t_next, net, tap, True, B)
    assert tuple(tap[-1].shape) == (2 * B, 128, 8, 8)
    d.update(tap_x=x.numpy(), tap_sigma=np.float64(TAP_SIGMA), tap_t_next=np.float64(TAP_T_NEXT), tap_out=tap[-1].numpy(), tap_denoised=den.numpy(),
             tap_scale_dir_setting=np.float64(TAP_PRED['scale_dir']), tap_scale_time_setting=np.float64(TAP_PRED['scale_time']),
             tap_r=r.numpy(), tap_scale_dir=sd.numpy(), tap_scale_time=st.numpy(),
             tap_afs_r=ra.numpy(), tap_afs_scale_dir=sda.numpy(), tap_afs_scale_time=sta.numpy())

    lo, hi = net.sigma_min / 2, 2 * net.sigma_max
    probe = torch.cat([torch.tensor([lo]), torch.exp(torch.linspace(np.log(lo), np.log(hi), 64)[1:-1]), torch.tensor([hi])]).to(torch.float32)
    with torch.no_grad():
        cn = net.M * net.sigma_inv(probe) - 1.
    assert probe.shape == (64,) and float(cn.min()) < 0 and float(cn.max()) > net.M - 1        # both extensions are hit
    d.update(probe_sigma=probe.numpy(), probe_c_noise=cn.numpy().astype(np.float32))
    np.savez_compressed(OUT, **d)
    print(os.path.relpath(OUT, ROOT), os.path.getsize(OUT), 'bytes')


def check(tag):
    z = np.load(OUT)
    latents, cond, uncond = inputs(int(z['cond'].shape[-1]))
    same_in = all(np.array_equal(t.numpy(), z[k]) for t, k in ((latents, 'latents'), (cond, 'cond'), (uncond, 'uncond')))
    same = same_in and np.array_equal(run_case(reference_modules(), tag).numpy(), z[f'{tag}_inters'])
    print(tag, 'reproduced' if same else 'DIFFERS')
    return 0 if same else 1


if __name__ == '__main__':
    torch.manual_seed(0)
    if '--check' in sys.argv:
        sys.exit(check(sys.argv[sys.argv.index('--check') + 1]))
    main()
