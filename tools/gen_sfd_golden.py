"""Regenerate tests/golden/sfd_*.npz by running the REFERENCE step-conditioned EDMPrecond (SongUNet / DhariwalUNet) and its Euler sampler on the CPU.

    python tools/gen_sfd_golden.py --reference /path/to/sfd-main

The reference classes (models/networks_edm.py) and the sampler (solvers.py) are imported at run time from that directory; nothing of their text
is copied here, and the fixtures hold inputs and recorded results only.  Weights are never stored: they are
``arch.init_params(spec_with_step_condition, seed)`` loaded into the reference with strict=False, where only ``resample_filter`` buffers may be
missing.

Files (compressed):
  sfd_net_<config>.npz     tiny_song, tiny_song_cond, tiny_adm, tiny_ncsnpp, cifar10, imagenet64, B = 2 each: x, sigma = [80, 1.7], labels,
                           out_none (no step condition), out_step4 (per-sample sigma), out_step4_scalar (sigma = 0.6), out_step6, and the
                           reference's state-dict keys and shapes (without the resample_filter buffers)
  sfd_sampler_tiny.npz     tiny_song and tiny_adm, B = 2: euler_sampler(step_condition=4, return_inters=True) with afs=True, num_steps=4 and
                           with afs=False, num_steps=3
  sfd_ldm_tiny.npz         tiny_ldm_1res under CFGPrecond (guidance 7.5, LatentDiffusion replaced by a shim that exposes alphas_cumprod and an
                           apply_model forwarding step_condition, as oracle/gen_golden.py does), B = 3: x, sigma = [11, 0.7, 2.3], cond, uncond,
                           out_none, out_step4, the U-Net's state-dict keys and shapes, and the 4-step discrete-schedule Euler trajectory with
                           step_condition=4

Per net the generator asserts rel(out_step4, out_none) > 1e-2 and rel(out_step4, out_step6) > 2e-3: a test on these files cannot pass with the
condition ignored or frozen.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, ROOT)

NETS = [('tiny_song', 2, 81), ('tiny_song_cond', 2, 82), ('tiny_adm', 2, 83), ('tiny_ncsnpp', 2, 84), ('cifar10', 2, 85), ('imagenet64', 2, 86)]
SAMPLERS = [('tiny_song', 87), ('tiny_adm', 88)]


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


def ref_net(name, seed):
    import diff_sampler_amd.arch as arch
    from models.networks_edm import EDMPrecond
    kw = dict(arch.NAMED_CONFIGS[name])
    spec = arch.edm_precond_spec(**kw, step_condition=True)
    net = EDMPrecond(**kw).eval().requires_grad_(False)
    missing, unexpected = net.load_state_dict(arch.init_params(spec, seed=seed), strict=False)
    assert not unexpected and all('resample_filter' in m for m in missing), (missing, unexpected)
    return net, kw, spec


def ref_cfg_net(name, seed, guidance_rate=7.5):
    """The reference CFGPrecond around the reference step-conditioned UNetModel, weights from ldm_arch.init_ldm_params; the `omegaconf` import
    of the reference's ldm package is satisfied by an empty stand-in where the library is absent."""
    import types
    if 'omegaconf' not in sys.modules:
        try:
            import omegaconf  # noqa: F401
        except ImportError:
            m, lc = types.ModuleType('omegaconf'), types.ModuleType('omegaconf.listconfig')
            lc.ListConfig = type('ListConfig', (list,), {})
            m.listconfig = lc
            sys.modules['omegaconf'], sys.modules['omegaconf.listconfig'] = m, lc
    import diff_sampler_amd.ldm_arch as la
    from models.ldm.modules.diffusionmodules.openaimodel import UNetModel
    from models.networks_edm import CFGPrecond
    kw = dict(la.NAMED_LDM_CONFIGS[name])
    spec = la.ldm_unet_spec(**kw, step_condition=True)
    unet = UNetModel(image_size=32, in_channels=kw['in_channels'], out_channels=kw['out_channels'], model_channels=kw['model_channels'],
                     attention_resolutions=list(kw['attention_resolutions']), num_res_blocks=kw['num_res_blocks'],
                     channel_mult=list(kw['channel_mult']), num_heads=kw['num_heads'], use_spatial_transformer=True,
                     transformer_depth=1, context_dim=kw['context_dim'], use_checkpoint=False, legacy=False).eval()
    unet.load_state_dict(la.init_ldm_params(spec, seed=seed), strict=True)

    class Shim(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.unet = unet
            self.register_buffer('alphas_cumprod', la.alphas_cumprod(spec))

        def apply_model(self, x, t, cond, step_condition=None):
            return self.unet(x, t, context=cond, step_condition=step_condition)

    net = CFGPrecond(Shim(), img_resolution=kw['img_resolution'], img_channels=kw['in_channels'], guidance_rate=guidance_rate,
                     guidance_type='classifier-free', label_dim=True).eval()
    return net, unet, kw, spec


def ldm_part(solvers):
    name, B, seed = 'tiny_ldm_1res', 3, 89
    net, unet, kw, spec = ref_cfg_net(name, seed)
    g = torch.Generator().manual_seed(seed + 100)
    R, Cc, ctx = kw['img_resolution'], kw['in_channels'], kw['context_dim']
    sig = torch.tensor([11.0, 0.7, 2.3][:B])
    x = torch.randn(B, Cc, R, R, generator=g) * sig.reshape(-1, 1, 1, 1)
    cond, uncond = torch.randn(B, 77, ctx, generator=g), torch.randn(B, 77, ctx, generator=g)
    lat = torch.randn(B, Cc, R, R, generator=g)
    out_none = net(x, sig, condition=cond, unconditional_condition=uncond)
    out4 = net(x, sig, condition=cond, unconditional_condition=uncond, step_condition=4)
    out6 = net(x, sig, condition=cond, unconditional_condition=uncond, step_condition=6)
    moved = (rel(out4, out_none), rel(out4, out6))
    assert moved[0] > 1e-2 and moved[1] > 2e-3, moved
    tr = solvers.euler_sampler(net, lat, condition=cond, unconditional_condition=uncond, num_steps=4, sigma_min=net.sigma_min, sigma_max=net.sigma_max,
                               schedule_type='discrete', schedule_rho=1, step_condition=4, return_inters=True)
    keys = [(k, list(v.shape)) for k, v in unet.state_dict().items()]
    np.savez_compressed(os.path.join(OUT, 'sfd_ldm_tiny.npz'), config=name, seed=seed, x=x.numpy(), sigma=sig.numpy(), cond=cond.numpy(),
                        uncond=uncond.numpy(), latents=lat.numpy(), out_none=out_none.numpy(), out_step4=out4.numpy(), out_step6=out6.numpy(),
                        traj_euler=tr.numpy(), sigma_min=net.sigma_min, sigma_max=net.sigma_max, state_dict=json.dumps(keys))
    print(f'ldm {name}: |out| {float(out4.abs().max()):.3g}, step 4 vs none {moved[0]:.3g}, 4 vs 6 {moved[1]:.3g}, trajectory {tuple(tr.shape)}', flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', required=True, help='directory of the reference project that holds models/networks_edm.py and solvers.py')
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    from oracle.cases import make_inputs
    torch.set_grad_enabled(False)
    for name, B, seed in NETS:
        net, kw, spec = ref_net(name, seed)
        x, lab = make_inputs(kw, B, seed + 100)
        sig = torch.tensor([80.0, 1.7][:B])
        x = x * sig.reshape(-1, 1, 1, 1)
        out_none = net(x, sig, class_labels=lab)
        out4 = net(x, sig, class_labels=lab, step_condition=4)
        out4_sc = net(x, torch.tensor(0.6), class_labels=lab, step_condition=4)
        out6 = net(x, sig, class_labels=lab, step_condition=6)
        moved = (rel(out4, out_none), rel(out4, out6))
        assert moved[0] > 1e-2 and moved[1] > 2e-3, (name, moved)
        keys = [(k, list(v.shape)) for k, v in net.state_dict().items() if 'resample_filter' not in k]
        np.savez_compressed(os.path.join(OUT, f'sfd_net_{name}.npz'), config=name, seed=seed, x=x.numpy(), sigma=sig.numpy(),
                            labels=(lab.numpy() if lab is not None else np.zeros(0, np.float32)), out_none=out_none.numpy(), out_step4=out4.numpy(),
                            out_step4_scalar=out4_sc.numpy(), out_step6=out6.numpy(), state_dict=json.dumps(keys))
        print(f'{name}: |out| {float(out4.abs().max()):.3g}, step 4 vs none {moved[0]:.3g}, 4 vs 6 {moved[1]:.3g}, {len(keys)} keys', flush=True)

    import solvers
    d = {}
    for name, seed in SAMPLERS:
        net, kw, spec = ref_net(name, seed)
        latents, lab = make_inputs(kw, 2, seed + 100)
        d[f'{name}_seed'], d[f'{name}_latents'] = seed, latents.numpy()
        d[f'{name}_labels'] = lab.numpy() if lab is not None else np.zeros(0, np.float32)
        for tag, kws in (('afs4', dict(afs=True, num_steps=4)), ('plain3', dict(afs=False, num_steps=3))):
            tr = solvers.euler_sampler(net, latents, class_labels=lab, sigma_min=0.002, sigma_max=80., schedule_type='polynomial', schedule_rho=7,
                                       step_condition=4, return_inters=True, **kws)
            d[f'{name}_{tag}'] = tr.numpy()
            print('sampler', name, tag, tuple(tr.shape), float(tr[-1].abs().max()), flush=True)
    np.savez_compressed(os.path.join(OUT, 'sfd_sampler_tiny.npz'), **d)
    ldm_part(solvers)


if __name__ == '__main__':
    main()
