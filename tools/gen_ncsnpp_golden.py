"""Regenerate tests/golden/ncsnpp_*.npz by running the REFERENCE EDMPrecond / SongUNet with the NCSN++ options, and the reference samplers, on the CPU.

    python tools/gen_ncsnpp_golden.py --reference /path/to/diff-solvers-main

The reference classes (models/networks_edm.py) and samplers (solvers.py) are imported at run time from that directory; nothing of their text
is copied here, and the fixtures hold inputs and recorded results only.  Weights are never stored: they are
``arch.init_params(spec, seed)`` loaded into the reference with strict=False, where only ``resample_filter`` buffers may be missing.

Files (compressed; 70 - 800 KB each):
  ncsnpp_net_<config>.npz     tiny_ncsnpp, tiny_ncsnpp_cond, cifar10_ve, ffhq_ve, B = 2 each: x, sigma = [80, 1.7, 0.05][:B], labels,
                              out_vec (per-sample sigma), out_scalar (sigma = 0.6), the reference's state-dict keys and shapes (without the
                              resample_filter buffers) and, for the tiny nets, every skip-stack tensor after the aux replacement (tap_<name>)
  ncsnpp_sampler_tiny.npz     tiny_ncsnpp, B = 2: dpm_pp_sampler (2M, x0 form, logSNR schedule, 6 steps) and heun_sampler (polynomial, 4 steps)
                              trajectories from the reference's solvers.py
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

NETS = [('tiny_ncsnpp', 2, 71), ('tiny_ncsnpp_cond', 2, 72), ('cifar10_ve', 2, 73), ('ffhq_ve', 2, 74)]
SAMPLER_SEED = 75


def ref_net(name, seed):
    import diff_sampler_amd.arch as arch
    from models.networks_edm import EDMPrecond
    kw = dict(arch.NAMED_CONFIGS[name])
    spec = arch.edm_precond_spec(**kw)
    net = EDMPrecond(**kw).eval().requires_grad_(False)
    missing, unexpected = net.load_state_dict(arch.init_params(spec, seed=seed), strict=False)
    assert not unexpected and all('resample_filter' in m for m in missing), (missing, unexpected)
    return net, kw, spec


def skip_taps(net):
    """Forward hooks on every encoder layer that reproduce the skip stack: an aux_residual layer's OUTPUT is not what is stacked -- the
    stacked tensor is (x + out) / sqrt(2), so it is recomputed from the hooked values the way the forward combines them."""
    vals, hooks = {}, []
    for key, mod in net.model.enc.items():
        hooks.append(mod.register_forward_hook(lambda m, i, o, key=key: vals.__setitem__(key, o.detach().clone())))
    return vals, hooks


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
        sig = torch.tensor([80.0, 1.7, 0.05][:B])
        x = x * sig.reshape(-1, 1, 1, 1)
        vals, hooks = skip_taps(net) if name.startswith('tiny') else ({}, [])
        out_vec = net(x, sig, class_labels=lab)
        for h in hooks:
            h.remove()
        out_sc = net(x, torch.tensor(0.6), class_labels=lab)
        keys = [(k, list(v.shape)) for k, v in net.state_dict().items() if 'resample_filter' not in k]
        d = dict(config=name, seed=seed, x=x.numpy(), sigma=sig.numpy(), labels=(lab.numpy() if lab is not None else np.zeros(0, np.float32)),
                 out_vec=out_vec.numpy(), out_scalar=out_sc.numpy(), state_dict=json.dumps(keys))
        prev = None
        for key, v in vals.items():
            if 'aux_residual' in key:      # x = skips[-1] = aux = (x + block(aux)) / sqrt(2): replaces the entry of the layer before it
                d.pop(f'tap_enc.{prev}')
                v = (vals[prev] + v) / np.sqrt(2)
            d[f'tap_enc.{key}'] = v.numpy()
            prev = key
        np.savez_compressed(os.path.join(OUT, f'ncsnpp_net_{name}.npz'), **d)
        print(name, float(out_vec.abs().max()), float(out_sc.abs().max()), len(keys), sorted(k for k in d if k.startswith('tap_')), flush=True)

    import solvers
    net, kw, spec = ref_net('tiny_ncsnpp', SAMPLER_SEED)
    latents, _ = make_inputs(kw, 2, SAMPLER_SEED + 100)
    d = dict(config='tiny_ncsnpp', seed=SAMPLER_SEED, latents=latents.numpy())
    d['dpmpp2m'] = solvers.dpm_pp_sampler(net, latents, num_steps=6, sigma_min=0.002, sigma_max=80., schedule_type='logsnr', schedule_rho=7,
                                          max_order=2, predict_x0=True, lower_order_final=True, return_inters=True).numpy()
    d['heun'] = solvers.heun_sampler(net, latents, num_steps=4, sigma_min=0.002, sigma_max=80., schedule_type='polynomial', schedule_rho=7,
                                     return_inters=True).numpy()
    np.savez_compressed(os.path.join(OUT, 'ncsnpp_sampler_tiny.npz'), **d)
    print('sampler', d['dpmpp2m'].shape, d['heun'].shape, float(np.abs(d['dpmpp2m'][-1]).max()), float(np.abs(d['heun'][-1]).max()))


if __name__ == '__main__':
    main()
