"""Regenerate tests/golden/cm_*.npz / cm_keys.json by running the REFERENCE CMPrecond + models/cm UNetModel, and the reference samplers, on the CPU.

    python tools/gen_cm_golden.py --reference /path/to/diff-solvers-main

The reference classes (models/cm/cm_model_loader.py, models/networks_edm.py CMPrecond) and samplers (solvers.py) are imported at run time from
that directory; nothing of their text is copied here, and the fixtures hold inputs and recorded results only.  Weights are never stored: they are
``arch.init_params(spec, seed)`` (every tensor carries signal, the reference's zero-initialised layers included) renamed by
``cm_arch.reference_state_dict`` and loaded strictly.

``flash_attn`` is not needed: the script registers a stand-in ``flash_attn.flash_attention.FlashAttention`` of its own -- plain softmax attention
on ``(b, s, 3, h, d)`` with the scale 1 / sqrt(d) -- before the reference is imported.

Files (each below 1 MiB):
  cm_keys.json                state-dict keys and shapes of the real ``lsun_setting()`` module (built on the meta device) and of both tiny nets
  cm_net_<config>.npz         tiny_cm, tiny_cm_wide, B = 2: x, sigma = [80, 0.5], out_vec (CMPrecond, fp32), the timestep embedding at sigma in
                              {0.002, 0.5, 80} (emb_sigma, emb) with its frequency table as this host rounds it (emb_freqs), the output of ``middle_block`` (mid; tiny_cm_wide: its first 16 channels and
                              mid_mean, the mean over all channels -- the whole tensor is 2 MiB) and rel_vs_fp32_golden, the distance of an
                              evaluation with fp16-rounded body operands and stored tensors from out_vec
  cm_traj_<solver>.npz        tiny_cm_wide, one image: latents and the states after each of 3 steps of euler_sampler and of dpm_pp_sampler (2M)
"""
import argparse
import json
import math
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, ROOT)

NETS = [('tiny_cm', 2, 81), ('tiny_cm_wide', 2, 82)]
TRAJ_SEED = 83
EMB_SIGMAS = [0.002, 0.5, 80.0]


class FlashAttention(torch.nn.Module):
    """The stand-in: softmax(q k^T * scale) v on qkv [b, s, 3, h, d], fp32 arithmetic; returns (out [b, s, h, d], None)."""

    def __init__(self, softmax_scale=None, attention_dropout=0.0, device=None, dtype=None):
        super().__init__()
        self.softmax_scale = softmax_scale

    def forward(self, qkv, key_padding_mask=None, causal=False, cu_seqlens=None, max_s=None, need_weights=False):
        assert key_padding_mask is None and not causal
        q, k, v = qkv.unbind(2)                                   # each [b, s, h, d]
        scale = self.softmax_scale or q.shape[-1] ** -0.5
        w = torch.einsum('bqhd,bkhd->bhqk', q.float(), k.float()) * scale
        o = torch.einsum('bhqk,bkhd->bqhd', torch.softmax(w, dim=-1), v.float())
        return o.to(qkv.dtype), None


def register_flash_attn_stub():
    pkg, mod = types.ModuleType('flash_attn'), types.ModuleType('flash_attn.flash_attention')
    mod.FlashAttention = FlashAttention
    pkg.flash_attention = mod
    sys.modules['flash_attn'], sys.modules['flash_attn.flash_attention'] = pkg, mod


def ref_net(name, seed):
    import diff_sampler_amd.arch as arch
    import diff_sampler_amd.cm_arch as cm_arch
    from models.cm.cm_model_loader import create_model
    from models.networks_edm import CMPrecond
    kw = dict(cm_arch.NAMED_CM_CONFIGS[name])
    spec = cm_arch.cm_unet_spec(**kw)
    model = create_model(**kw)
    model.load_state_dict(cm_arch.reference_state_dict(spec, arch.init_params(spec, seed=seed)), strict=True)
    return CMPrecond(model).eval().requires_grad_(False), spec


def f16_hooks(model):
    """fp16 operands and stored tensors in the body, as convert_to_fp16 has them: inputs, weights and outputs of every convolution / Linear of
    input_blocks, middle_block and output_blocks are rounded to fp16; arithmetic stays fp32."""
    r = lambda t: t.to(torch.float16).to(torch.float32)
    hooks = []
    for part in (model.input_blocks, model.middle_block, model.output_blocks):
        for m in part.modules():
            if isinstance(m, (torch.nn.Conv2d, torch.nn.Conv1d, torch.nn.Linear)):
                m.weight.data = r(m.weight.data)
                hooks.append(m.register_forward_pre_hook(lambda mod, inp: tuple(r(t) for t in inp)))
                hooks.append(m.register_forward_hook(lambda mod, inp, out: r(out)))
    return hooks


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reference', required=True, help='directory of the reference project that holds models/cm, models/networks_edm.py and solvers.py')
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.reference))
    register_flash_attn_stub()
    torch.set_grad_enabled(False)
    import diff_sampler_amd.cm_arch as cm_arch
    from models.cm.cm_model_loader import create_model, lsun_setting
    from models.cm.nn import timestep_embedding

    keys = {}
    with torch.device('meta'):
        big = create_model(**lsun_setting())
    keys['lsun'] = [(k, list(v.shape)) for k, v in big.state_dict().items()]
    keys['lsun_setting'] = lsun_setting()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    for name, B, seed in NETS:
        net, spec = ref_net(name, seed)
        keys[name] = [(k, list(v.shape)) for k, v in net.model.state_dict().items()]
        g = torch.Generator().manual_seed(seed + 100)
        R = spec.img_resolution
        sig = torch.tensor([80.0, 0.5][:B])
        x = torch.randn(B, 3, R, R, generator=g) * 0.5 + torch.randn(B, 3, R, R, generator=g) * sig.reshape(-1, 1, 1, 1)
        mid = {}
        h = net.model.middle_block.register_forward_hook(lambda m, i, o: mid.__setitem__('v', o.detach().clone()))
        out = net(x, sig)
        h.remove()
        es = torch.tensor(EMB_SIGMAS)
        emb = timestep_embedding(1000 * (es.log() / 4), spec.model_channels)
        # the frequency table behind `emb`, as THIS host's torch.exp rounds it (a vectorised fp32 exp is not the same to the last bit on every
        # CPU: one of the 64 entries differs from the correctly rounded value here).  Recorded so that the embedding kernel can be checked
        # on the reference's own frequencies; proven to be the reference's by reproducing `emb` from it to the bit.
        half = spec.model_channels // 2
        freqs = torch.exp(-math.log(10000) * torch.arange(0, half, dtype=torch.float32) / half)
        args = (1000 * (es.log() / 4))[:, None].float() * freqs[None]
        assert torch.equal(torch.cat([torch.cos(args), torch.sin(args)], dim=-1), emb)
        hooks = f16_hooks(net.model)
        out16 = net(x, sig)
        for hk in hooks:
            hk.remove()
        d = dict(config=name, seed=seed, x=x.numpy(), sigma=sig.numpy(), out_vec=out.numpy(), emb_sigma=es.numpy(), emb=emb.numpy(), emb_freqs=freqs.numpy(),
                 mid_name=cm_arch.middle_block_name(spec), rel_vs_fp32_golden=rel(out16, out))
        m = mid['v']
        d['mid_mean'] = m.mean(dim=1).numpy()
        d['mid'] = (m if m.numel() * 4 < (600 << 10) else m[:, :16]).numpy()
        np.savez_compressed(os.path.join(OUT, f'cm_net_{name}.npz'), **d)
        print(name, float(out.abs().max()), tuple(m.shape), 'f16 ops vs fp32', d['rel_vs_fp32_golden'], len(keys[name]), flush=True)
    with open(os.path.join(OUT, 'cm_keys.json'), 'w') as fh:
        json.dump(keys, fh, separators=(',', ':'))

    import solvers
    net, spec = ref_net('tiny_cm_wide', TRAJ_SEED)
    latents = torch.randn(1, 3, spec.img_resolution, spec.img_resolution, generator=torch.Generator().manual_seed(TRAJ_SEED + 100))
    common = dict(num_steps=4, sigma_min=0.002, sigma_max=80., schedule_type='polynomial', schedule_rho=7, return_inters=True)
    for tag, tr in (('euler', solvers.euler_sampler(net, latents, **common)),
                    ('dpmpp2m', solvers.dpm_pp_sampler(net, latents, max_order=2, predict_x0=True, lower_order_final=True, **common))):
        tr = tr.numpy()
        assert tr.shape[0] == 4 and np.allclose(tr[0], (latents * 80.0).numpy(), rtol=1e-6)      # state 0 is latents * t_0: not stored
        np.savez_compressed(os.path.join(OUT, f'cm_traj_{tag}.npz'), config='tiny_cm_wide', seed=TRAJ_SEED, latents=latents.numpy(), steps=tr[1:])
        print('sampler', tag, tr.shape, float(np.abs(tr[-1]).max()), flush=True)


if __name__ == '__main__':
    main()
