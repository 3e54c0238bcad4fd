#!/usr/bin/env python
"""Record the AutoencoderKL-decoder goldens tests/golden/vae_*.npz from the REAL reference classes, on the CPU.

    python tools/gen_vae_golden.py --reference <checkout of the reference tree> [tiny] [sd15_16] [sd15]

The reference's ``Decoder`` (diff-solvers-main/models/ldm/modules/diffusionmodules/model.py:462-568) is imported from its own tree and
instantiated with the numbers of ``vae_arch.NAMED_VAE_CONFIGS``; ``post_quant_conv`` is the 1x1 ``torch.nn.Conv2d(embed_dim, z_channels)``
``AutoencoderKL.__init__`` makes (autoencoder.py:304) and the decode is ``decoder(post_quant_conv(z / scale_factor))``
(autoencoder.py:330-332, ddpm.py:714).  Weights: ``vae_arch.init_vae_params(spec, seed)`` loaded with ``strict=True``, so the key names
and shapes of our table are checked against the real modules here.  Nothing of the reference is copied: the goldens hold inputs, the
seed and recorded outputs only.

Every golden also records ``f16_dist``: the distance (max |a - b| / max |b|) from the fp32 output of the same real modules evaluated
with every convolution's weights, input and output rounded to fp16 (forward hooks) -- an emulation on the CPU of the autocast mode the
reference decodes in (sample.py:296-299).  The fp16 test of the engine takes its bound from it.

  vae_tiny.npz      reduced spec (ch 32), 8 x 8 latents, B = 3
  vae_sd15_16.npz   full-width spec, 16 x 16 latents -> 128 x 128, B = 2
  vae_sd15.npz      full-width spec, one 64 x 64 latent -> 512 x 512; a fixed subset of output rows is stored (``rows``)
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, ROOT)

CASES = {'tiny': ('tiny_vae', 61, 3, 'vae_tiny.npz'), 'sd15_16': ('sd15_16', 62, 2, 'vae_sd15_16.npz'), 'sd15': ('sd15', 63, 1, 'vae_sd15.npz')}
# rows of the 512 x 512 output kept in vae_sd15.npz: every eighth row plus both sides of some 4-row patch borders and the last row
SD15_ROWS = sorted(set(range(0, 512, 8)) | {3, 4, 63, 64, 127, 255, 256, 257, 511})


def _real_decoder(ref, spec):
    sys.path.insert(0, os.path.join(ref, 'diff-solvers-main'))
    if 'omegaconf' not in sys.modules:
        try:
            import omegaconf  # noqa: F401
        except ImportError:
            m, lc = types.ModuleType('omegaconf'), types.ModuleType('omegaconf.listconfig')
            lc.ListConfig = type('ListConfig', (list,), {})
            m.listconfig = lc
            sys.modules['omegaconf'], sys.modules['omegaconf.listconfig'] = m, lc
    from models.ldm.modules.diffusionmodules.model import Decoder
    dec = Decoder(ch=spec.ch, out_ch=spec.out_ch, ch_mult=spec.ch_mult, num_res_blocks=spec.num_res_blocks, attn_resolutions=[],
                  dropout=0.0, in_channels=3, resolution=spec.img_resolution, z_channels=spec.z_channels, double_z=True).eval()
    pq = torch.nn.Conv2d(spec.embed_dim, spec.z_channels, 1).eval()
    return dec, pq


def _load(dec, pq, params):
    dec.load_state_dict({k[len('decoder.'):]: v for k, v in params.items() if k.startswith('decoder.')}, strict=True)
    pq.load_state_dict({k[len('post_quant_conv.'):]: v for k, v in params.items() if k.startswith('post_quant_conv.')}, strict=True)


def _h(t):
    return t.to(torch.float16).to(torch.float32)


def _round_convs_to_f16(mods):
    for root in mods:
        for m in root.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.weight.data = _h(m.weight.data)
                m.bias.data = _h(m.bias.data)
                m.register_forward_pre_hook(lambda mod, inp: tuple(_h(t) for t in inp))
                m.register_forward_hook(lambda mod, inp, out: _h(out))


def make(ref, case):
    import diff_sampler_amd.vae_arch as va
    name, seed, B, fname = CASES[case]
    spec = va.vae_decoder_spec(**va.NAMED_VAE_CONFIGS[name])
    params = va.init_vae_params(spec, seed=seed)
    g = torch.Generator().manual_seed(seed + 1000)
    R = spec.latent_resolution
    z = torch.randn(B, spec.z_channels, R, R, generator=g) * spec.scale_factor * 4.0     # sampler outputs are scaled latents
    with torch.no_grad():
        dec, pq = _real_decoder(ref, spec)
        _load(dec, pq, params)
        out = dec(pq(z / spec.scale_factor))
        dec16, pq16 = _real_decoder(ref, spec)
        _load(dec16, pq16, params)
        _round_convs_to_f16([dec16, pq16])
        out16 = dec16(pq16(z / spec.scale_factor))
    dist = float((out16 - out).abs().max() / out.abs().max())
    d = dict(config=name, seed=seed, z=z.numpy(), f16_dist=np.float64(dist), out_absmax=np.float64(out.abs().max()))
    u8 = (out * 127.5 + 128).clip(0, 255).to(torch.uint8).permute(0, 2, 3, 1).numpy()
    if case == 'sd15':
        rows = np.array(SD15_ROWS)
        d.update(rows=rows, out=out.numpy()[:, :, rows, :], u8=u8[:, rows])
    else:
        d.update(out=out.numpy(), u8=u8)
    np.savez_compressed(os.path.join(OUT, fname), **d)
    print(fname, 'out', tuple(out.shape), 'absmax %.4f' % float(out.abs().max()), 'f16_dist %.3e' % dist,
          '%d bytes' % os.path.getsize(os.path.join(OUT, fname)))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', default=os.environ.get('DS_REFERENCE_ROOT'), help='checkout of the reference tree (holds diff-solvers-main/)')
    ap.add_argument('cases', nargs='*', default=list(CASES))
    a = ap.parse_args()
    if not a.reference:
        ap.error('--reference (or DS_REFERENCE_ROOT) is required')
    torch.manual_seed(0)
    for c in a.cases:
        make(a.reference, c)
