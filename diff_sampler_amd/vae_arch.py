"""Architecture description of the ``AutoencoderKL`` decoder behind Stable Diffusion v1.x (``first_stage_config`` of
``v1-inference.yaml``): what ``LatentDiffusion.decode_first_stage`` runs on a sampled latent.

The reference builds it imperatively (diff-solvers-main/models/ldm/models/autoencoder.py:285-332 ``AutoencoderKL``: ``post_quant_conv``
+ ``Decoder``; ldm/modules/diffusionmodules/model.py:462-568 ``Decoder``, :82-141 ``ResnetBlock`` with ``temb_ch = 0``, :150-202
``AttnBlock``, :42-57 ``Upsample``, :38-39 ``Normalize`` = GroupNorm(32, eps 1e-6); ddpm.py:714 ``z / scale_factor``).  As for the
U-Nets (``arch.py``, ``ldm_arch.py``) the HIP engine (``vae_engine.py``) runs a flat plan compiled from a data model: ``VAEDecoderSpec``
lists every layer with its channels, resolution and the *reference state_dict key* of its weights (relative to ``first_stage_model.``),
so a real SD checkpoint binds by name.

Supported: the decoder of ``v1-inference.yaml`` and reduced-width copies of it -- ``attn_resolutions = []`` (the mid block's vanilla
``AttnBlock`` only), ``resamp_with_conv``, no ``tanh_out``, no ``give_pre_end``.  Anything else raises NotImplementedError.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import torch


@dataclass
class VAELayer:
    kind: str                  # 'conv_in' | 'res' | 'attn' | 'up' | 'conv_out'
    key: str                   # state_dict prefix below first_stage_model., e.g. 'decoder.up.2.block.0'
    cin: int
    cout: int
    res_in: int
    res_out: int


@dataclass
class VAEDecoderSpec:
    ch: int
    ch_mult: Tuple[int, ...]
    num_res_blocks: int
    z_channels: int
    embed_dim: int
    out_ch: int
    scale_factor: float
    latent_resolution: int     # side of the latent the plans are built for (64 for SD 512 x 512)
    layers: List[VAELayer] = field(default_factory=list)

    @property
    def img_resolution(self):
        return self.latent_resolution * 2 ** (len(self.ch_mult) - 1)


def vae_decoder_spec(ch=128, out_ch=3, ch_mult=(1, 2, 4, 4), num_res_blocks=2, attn_resolutions=(), z_channels=4, embed_dim=4,
                     scale_factor=0.18215, latent_resolution=64, resamp_with_conv=True, give_pre_end=False, tanh_out=False,
                     use_linear_attn=False, attn_type='vanilla', first_stage='kl', dropout=0.0, **ignored) -> VAEDecoderSpec:
    """Layer list in the order of ``Decoder.forward`` (model.py:535-568).  ``ignored``: the encoder-side entries of ``ddconfig``
    (``double_z``, ``resolution``, ``in_channels``)."""
    if first_stage != 'kl':
        raise NotImplementedError('only the AutoencoderKL first stage is supported (no VQ first stages)')
    if tuple(attn_resolutions) or use_linear_attn or attn_type != 'vanilla':
        raise NotImplementedError('only attn_resolutions = [] with the vanilla mid-block attention is supported')
    if tanh_out or give_pre_end or not resamp_with_conv:
        raise NotImplementedError('tanh_out / give_pre_end / Upsample without convolution are not supported')
    if ch % 32 or any(ch * m % 32 for m in ch_mult):
        raise NotImplementedError('GroupNorm(32) needs channel counts that are multiples of 32')
    ch_mult = tuple(int(m) for m in ch_mult)
    spec = VAEDecoderSpec(ch, ch_mult, num_res_blocks, z_channels, embed_dim, out_ch, float(scale_factor), int(latent_resolution))
    L = spec.layers
    res = spec.latent_resolution
    block_in = ch * ch_mult[-1]
    L.append(VAELayer('conv_in', 'decoder.conv_in', z_channels, block_in, res, res))
    L.append(VAELayer('res', 'decoder.mid.block_1', block_in, block_in, res, res))
    L.append(VAELayer('attn', 'decoder.mid.attn_1', block_in, block_in, res, res))
    L.append(VAELayer('res', 'decoder.mid.block_2', block_in, block_in, res, res))
    for i_level in reversed(range(len(ch_mult))):
        block_out = ch * ch_mult[i_level]
        for i_block in range(num_res_blocks + 1):
            L.append(VAELayer('res', f'decoder.up.{i_level}.block.{i_block}', block_in, block_out, res, res))
            block_in = block_out
        if i_level != 0:
            L.append(VAELayer('up', f'decoder.up.{i_level}.upsample', block_in, block_in, res, res * 2))
            res *= 2
    L.append(VAELayer('conv_out', 'decoder.conv_out', block_in, out_ch, res, res))
    return spec


NAMED_VAE_CONFIGS = {
    # Stable Diffusion v1.x (models/ldm/configs/stable-diffusion/v1-inference.yaml:46-64)
    'sd15': dict(ch=128, out_ch=3, ch_mult=(1, 2, 4, 4), num_res_blocks=2, attn_resolutions=(), z_channels=4, embed_dim=4,
                 scale_factor=0.18215, latent_resolution=64),
    # the full-width net on a 16 x 16 latent (128 x 128 image): every level has its real channel counts
    'sd15_16': dict(ch=128, out_ch=3, ch_mult=(1, 2, 4, 4), num_res_blocks=2, attn_resolutions=(), z_channels=4, embed_dim=4,
                    scale_factor=0.18215, latent_resolution=16),
    # same topology at test size
    'tiny_vae': dict(ch=32, out_ch=3, ch_mult=(1, 2, 4, 4), num_res_blocks=2, attn_resolutions=(), z_channels=4, embed_dim=4,
                     scale_factor=0.18215, latent_resolution=8),
}


def _conv(keys, prefix, cin, cout, k):
    keys.append((f'{prefix}.weight', (cout, cin, k, k), ('w', cin * k * k)))
    keys.append((f'{prefix}.bias', (cout,), ('b',)))


def _norm(keys, prefix, c):
    keys.append((f'{prefix}.weight', (c,), ('g',)))
    keys.append((f'{prefix}.bias', (c,), ('b',)))


def vae_param_table(spec: VAEDecoderSpec):
    """Every learnable tensor the decode path reads, keyed like ``first_stage_model``'s state_dict."""
    keys: list = []
    _conv(keys, 'post_quant_conv', spec.embed_dim, spec.z_channels, 1)
    for l in spec.layers:
        p = l.key
        if l.kind == 'conv_in':
            _conv(keys, p, l.cin, l.cout, 3)
        elif l.kind == 'res':
            _norm(keys, f'{p}.norm1', l.cin)
            _conv(keys, f'{p}.conv1', l.cin, l.cout, 3)
            _norm(keys, f'{p}.norm2', l.cout)
            _conv(keys, f'{p}.conv2', l.cout, l.cout, 3)
            if l.cin != l.cout:
                _conv(keys, f'{p}.nin_shortcut', l.cin, l.cout, 1)
        elif l.kind == 'attn':
            _norm(keys, f'{p}.norm', l.cin)
            for n in ('q', 'k', 'v', 'proj_out'):
                _conv(keys, f'{p}.{n}', l.cin, l.cin, 1)
        elif l.kind == 'up':
            _conv(keys, f'{p}.conv', l.cin, l.cout, 3)
        elif l.kind == 'conv_out':
            _norm(keys, 'decoder.norm_out', l.cin)
            _conv(keys, p, l.cin, l.cout, 3)
    return keys


def init_vae_params(spec: VAEDecoderSpec, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Deterministic CPU-generated weights (the rule of ``ldm_arch.init_ldm_params``): weights ~ N(0, 1/fan_in), biases ~ N(0, 0.1^2),
    norm gains 1 + N(0, 0.1^2)."""
    g = torch.Generator(device='cpu').manual_seed(int(seed))
    out: Dict[str, torch.Tensor] = {}
    for key, shape, rule in vae_param_table(spec):
        if rule[0] == 'w':
            t = torch.randn(shape, generator=g) * (1.0 / math.sqrt(rule[1]))
        elif rule[0] == 'b':
            t = torch.randn(shape, generator=g) * 0.1
        else:
            t = 1.0 + torch.randn(shape, generator=g) * 0.1
        out[key] = t.to(torch.float32).contiguous()
    return out


FIRST_STAGE_PREFIX = 'first_stage_model.'


def vae_params_from_state_dict(spec: VAEDecoderSpec, state_dict) -> Dict[str, torch.Tensor]:
    """The decoder's tensors out of a checkpoint's state_dict: keys ``first_stage_model.decoder.*`` / ``first_stage_model.post_quant_conv.*``
    (a whole SD checkpoint) or the same keys without the prefix (an AutoencoderKL checkpoint).  Missing keys and wrong shapes raise; the
    encoder, ``quant_conv`` and the loss are ignored."""
    out: Dict[str, torch.Tensor] = {}
    for key, shape, _ in vae_param_table(spec):
        t = state_dict.get(FIRST_STAGE_PREFIX + key)
        if t is None:
            t = state_dict.get(key)
        if t is None:
            raise KeyError(f'checkpoint has no {FIRST_STAGE_PREFIX + key!r}')
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f'{key}: checkpoint shape {tuple(t.shape)}, the spec needs {tuple(shape)}')
        out[key] = t.detach().to(torch.float32).contiguous()
    return out


def split_first_stage(state_dict):
    """(tensors of the decode path keyed below ``first_stage_model.``, True) when the checkpoint carries them, else ({}, False)."""
    keep = {k[len(FIRST_STAGE_PREFIX):]: v for k, v in state_dict.items()
            if k.startswith(FIRST_STAGE_PREFIX + 'decoder.') or k.startswith(FIRST_STAGE_PREFIX + 'post_quant_conv.')}
    return keep, bool(keep)


def vae_layer_flops(spec: VAEDecoderSpec):
    """[(name, FLOPs per image)] of every matrix product of one decode (2 x MAC): convolutions, 1x1 projections, attention."""
    f = [('post_quant_conv', 2.0 * spec.latent_resolution ** 2 * spec.embed_dim * spec.z_channels)]
    for l in spec.layers:
        hw = float(l.res_out * l.res_out)
        if l.kind in ('conv_in', 'up', 'conv_out'):
            f.append((l.key + ('.conv' if l.kind == 'up' else ''), 2.0 * hw * 9 * l.cin * l.cout))
        elif l.kind == 'res':
            f.append((l.key + '.conv1', 2.0 * hw * 9 * l.cin * l.cout))
            f.append((l.key + '.conv2', 2.0 * hw * 9 * l.cout * l.cout))
            if l.cin != l.cout:
                f.append((l.key + '.nin_shortcut', 2.0 * hw * l.cin * l.cout))
        elif l.kind == 'attn':
            f.append((l.key + '.qkv', 2.0 * hw * l.cin * l.cin * 3))
            f.append((l.key + '.attention', 4.0 * hw * hw * l.cin))
            f.append((l.key + '.proj_out', 2.0 * hw * l.cin * l.cin))
    return f


def vae_flops_per_image(spec: VAEDecoderSpec) -> float:
    return float(sum(v for _, v in vae_layer_flops(spec)))
