"""Architecture of the Consistency-Models pixel-space nets the reference wraps in ``CMPrecond`` (diff-solvers-main/sample.py:86-91,
models/cm/unet.py ``UNetModel``, models/cm/cm_model_loader.py): ``lsun_bedroom`` and ``lsun_cat``.

With ``resblock_updown=True`` the CM ``UNetModel`` is, layer for layer, the ADM block list ``arch.dhariwal_unet_spec`` describes:

    ResBlock            GroupNorm(32) -> SiLU -> [avg-pool /2 | nearest x2] -> 3x3;  SiLU -> Linear embedding, added (or scale / shift with
                        ``use_scale_shift_norm``);  GroupNorm -> SiLU -> 3x3;  1x1 skip where the channel count changes
    AttentionBlock      GroupNorm -> 1x1 qkv -> softmax(q k^T / sqrt(d)) v per 64-channel head -> 1x1, residual
    time_embed          [cos | sin] timestep embedding (no endpoint) -> Linear -> SiLU -> Linear (every block applies the second SiLU itself)
    middle_block        the spec's two ``dec.RxR_in*`` blocks; an ``output_blocks`` entry's trailing up-ResBlock is the spec's ``dec.RxR_up``

so the engine needs no new block: ``cm_unet_spec`` returns that ``UNetSpec`` (``skip_scale = 1``, ``eps = 1e-5``, no sin / cos swap, and
``cm_noise``: the embedding of ``1000 * ln(sigma) / 4``), and this file holds the parameter table under the reference's own state-dict
names with the mapping onto the names ``UNetEngine._pack`` reads.  What the engine would not evaluate as the reference does is refused with
NotImplementedError -- never approximated.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import torch

from . import arch

# models/cm/cm_model_loader.py lsun_setting(): LSUN-Bedroom and LSUN-Cat share it (load_cm_model picks it for every non-ImageNet path)
_LSUN = dict(image_size=256, num_channels=256, num_res_blocks=2, num_heads=4, num_heads_upsample=-1, num_head_channels=64,
             attention_resolutions='32,16,8', channel_mult='', dropout=0.1, class_cond=False, use_checkpoint=False,
             use_scale_shift_norm=False, resblock_updown=True, use_fp16=True, use_new_attention_order=False, learn_sigma=False)

NAMED_CM_CONFIGS: Dict[str, dict] = {
    'lsun_bedroom': dict(_LSUN),
    'lsun_cat': dict(_LSUN),
    # reduced nets of the parity tests.  tiny_cm: scale / shift blocks, attention in every block of the 16-pixel level;
    # tiny_cm_wide: the LSUN block form (embedding added) with a level above 64 pixels, so that the wide fp16 block convolutions run
    'tiny_cm': dict(image_size=32, num_channels=128, num_res_blocks=1, channel_mult='1,2', attention_resolutions='16', num_heads=4,
                    num_head_channels=64, use_scale_shift_norm=True, resblock_updown=True, use_fp16=False),
    'tiny_cm_wide': dict(image_size=128, num_channels=128, num_res_blocks=1, channel_mult='1,1,2', attention_resolutions='32', num_heads=4,
                         num_head_channels=64, use_scale_shift_norm=False, resblock_updown=True, use_fp16=False),
}

_DEFAULT_MULT = {512: (0.5, 1, 1, 2, 2, 4, 4), 256: (1, 1, 2, 2, 4, 4), 128: (1, 1, 2, 3, 4), 64: (1, 2, 3, 4)}


def cm_unet_spec(image_size, num_channels, num_res_blocks, channel_mult='', learn_sigma=False, class_cond=False, use_checkpoint=False,
                 attention_resolutions='16', num_heads=1, num_head_channels=-1, num_heads_upsample=-1, use_scale_shift_norm=False, dropout=0,
                 resblock_updown=False, use_fp16=False, use_new_attention_order=False, sigma_min=0.002, sigma_max=80.0,
                 sigma_data=0.5) -> arch.UNetSpec:
    """Keyword-compatible with ``models/cm/cm_model_loader.create_model``; the last three are ``CMPrecond``'s."""
    if not resblock_updown:
        raise NotImplementedError('CM UNetModel with resblock_updown=False (Downsample / Upsample with a learned 3x3) is not supported')
    if num_head_channels == -1:
        raise NotImplementedError('CM UNetModel with num_head_channels=-1 (a fixed head count) is not supported: the engine\'s attention '
                                  'blocks have 64-channel heads')
    if num_head_channels != 64:
        raise NotImplementedError(f'CM UNetModel with num_head_channels={num_head_channels}: the engine\'s attention blocks have 64-channel heads')
    if use_new_attention_order:
        raise NotImplementedError('CM UNetModel with use_new_attention_order=True is not supported')
    if class_cond:
        raise NotImplementedError('class-conditional CM nets (label_emb) are not supported')
    if learn_sigma:
        raise NotImplementedError('CM UNetModel with learn_sigma=True (six output channels) is not supported')
    if channel_mult == '':
        if image_size not in _DEFAULT_MULT:
            raise ValueError(f'unsupported image size: {image_size}')
        mult = _DEFAULT_MULT[image_size]
    else:
        mult = tuple(int(m) for m in channel_mult.split(',')) if isinstance(channel_mult, str) else tuple(channel_mult)
    if any(int(m) != m for m in mult):
        raise NotImplementedError(f'fractional channel_mult {mult} is not supported')
    attn = tuple(int(r) for r in attention_resolutions.split(',')) if isinstance(attention_resolutions, str) else tuple(attention_resolutions)
    spec = arch.dhariwal_unet_spec(img_resolution=image_size, in_channels=3, out_channels=3, label_dim=0, augment_dim=0,
                                   model_channels=num_channels, channel_mult=tuple(int(m) for m in mult), channel_mult_emb=4,
                                   num_blocks=num_res_blocks, attn_resolutions=attn, dropout=dropout)
    for b in spec.blocks:
        if b.kind != 'block':
            continue
        b.adaptive_scale = bool(use_scale_shift_norm)
        b.skip_scale, b.eps = 1.0, 1e-5
        for c in (b.cin, b.cout):
            # the reference normalises with GroupNorm(32, c) (models/cm/nn.py normalization); the engine's rule is min(32, c // 4) groups
            if c % 32 or arch.num_groups(c) != 32:
                raise NotImplementedError(f'{b.name}: GroupNorm(32) on {c} channels differs from the engine\'s group rule')
        if b.heads and b.cout % 64:
            raise NotImplementedError(f'{b.name}: {b.cout} channels are not whole 64-channel heads')
    spec.cm_noise = True
    spec.sigma_min, spec.sigma_max, spec.sigma_data, spec.use_fp16 = float(sigma_min), float(sigma_max), float(sigma_data), bool(use_fp16)
    return spec


def cm_precond_spec(name_or_kwargs) -> arch.UNetSpec:
    kw = NAMED_CM_CONFIGS[name_or_kwargs] if isinstance(name_or_kwargs, str) else name_or_kwargs
    return cm_unet_spec(**kw)


# ------------------------------------------------------------------------------------------------
# Parameter table under the reference's names

_RES_LEAVES = (('in_layers.0', 'norm0'), ('in_layers.2', 'conv0'), ('emb_layers.1', 'affine'), ('out_layers.0', 'norm1'),
               ('out_layers.3', 'conv1'), ('skip_connection', 'skip'))
_ATTN_LEAVES = (('norm', 'norm2'), ('qkv', 'qkv'), ('proj_out', 'proj'))


def module_prefixes(spec: arch.UNetSpec) -> List[Tuple[str, str, bool]]:
    """(reference module prefix, engine key prefix, is an AttentionBlock) of every parameterised module, in the reference's state-dict order."""
    m = 'model'
    out = [('time_embed.0', f'{m}.map_layer0', False), ('time_embed.2', f'{m}.map_layer1', False)]
    n_in = 0
    mid = [b for b in spec.blocks if '_in' in b.name.rsplit('x', 1)[-1] and b.name.startswith('dec.')]
    n_out, pos = -1, 0
    for b in spec.blocks:
        e = f'{m}.{b.name}'
        if b.name.startswith('enc.'):
            if b.kind == 'conv':
                out.append(('input_blocks.0.0', e, False))
                continue
            n_in += 1
            out.append((f'input_blocks.{n_in}.0', e, False))
            if b.heads:
                out.append((f'input_blocks.{n_in}.1', e, True))
        elif b in mid:
            if b is mid[0]:
                out.append(('middle_block.0', e, False))
                out.append(('middle_block.1', e, True))
            else:
                out.append(('middle_block.2', e, False))
        elif b.up:                       # the trailing up-ResBlock of the output_blocks entry before it
            out.append((f'output_blocks.{n_out}.{pos}', e, False))
        else:
            n_out, pos = n_out + 1, 1
            out.append((f'output_blocks.{n_out}.0', e, False))
            if b.heads:
                out.append((f'output_blocks.{n_out}.1', e, True))
                pos = 2
    assert len(mid) == 2 and mid[0].heads and not mid[1].heads
    out.append(('out.0', f'{m}.{spec.out_norm}', False))
    out.append(('out.2', f'{m}.{spec.out_conv}', False))
    return out


def cm_param_table(spec: arch.UNetSpec) -> List[Tuple[str, Tuple[int, ...], str]]:
    """(reference state-dict key, its shape, the engine's key) of every tensor of ``UNetModel``, in state-dict order.  The shapes are those of
    ``arch.param_table``: the attention 1x1s are 2-D convolutions in both (``AttentionBlock(dims=2)``)."""
    shapes = {k: s for k, s, _ in arch.param_table(spec)}
    rows = []
    for ref, eng, attn in module_prefixes(spec):
        leaves = _ATTN_LEAVES if attn else (_RES_LEAVES if f'{eng}.norm0.weight' in shapes else (('', ''),))
        for rl, el in leaves:
            rp, ep = (f'{ref}.{rl}', f'{eng}.{el}') if rl else (ref, eng)
            for leaf in ('weight', 'bias'):
                if f'{ep}.{leaf}' not in shapes:
                    assert el == 'skip', (ep, leaf)
                    continue
                s = shapes[f'{ep}.{leaf}']
                rows.append((f'{rp}.{leaf}', tuple(s), f'{ep}.{leaf}'))
    assert len(rows) == len(shapes) and len({r[2] for r in rows}) == len(rows)
    return rows


def qkv_to_engine(t: torch.Tensor, heads: int) -> torch.Tensor:
    """Rows of a ``qkv`` weight / bias from QKVFlashAttention's order (three, head, d) (models/cm/unet.py:366) to the (head, d, three) order
    of EDM's attention (networks_edm.py:174), which ``UNetEngine._pack`` unpacks."""
    d = t.shape[0] // (3 * heads)
    return t.reshape(3, heads, d, *t.shape[1:]).permute(1, 2, 0, *range(3, t.dim() + 2)).reshape(t.shape).contiguous()


def qkv_to_reference(t: torch.Tensor, heads: int) -> torch.Tensor:
    d = t.shape[0] // (3 * heads)
    return t.reshape(heads, d, 3, *t.shape[1:]).permute(2, 0, 1, *range(3, t.dim() + 2)).reshape(t.shape).contiguous()


def _heads_of(spec):
    return {f'model.{b.name}.qkv': b.heads for b in spec.blocks if b.heads}


def engine_params(spec: arch.UNetSpec, state_dict: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """A reference ``UNetModel`` state dict (fp32 or fp16 tensors) under the names and layouts ``UNetEngine._pack`` reads.  Entries with no
    place in the spec, missing entries and shape mismatches are errors."""
    table = cm_param_table(spec)
    known = {r[0] for r in table}
    extra = sorted(k for k in state_dict if k not in known)
    if extra:
        raise NotImplementedError(f'{len(extra)} state-dict entries have no place in the spec: {extra[:4]} ...')
    missing = [r[0] for r in table if r[0] not in state_dict]
    if missing:
        raise KeyError(f'{len(missing)} tensors of the spec are missing from the state dict: {missing[:4]} ...')
    shapes = {k: s for k, s, _ in arch.param_table(spec)}
    heads = _heads_of(spec)
    out = {}
    for rk, rs, ek in table:
        t = state_dict[rk].detach().to(torch.float32)
        if tuple(t.shape) != rs:
            raise ValueError(f'{rk}: shape {tuple(t.shape)}, the spec has {rs}')
        if ek.rsplit('.', 1)[0] in heads:
            t = qkv_to_engine(t, heads[ek.rsplit('.', 1)[0]])
        out[ek] = t.reshape(shapes[ek]).contiguous()
    return out


def reference_state_dict(spec: arch.UNetSpec, params: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The inverse of ``engine_params``: engine-keyed tensors as a ``UNetModel`` state dict (tools/gen_cm_golden.py loads it into the reference)."""
    heads = _heads_of(spec)
    out = {}
    for rk, rs, ek in cm_param_table(spec):
        t = params[ek].detach().to(torch.float32)
        if ek.rsplit('.', 1)[0] in heads:
            t = qkv_to_reference(t, heads[ek.rsplit('.', 1)[0]])
        out[rk] = t.reshape(rs).contiguous()
    return out


def middle_block_name(spec: arch.UNetSpec) -> str:
    """The spec block whose output is the output of the reference's ``middle_block`` (the AMED tap of a CM net)."""
    return [b.name for b in spec.blocks if b.name.startswith('dec.') and b.name.endswith('_in1')][0]
