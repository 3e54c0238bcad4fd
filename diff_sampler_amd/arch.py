"""Denoiser architecture descriptions (EDM SongUNet / DhariwalUNet).

The reference builds its U-Nets imperatively inside ``torch.nn.Module``
constructors (diff-solvers-main/models/networks_edm.py:221-310 SongUNet,
:364-425 DhariwalUNet, :126-156 UNetBlock).  The HIP engine does not run
modules; it runs a flat plan.  This file is the data model the plan is compiled
from: a ``UNetSpec`` listing every layer with its channel counts, resolution,
resampling, attention heads and the *reference state_dict key prefix* its
weights live under, so that a pickled EDM network (or a random-init one with the
same key names) can be bound by name.

Described: both SongUNet families of the published EDM checkpoints -- DDPM++ (``embedding_type='positional'``,
``encoder_type='standard'``, ``resample_filter=[1,1]``, ``channel_mult_noise=1``) and NCSN++ (``'fourier'``,
``'residual'``, ``[1,3,3,1]``, ``channel_mult_noise=2``), the four options independently of each other -- and ADM.
``encoder_type='skip'``, ``decoder_type='skip'`` and other filters raise NotImplementedError (no EDM checkpoint uses them).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Tuple

import torch


@dataclass
class BlockSpec:
    name: str                 # e.g. 'enc.16x16_block0'
    kind: str                 # 'conv' (plain 3x3 stem) | 'block' (UNetBlock) | 'aux' (enc.RxR_aux_residual: cin = caux, right after enc.RxR_down)
    cin: int
    cout: int
    res_in: int               # spatial size of the block input
    res_out: int              # spatial size of the block output
    up: bool = False
    down: bool = False
    heads: int = 0            # 0 = no attention
    skip_conv: bool = False   # 1x1 projection on the skip path
    adaptive_scale: bool = False
    skip_scale: float = 1.0
    eps: float = 1e-5
    pops_skip: bool = False   # decoder block that concatenates an encoder skip
    skip_cin: int = 0         # channels of the popped skip tensor (cin = x.C + skip_cin)
    pushes_skip: bool = False  # encoder layer whose output is pushed on the skip stack


@dataclass
class UNetSpec:
    model_type: str                     # 'SongUNet' | 'DhariwalUNet'
    img_resolution: int
    in_channels: int
    out_channels: int
    label_dim: int
    augment_dim: int
    model_channels: int
    emb_channels: int
    noise_channels: int
    pos_endpoint: bool                  # PositionalEmbedding(endpoint=...)
    pos_max_positions: int
    swap_sincos: bool                   # SongUNet flips [cos|sin] -> [sin|cos] (networks_edm.py:315)
    out_norm: str                       # key of the output GroupNorm, relative to 'model.'
    out_conv: str                       # key of the output conv
    out_eps: float
    blocks: List[BlockSpec] = field(default_factory=list)
    # EDMPrecond (networks_edm.py:460-480)
    sigma_data: float = 0.5
    sigma_min: float = 0.002
    sigma_max: float = 80.0
    use_fp16: bool = False
    # SongUNet variants (networks_edm.py:237-241)
    embedding_type: str = 'positional'  # 'positional' | 'fourier' (FourierEmbedding: a `map_noise.freqs` buffer in the state dict)
    encoder_type: str = 'standard'      # 'standard' | 'residual' ('aux' entries in `blocks`)
    resample_filter: Tuple[int, ...] = (1, 1)      # (1, 1) | (1, 3, 3, 1): the 1-D taps of every up / down block (and of the aux layers)
    # SFD's distilled, step-conditioned nets (sfd-main/models/networks_edm.py:290-292, :438-440, :153): a second embedding path `map_step*` and an
    # `affine_step` Linear in every block.  False: the key list and the parameters of the spec are those of a plain EDM net.
    step_condition: bool = False
    # The consistency-model nets behind CMPrecond (cm_arch.py; networks_edm.py:540-541): the embedding takes 1000 * c_noise, and its frequencies
    # are rounded as models/cm/nn.py timestep_embedding rounds them.
    cm_noise: bool = False

    @property
    def ncsnpp(self) -> bool:
        """Does the network use any NCSN++ option (plans with launches outside libdsamd; fp32 only)?"""
        return self.embedding_type != 'positional' or self.encoder_type != 'standard' or tuple(self.resample_filter) != (1, 1)

    @property
    def enc(self) -> List[BlockSpec]:
        return [b for b in self.blocks if b.name.startswith('enc.')]

    @property
    def dec(self) -> List[BlockSpec]:
        return [b for b in self.blocks if b.name.startswith('dec.')]


def song_unet_spec(
    img_resolution, in_channels, out_channels, label_dim=0, augment_dim=0,
    model_channels=128, channel_mult=(1, 2, 2, 2), channel_mult_emb=4, num_blocks=4,
    attn_resolutions=(16,), dropout=0.10, label_dropout=0, embedding_type='positional',
    channel_mult_noise=1, encoder_type='standard', decoder_type='standard',
    resample_filter=(1, 1), step_condition=False,
) -> UNetSpec:
    """DDPM++ / NCSN++ layer list; mirrors the construction order of networks_edm.py:260-310."""
    if embedding_type not in ('positional', 'fourier'):
        raise ValueError(f'unknown embedding_type {embedding_type!r}')
    if encoder_type not in ('standard', 'residual') or decoder_type != 'standard':
        raise NotImplementedError(f'SongUNet encoder_type={encoder_type!r} / decoder_type={decoder_type!r}: only the standard and the residual '
                                  f'encoder and the standard decoder are supported (no EDM checkpoint uses the skip variants)')
    resample_filter = tuple(int(v) for v in resample_filter)
    if resample_filter not in ((1, 1), (1, 3, 3, 1)):
        raise NotImplementedError(f'SongUNet resample_filter={list(resample_filter)}: only [1,1] and [1,3,3,1] are supported')
    emb_channels = model_channels * channel_mult_emb
    noise_channels = model_channels * channel_mult_noise
    spec = UNetSpec(
        model_type='SongUNet', img_resolution=img_resolution, in_channels=in_channels, out_channels=out_channels,
        label_dim=label_dim, augment_dim=augment_dim, model_channels=model_channels, emb_channels=emb_channels,
        noise_channels=noise_channels, pos_endpoint=True, pos_max_positions=10000, swap_sincos=True,
        out_norm=f'dec.{img_resolution}x{img_resolution}_aux_norm', out_conv=f'dec.{img_resolution}x{img_resolution}_aux_conv',
        out_eps=1e-6, embedding_type=embedding_type, encoder_type=encoder_type, resample_filter=resample_filter,
        step_condition=bool(step_condition),
    )
    common = dict(skip_scale=math.sqrt(0.5), eps=1e-6, adaptive_scale=False)
    cout = caux = in_channels
    skips: List[int] = []
    for level, mult in enumerate(channel_mult):
        res = img_resolution >> level
        if level == 0:
            cin, cout = cout, model_channels
            spec.blocks.append(BlockSpec(f'enc.{res}x{res}_conv', 'conv', cin, cout, res, res, pushes_skip=True))
        else:
            spec.blocks.append(BlockSpec(f'enc.{res}x{res}_down', 'block', cout, cout, res * 2, res, down=True,
                                         skip_conv=True, pushes_skip=True, **common))
            if encoder_type == 'residual':
                # x = skips[-1] = aux = (x + aux_residual(aux)) / sqrt(2)  (networks_edm.py:283, :335): replaces the down block's skip entry
                spec.blocks.append(BlockSpec(f'enc.{res}x{res}_aux_residual', 'aux', caux, cout, res * 2, res, down=True,
                                             skip_scale=math.sqrt(0.5)))
                caux = cout
        skips.append(cout)
        for idx in range(num_blocks):
            cin, cout = cout, model_channels * mult
            heads = 1 if res in attn_resolutions else 0
            spec.blocks.append(BlockSpec(f'enc.{res}x{res}_block{idx}', 'block', cin, cout, res, res, heads=heads,
                                         skip_conv=(cin != cout), pushes_skip=True, **common))
            skips.append(cout)
    for level, mult in reversed(list(enumerate(channel_mult))):
        res = img_resolution >> level
        if level == len(channel_mult) - 1:
            spec.blocks.append(BlockSpec(f'dec.{res}x{res}_in0', 'block', cout, cout, res, res, heads=1, **common))
            spec.blocks.append(BlockSpec(f'dec.{res}x{res}_in1', 'block', cout, cout, res, res, **common))
        else:
            spec.blocks.append(BlockSpec(f'dec.{res}x{res}_up', 'block', cout, cout, res // 2, res, up=True,
                                         skip_conv=True, **common))
        for idx in range(num_blocks + 1):
            sc = skips.pop()
            cin, cout = cout + sc, model_channels * mult
            heads = 1 if (idx == num_blocks and res in attn_resolutions) else 0
            spec.blocks.append(BlockSpec(f'dec.{res}x{res}_block{idx}', 'block', cin, cout, res, res, heads=heads,
                                         skip_conv=(cin != cout), pops_skip=True, skip_cin=sc, **common))
    assert not skips
    return spec


def dhariwal_unet_spec(
    img_resolution, in_channels, out_channels, label_dim=0, augment_dim=0,
    model_channels=192, channel_mult=(1, 2, 3, 4), channel_mult_emb=4, num_blocks=3,
    attn_resolutions=(32, 16, 8), dropout=0.10, label_dropout=0, step_condition=False,
) -> UNetSpec:
    """ADM layer list; mirrors networks_edm.py:387-425."""
    emb_channels = model_channels * channel_mult_emb
    spec = UNetSpec(
        model_type='DhariwalUNet', img_resolution=img_resolution, in_channels=in_channels, out_channels=out_channels,
        label_dim=label_dim, augment_dim=augment_dim, model_channels=model_channels, emb_channels=emb_channels,
        noise_channels=model_channels, pos_endpoint=False, pos_max_positions=10000, swap_sincos=False,
        out_norm='out_norm', out_conv='out_conv', out_eps=1e-5, step_condition=bool(step_condition),
    )
    common = dict(skip_scale=1.0, eps=1e-5, adaptive_scale=True)

    def heads_of(c, attn):
        return c // 64 if attn else 0

    cout = in_channels
    skips: List[int] = []
    for level, mult in enumerate(channel_mult):
        res = img_resolution >> level
        if level == 0:
            cin, cout = cout, model_channels * mult
            spec.blocks.append(BlockSpec(f'enc.{res}x{res}_conv', 'conv', cin, cout, res, res, pushes_skip=True))
        else:
            spec.blocks.append(BlockSpec(f'enc.{res}x{res}_down', 'block', cout, cout, res * 2, res, down=True,
                                         pushes_skip=True, **common))
        skips.append(cout)
        for idx in range(num_blocks):
            cin, cout = cout, model_channels * mult
            spec.blocks.append(BlockSpec(f'enc.{res}x{res}_block{idx}', 'block', cin, cout, res, res,
                                         heads=heads_of(cout, res in attn_resolutions), skip_conv=(cin != cout),
                                         pushes_skip=True, **common))
            skips.append(cout)
    for level, mult in reversed(list(enumerate(channel_mult))):
        res = img_resolution >> level
        if level == len(channel_mult) - 1:
            spec.blocks.append(BlockSpec(f'dec.{res}x{res}_in0', 'block', cout, cout, res, res, heads=heads_of(cout, True), **common))
            spec.blocks.append(BlockSpec(f'dec.{res}x{res}_in1', 'block', cout, cout, res, res, **common))
        else:
            spec.blocks.append(BlockSpec(f'dec.{res}x{res}_up', 'block', cout, cout, res // 2, res, up=True, **common))
        for idx in range(num_blocks + 1):
            sc = skips.pop()
            cin, cout = cout + sc, model_channels * mult
            spec.blocks.append(BlockSpec(f'dec.{res}x{res}_block{idx}', 'block', cin, cout, res, res,
                                         heads=heads_of(cout, res in attn_resolutions), skip_conv=(cin != cout),
                                         pops_skip=True, skip_cin=sc, **common))
    assert not skips
    return spec


def edm_precond_spec(img_resolution, img_channels, label_dim=0, use_fp16=False, sigma_min=0.002, sigma_max=80.0,
                     sigma_data=0.5, model_type='DhariwalUNet', **model_kwargs) -> UNetSpec:
    """Keyword-compatible with the reference ``EDMPrecond.__init__`` (networks_edm.py:461-480)."""
    builder = {'SongUNet': song_unet_spec, 'DhariwalUNet': dhariwal_unet_spec}.get(model_type)
    if builder is None:
        raise ValueError(f'unknown model_type {model_type!r}')
    spec = builder(img_resolution=img_resolution, in_channels=img_channels, out_channels=img_channels,
                   label_dim=label_dim, **model_kwargs)
    spec.sigma_data, spec.sigma_min, spec.sigma_max, spec.use_fp16 = sigma_data, sigma_min, sigma_max, use_fp16
    return spec


# Named configurations.  Architecture kwargs are the ones the reference itself states
# (sfd-main/training/training_loop.py:62-76).
NAMED_CONFIGS: Dict[str, dict] = {
    'cifar10': dict(img_resolution=32, img_channels=3, label_dim=0, model_type='SongUNet', embedding_type='positional',
                    encoder_type='standard', decoder_type='standard', channel_mult_noise=1, resample_filter=[1, 1],
                    model_channels=128, channel_mult=[2, 2, 2], dropout=0.13, augment_dim=9),
    'ffhq': dict(img_resolution=64, img_channels=3, label_dim=0, model_type='SongUNet', embedding_type='positional',
                 encoder_type='standard', decoder_type='standard', channel_mult_noise=1, resample_filter=[1, 1],
                 model_channels=128, channel_mult=[1, 2, 2, 2], dropout=0.05, augment_dim=9),
    'afhqv2': dict(img_resolution=64, img_channels=3, label_dim=0, model_type='SongUNet', embedding_type='positional',
                   encoder_type='standard', decoder_type='standard', channel_mult_noise=1, resample_filter=[1, 1],
                   model_channels=128, channel_mult=[1, 2, 2, 2], dropout=0.05, augment_dim=9),
    'imagenet64': dict(img_resolution=64, img_channels=3, label_dim=1000, model_type='DhariwalUNet',
                       model_channels=192, channel_mult=[1, 2, 3, 4]),
    # NCSN++ ('-ve' checkpoints: edm-cifar10-32x32-{uncond,cond}-ve, edm-ffhq-64x64-uncond-ve, edm-afhqv2-64x64-uncond-ve).  These
    # hyper-parameters are quoted from memory of the published EDM training script, which is not in the reference tree: the
    # architecture options are the ones networks_edm.py:237-241 names for NCSN++, dropout and augment_dim are those of the DDPM++
    # entries above.  A real pickle does not depend on them: it goes through engine.spec_from_module.
    'cifar10_ve': dict(img_resolution=32, img_channels=3, label_dim=0, model_type='SongUNet', embedding_type='fourier',
                       encoder_type='residual', decoder_type='standard', channel_mult_noise=2, resample_filter=[1, 3, 3, 1],
                       model_channels=128, channel_mult=[2, 2, 2], dropout=0.13, augment_dim=9),
    'ffhq_ve': dict(img_resolution=64, img_channels=3, label_dim=0, model_type='SongUNet', embedding_type='fourier',
                    encoder_type='residual', decoder_type='standard', channel_mult_noise=2, resample_filter=[1, 3, 3, 1],
                    model_channels=128, channel_mult=[1, 2, 2, 2], dropout=0.05, augment_dim=9),
    'afhqv2_ve': dict(img_resolution=64, img_channels=3, label_dim=0, model_type='SongUNet', embedding_type='fourier',
                      encoder_type='residual', decoder_type='standard', channel_mult_noise=2, resample_filter=[1, 3, 3, 1],
                      model_channels=128, channel_mult=[1, 2, 2, 2], dropout=0.05, augment_dim=9),
    # Reduced nets used by the parity tests (same code paths, seconds on CPU).
    'tiny_song': dict(img_resolution=16, img_channels=3, label_dim=0, model_type='SongUNet', model_channels=32,
                      channel_mult=[1, 2], num_blocks=1, attn_resolutions=[8], augment_dim=9),
    'tiny_song_cond': dict(img_resolution=16, img_channels=3, label_dim=10, model_type='SongUNet', model_channels=32,
                           channel_mult=[1, 2], num_blocks=1, attn_resolutions=[8], augment_dim=0),
    # tiny nets with the '8x8_block2/3' encoder layers the AMED bottleneck tap needs (solvers_amed.py:16-17).
    'tiny_song_amed': dict(img_resolution=16, img_channels=3, label_dim=0, model_type='SongUNet', model_channels=32,
                           channel_mult=[1, 2], num_blocks=4, attn_resolutions=[8], augment_dim=9),
    'tiny_song_amed_cond': dict(img_resolution=16, img_channels=3, label_dim=10, model_type='SongUNet', model_channels=32,
                                channel_mult=[1, 2], num_blocks=4, attn_resolutions=[8], augment_dim=0),
    # reduced NCSN++ nets: three levels, so that the second aux layer -- whose input is the previous level's aux, not the image -- exists
    'tiny_ncsnpp': dict(img_resolution=32, img_channels=3, label_dim=0, model_type='SongUNet', embedding_type='fourier',
                        encoder_type='residual', channel_mult_noise=2, resample_filter=[1, 3, 3, 1], model_channels=32,
                        channel_mult=[1, 2, 2], num_blocks=1, attn_resolutions=[16], augment_dim=9),
    'tiny_ncsnpp_cond': dict(img_resolution=32, img_channels=3, label_dim=10, model_type='SongUNet', embedding_type='fourier',
                             encoder_type='residual', channel_mult_noise=2, resample_filter=[1, 3, 3, 1], model_channels=32,
                             channel_mult=[1, 2, 2], num_blocks=1, attn_resolutions=[16], augment_dim=0),
    'tiny_adm': dict(img_resolution=16, img_channels=3, label_dim=10, model_type='DhariwalUNet', model_channels=64,
                     channel_mult=[1, 2], num_blocks=1, attn_resolutions=[8]),
}


# ------------------------------------------------------------------------------------------------
# Parameter table: (state_dict key, shape, init rule).  Key names are the reference's.

def _linear(keys, prefix, fin, fout, bias=True):
    keys.append((f'{prefix}.weight', (fout, fin), ('linear', fin, fout)))
    if bias:
        keys.append((f'{prefix}.bias', (fout,), ('linear_bias', fin, fout)))


def _conv(keys, prefix, cin, cout, k):
    keys.append((f'{prefix}.weight', (cout, cin, k, k), ('conv', cin * k * k, cout * k * k)))
    keys.append((f'{prefix}.bias', (cout,), ('conv_bias', cin * k * k, cout * k * k)))


def _gn(keys, prefix, c):
    keys.append((f'{prefix}.weight', (c,), ('ones',)))
    keys.append((f'{prefix}.bias', (c,), ('zeros',)))


def param_table(spec: UNetSpec) -> List[Tuple[str, Tuple[int, ...], tuple]]:
    """Every learnable tensor of ``EDMPrecond(model=<spec>)`` in state_dict order."""
    keys: list = []
    m = 'model'
    if spec.model_type == 'SongUNet':
        if spec.embedding_type == 'fourier':       # a registered buffer of FourierEmbedding (networks_edm.py:207): first in the state dict
            keys.append((f'{m}.map_noise.freqs', (spec.noise_channels // 2,), ('fourier', 16.0)))
        if spec.label_dim:
            _linear(keys, f'{m}.map_label', spec.label_dim, spec.noise_channels)
        if spec.augment_dim:
            _linear(keys, f'{m}.map_augment', spec.augment_dim, spec.noise_channels, bias=False)
        _linear(keys, f'{m}.map_layer0', spec.noise_channels, spec.emb_channels)
        _linear(keys, f'{m}.map_layer1', spec.emb_channels, spec.emb_channels)
        if spec.step_condition:
            if spec.embedding_type == 'fourier':   # map_step is a FourierEmbedding of its own: a second random frequency buffer
                keys.append((f'{m}.map_step.freqs', (spec.noise_channels // 2,), ('fourier', 16.0)))
            _linear(keys, f'{m}.map_step_layer0', spec.noise_channels, spec.emb_channels)
            _linear(keys, f'{m}.map_step_layer1', spec.emb_channels, spec.emb_channels)
    else:
        if spec.augment_dim:
            _linear(keys, f'{m}.map_augment', spec.augment_dim, spec.model_channels, bias=False)
        _linear(keys, f'{m}.map_layer0', spec.model_channels, spec.emb_channels)
        _linear(keys, f'{m}.map_layer1', spec.emb_channels, spec.emb_channels)
        if spec.label_dim:
            _linear(keys, f'{m}.map_label', spec.label_dim, spec.emb_channels, bias=False)
        if spec.step_condition:
            _linear(keys, f'{m}.map_step_layer0', spec.model_channels, spec.emb_channels)
            _linear(keys, f'{m}.map_step_layer1', spec.emb_channels, spec.emb_channels)
    for b in spec.blocks:
        p = f'{m}.{b.name}'
        if b.kind in ('conv', 'aux'):
            _conv(keys, p, b.cin, b.cout, 3)
            continue
        _gn(keys, f'{p}.norm0', b.cin)
        _conv(keys, f'{p}.conv0', b.cin, b.cout, 3)
        _linear(keys, f'{p}.affine', spec.emb_channels, b.cout * (2 if b.adaptive_scale else 1))
        _gn(keys, f'{p}.norm1', b.cout)
        _conv(keys, f'{p}.conv1', b.cout, b.cout, 3)
        if spec.step_condition:
            _linear(keys, f'{p}.affine_step', spec.emb_channels, b.cout * (2 if b.adaptive_scale else 1))
        if b.skip_conv:
            _conv(keys, f'{p}.skip', b.cin, b.cout, 1)
        if b.heads:
            _gn(keys, f'{p}.norm2', b.cout)
            _conv(keys, f'{p}.qkv', b.cout, b.cout * 3, 1)
            _conv(keys, f'{p}.proj', b.cout, b.cout, 1)
    last = spec.blocks[-1].cout
    _gn(keys, f'{m}.{spec.out_norm}', last)
    _conv(keys, f'{m}.{spec.out_conv}', last, spec.out_channels, 3)
    return keys


def num_groups(c: int) -> int:
    """GroupNorm group count rule (networks_edm.py:89-91): min(32, C // 4)."""
    return min(32, c // 4)


def init_params(spec: UNetSpec, seed: int = 0, mode: str = 'signal') -> Dict[str, torch.Tensor]:
    """Deterministic CPU-generated weights keyed like the reference state_dict.

    mode='signal': every tensor carries signal (weights ~ N(0, 1/fan_in), biases ~ N(0, 0.1^2), GroupNorm
        gains 1 + N(0, 0.1^2)).  The reference initialisers zero conv1/proj/out_conv (init_zero,
        networks_edm.py:252,384), which would make parity vacuous, so tests and the
        benchmark use this mode.
    mode='reference': the distributions of the reference initialisers (xavier_uniform / kaiming_uniform with
        the init_weight multipliers) — same statistics, not the same random stream.
    The NCSN++ tensors (``map_noise.freqs`` ~ N(0, 16^2) in both modes, networks_edm.py:207; the ``aux_residual`` layers) are drawn from
    a generator of their own: every other tensor of a network keeps the bits it has without them.  So are the step-condition tensors
    (``map_step*``, every ``affine_step``) of a spec with ``step_condition``: the other tensors are those of the plain spec, bit for bit.  They
    follow the same rules as their noise-path twins (weights ~ N(0, 1/fan_in) in 'signal' mode: the step embedding moves the output by
    percents of its scale, tools/gen_sfd_golden.py asserts it).
    """
    g_main = torch.Generator(device='cpu').manual_seed(int(seed))
    g_ncsnpp = torch.Generator(device='cpu').manual_seed(int(seed) + 0x4e43534e)
    g_step = torch.Generator(device='cpu').manual_seed(int(seed) + 0x53544550)
    out: Dict[str, torch.Tensor] = {}
    song = spec.model_type == 'SongUNet'
    if mode not in ('signal', 'reference'):
        raise ValueError(mode)
    for key, shape, rule in param_table(spec):
        kind = rule[0]
        g = g_ncsnpp if (kind == 'fourier' or '_aux_residual.' in key) else g_main
        if '.map_step' in key or '.affine_step.' in key:
            g = g_step
        if kind == 'fourier':
            t = torch.randn(shape, generator=g) * rule[1]
        elif mode == 'signal':
            if kind in ('conv', 'linear'):
                t = torch.randn(shape, generator=g) * (1.0 / math.sqrt(rule[1]))
            elif kind in ('conv_bias', 'linear_bias', 'zeros'):
                t = torch.randn(shape, generator=g) * 0.1
            else:  # 'ones'
                t = 1.0 + torch.randn(shape, generator=g) * 0.1
        elif mode == 'reference':
            leaf = key.rsplit('.', 2)[-2]
            leaf = {'affine_step': 'affine', 'map_step_layer0': 'map_layer0', 'map_step_layer1': 'map_layer1'}.get(leaf, leaf)
            zero_init = leaf in ('conv1', 'proj') or key.startswith(f'model.{spec.out_conv}')
            if kind in ('conv', 'linear', 'conv_bias', 'linear_bias'):
                fin, fout = rule[1], rule[2]
                if song:
                    bound = math.sqrt(6.0 / (fin + fout))
                    mult = 1e-5 if zero_init else (math.sqrt(0.2) if leaf == 'qkv' else 1.0)
                    if kind.endswith('bias'):
                        mult = 0.0
                else:
                    bound = math.sqrt(3.0 / fin)
                    mult = 0.0 if zero_init else math.sqrt(1.0 / 3.0)
                    if leaf in ('map_label',):
                        bound, mult = 1.0, 1.0  # kaiming_normal * sqrt(label_dim): N(0,1)
                if leaf == 'map_label' and not song:
                    t = torch.randn(shape, generator=g)
                else:
                    t = (torch.rand(shape, generator=g) * 2 - 1) * bound * mult
            elif kind == 'ones':
                t = torch.ones(shape)
            else:
                t = torch.zeros(shape)
        else:
            raise ValueError(mode)
        out[key] = t.to(torch.float32).contiguous()
    return out


def flops_per_image(spec: UNetSpec) -> float:
    """Algorithmic FLOPs (2 x MAC) of one denoiser evaluation on one image: convs, 1x1s, attention, linears."""
    f = 0.0
    for b in spec.blocks:
        hw = b.res_out * b.res_out
        if b.kind == 'conv':
            f += 2.0 * hw * 9 * b.cin * b.cout
            continue
        if b.kind == 'aux':         # the fused down form: the 3x3 runs at (res_in + 2)^2 (conv2d(padding=2), networks_edm.py:71)
            f += 2.0 * (b.res_in + 2) ** 2 * 9 * b.cin * b.cout
            continue
        f += 2.0 * hw * 9 * b.cin * b.cout + 2.0 * hw * 9 * b.cout * b.cout
        f += 2.0 * spec.emb_channels * b.cout * (2 if b.adaptive_scale else 1)
        if b.skip_conv:
            f += 2.0 * hw * b.cin * b.cout
        if b.heads:
            f += 2.0 * hw * b.cout * 3 * b.cout + 2.0 * hw * b.cout * b.cout
            f += 2.0 * 2.0 * hw * hw * b.cout
    f += 2.0 * spec.img_resolution ** 2 * 9 * spec.blocks[-1].cout * spec.out_channels
    f += 2.0 * (spec.noise_channels * spec.emb_channels + spec.emb_channels ** 2)
    return f
