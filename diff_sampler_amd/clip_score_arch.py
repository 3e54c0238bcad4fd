"""Architecture description of the two-tower CLIP behind the reference's ``clip_score.py`` (the same file in diff-solvers-main, gits-main,
amed-solver-main and sfd-main: ``open_clip.create_model_and_transforms('ViT-g-14', pretrained='laion2b_s34b_b88k')``, lines 59-60).

    image tower   x = [class | conv_P(image)] + position            patches of P x P pixels, no bias; tokens = 1 + (size / P)^2
                  x = pre-LayerNorm(x)
                  L x   x += out_proj(attention(q, k, v of LayerNorm1(x)))      bidirectional, `heads` heads of width / heads
                        x += fc2(act(fc1(LayerNorm2(x))))
                  feature = visual_projection(post-LayerNorm(x[class row]))     -> [embed]
    text tower    x = token_embedding[ids] + position                           ids [B, 77]
                  L x   the same layer with the causal mask j <= i
                  feature = text_projection(final LayerNorm(x)[first argmax(ids)])   the end-of-text token has the largest id

``act`` is ``'gelu'`` (erf; the laion ViT-g-14) or ``'quick_gelu'`` (the OpenAI towers).  The parameter table carries the key names of
transformers' ``CLIPModel.state_dict()`` (tools/gen_clip_score_golden.py loads it into the real class with ``strict=True``);
``from_open_clip`` maps the layout the reference's checkpoint actually has (open_clip's ``CLIP`` module) onto it.  That converter is a pure
key-and-shape mapping and is TESTED AGAINST A SYNTHETIC DICT made by its inverse (``to_open_clip``), not against the ``open_clip``
package, which the tests cannot rely on being installed.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict

import torch

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


@dataclass
class ClipTowerSpec:
    width: int
    layers: int
    heads: int
    ffn: int

    @property
    def head_dim(self):
        return self.width // self.heads


@dataclass
class ClipScoreSpec:
    vision: ClipTowerSpec
    image_size: int
    patch: int
    text: ClipTowerSpec
    vocab: int
    positions: int
    embed: int
    act: str
    eps: float = 1e-5

    @property
    def grid(self):
        return self.image_size // self.patch

    @property
    def vision_tokens(self):
        return 1 + self.grid * self.grid

    @property
    def patch_k(self):
        return 3 * self.patch * self.patch


_G14 = dict(vision=dict(width=1408, layers=40, heads=16, ffn=6144), image_size=224, patch=14,
            text=dict(width=1024, layers=24, heads=16, ffn=4096), vocab=49408, positions=77, embed=1024, act='gelu')

NAMED_CLIP_SCORE_CONFIGS = {
    # open_clip 'ViT-g-14' (laion2b_s34b_b88k): what clip_score.py:59 loads
    'vit_g_14': _G14,
    # the same geometry with 2 + 2 layers (tests)
    'vit_g_14_2l': dict(_G14, vision=dict(_G14['vision'], layers=2), text=dict(_G14['text'], layers=2)),
    # test size: the image tower keeps head size 88 and 257 tokens, the text tower head size 64
    'tiny_clip_score': dict(vision=dict(width=352, layers=2, heads=4, ffn=1536), image_size=224, patch=14,
                            text=dict(width=128, layers=2, heads=2, ffn=512), vocab=512, positions=77, embed=64, act='gelu'),
}


def clip_score_spec(vision, text, image_size=224, patch=14, vocab=49408, positions=77, embed=1024, act='gelu', eps=1e-5) -> ClipScoreSpec:
    towers = []
    for t in (vision, text):
        t = ClipTowerSpec(int(t['width']), int(t['layers']), int(t['heads']), int(t['ffn']))
        if t.width % t.heads:
            raise ValueError('width must be a multiple of heads')
        if t.width % 32 or t.ffn % 32:
            raise NotImplementedError('the projection kernels need width and ffn to be multiples of 32')
        towers.append(t)
    if act not in ('gelu', 'quick_gelu'):
        raise ValueError(f"act must be 'gelu' (erf) or 'quick_gelu', got {act!r}")
    if image_size % patch:
        raise ValueError('image_size must be a multiple of patch')
    if positions != 77:
        raise NotImplementedError('the CLIP text towers have 77 positions')
    if embed % 4:
        raise NotImplementedError('embed must be a multiple of 4')
    return ClipScoreSpec(towers[0], int(image_size), int(patch), towers[1], int(vocab), int(positions), int(embed), act, float(eps))


def named_spec(name_or_kwargs) -> ClipScoreSpec:
    return clip_score_spec(**(NAMED_CLIP_SCORE_CONFIGS[name_or_kwargs] if isinstance(name_or_kwargs, str) else name_or_kwargs))


def _tower_keys(keys, prefix, t: ClipTowerSpec):
    W, F = t.width, t.ffn

    def lin(p, cin, cout):
        keys.append((f'{p}.weight', (cout, cin), ('w', cin)))
        keys.append((f'{p}.bias', (cout,), ('b',)))

    def norm(p):
        keys.append((f'{p}.weight', (W,), ('g',)))
        keys.append((f'{p}.bias', (W,), ('b',)))

    for i in range(t.layers):
        p = f'{prefix}.encoder.layers.{i}'
        for n in ('k_proj', 'v_proj', 'q_proj', 'out_proj'):
            lin(f'{p}.self_attn.{n}', W, W)
        norm(f'{p}.layer_norm1')
        lin(f'{p}.mlp.fc1', W, F)
        lin(f'{p}.mlp.fc2', F, W)
        norm(f'{p}.layer_norm2')
    return norm


def clip_score_param_table(spec: ClipScoreSpec):
    """[(key, shape, init rule)] of every tensor the scorer reads, keyed like ``transformers.CLIPModel.state_dict()`` (``logit_scale``,
    which the score does not use, is not listed; ``params_from_state_dict`` accepts and ignores it)."""
    V, T = spec.vision, spec.text
    keys = [('text_model.embeddings.token_embedding.weight', (spec.vocab, T.width), ('e',)),
            ('text_model.embeddings.position_embedding.weight', (spec.positions, T.width), ('e',))]
    norm = _tower_keys(keys, 'text_model', T)
    norm('text_model.final_layer_norm')
    keys += [('vision_model.embeddings.class_embedding', (V.width,), ('e',)),
             ('vision_model.embeddings.patch_embedding.weight', (V.width, 3, spec.patch, spec.patch), ('w', spec.patch_k)),
             ('vision_model.embeddings.position_embedding.weight', (spec.vision_tokens, V.width), ('e',))]
    norm = _tower_keys(keys, 'vision_model', V)
    norm('vision_model.pre_layrnorm')                     # (sic: the class's own spelling)
    norm('vision_model.post_layernorm')
    keys += [('visual_projection.weight', (spec.embed, V.width), ('w', V.width)),
             ('text_projection.weight', (spec.embed, T.width), ('w', T.width))]
    return keys


IGNORED_KEYS = ('logit_scale', 'text_model.embeddings.position_ids', 'vision_model.embeddings.position_ids')


def init_clip_score_params(spec: ClipScoreSpec, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Deterministic CPU-generated weights WITH SIGNAL, the rules of ``clip_arch.init_clip_params``: projection / MLP / patch weights
    ~ N(0, (1.5 / sqrt(fan_in))^2), biases ~ N(0, 0.1^2), embeddings ~ N(0, 0.5^2), norm gains 1 + N(0, 0.1^2)."""
    g = torch.Generator(device='cpu').manual_seed(int(seed))
    out: Dict[str, torch.Tensor] = {}
    for key, shape, rule in clip_score_param_table(spec):
        if rule[0] == 'w':
            t = torch.randn(shape, generator=g) * (1.5 / math.sqrt(rule[1]))
        elif rule[0] == 'b':
            t = torch.randn(shape, generator=g) * 0.1
        elif rule[0] == 'e':
            t = torch.randn(shape, generator=g) * 0.5
        else:
            t = 1.0 + torch.randn(shape, generator=g) * 0.1
        out[key] = t.to(torch.float32).contiguous()
    return out


def params_from_state_dict(spec: ClipScoreSpec, state_dict) -> Dict[str, torch.Tensor]:
    """Strict: the table's tensors out of a ``CLIPModel`` state_dict.  ``logit_scale`` and the ``position_ids`` buffers are accepted and
    ignored; any other missing or unexpected key, or a wrong shape, raises."""
    table = clip_score_param_table(spec)
    have = {k: v for k, v in state_dict.items() if k not in IGNORED_KEYS}
    want = {k for k, _, _ in table}
    missing, extra = sorted(want - set(have)), sorted(set(have) - want)
    if missing or extra:
        raise KeyError(f'CLIP state_dict: missing {missing[:4]}{"..." if len(missing) > 4 else ""}, '
                       f'unexpected {extra[:4]}{"..." if len(extra) > 4 else ""}')
    out: Dict[str, torch.Tensor] = {}
    for key, shape, _ in table:
        t = have[key]
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f'{key}: checkpoint shape {tuple(t.shape)}, the spec needs {tuple(shape)}')
        out[key] = t.detach().to(torch.float32).contiguous()
    return out


# ---- the open_clip layout ---------------------------------------------------------------------------------------------------------------
_BLOCK = (('ln_1', 'layer_norm1'), ('ln_2', 'layer_norm2'), ('attn.out_proj', 'self_attn.out_proj'), ('mlp.c_fc', 'mlp.fc1'),
          ('mlp.c_proj', 'mlp.fc2'))
OPEN_CLIP_IGNORED = ('logit_scale', 'attn_mask')


def _open_clip_pairs(spec: ClipScoreSpec):
    """[(open_clip key, ours, how)]: how = '' same tensor, 't' transposed, 'conv' / 'qkvw' / 'qkvb' handled by name."""
    pairs = [('visual.conv1.weight', 'vision_model.embeddings.patch_embedding.weight', ''),
             ('visual.class_embedding', 'vision_model.embeddings.class_embedding', ''),
             ('visual.positional_embedding', 'vision_model.embeddings.position_embedding.weight', ''),
             ('visual.proj', 'visual_projection.weight', 't'),
             ('token_embedding.weight', 'text_model.embeddings.token_embedding.weight', ''),
             ('positional_embedding', 'text_model.embeddings.position_embedding.weight', ''),
             ('text_projection', 'text_projection.weight', 't')]
    for oc, ours in (('visual.ln_pre', 'vision_model.pre_layrnorm'), ('visual.ln_post', 'vision_model.post_layernorm'),
                     ('ln_final', 'text_model.final_layer_norm')):
        pairs += [(f'{oc}.{x}', f'{ours}.{x}', '') for x in ('weight', 'bias')]
    for ocp, ourp, layers in (('visual.transformer', 'vision_model', spec.vision.layers), ('transformer', 'text_model', spec.text.layers)):
        for i in range(layers):
            a, b = f'{ocp}.resblocks.{i}', f'{ourp}.encoder.layers.{i}'
            for oc, ours in _BLOCK:
                pairs += [(f'{a}.{oc}.{x}', f'{b}.{ours}.{x}', '') for x in ('weight', 'bias')]
            pairs += [(f'{a}.attn.in_proj_weight', f'{b}.self_attn', 'qkvw'), (f'{a}.attn.in_proj_bias', f'{b}.self_attn', 'qkvb')]
    return pairs


def from_open_clip(spec: ClipScoreSpec, state_dict) -> Dict[str, torch.Tensor]:
    """The table's tensors out of an open_clip ``CLIP`` state_dict: ``attn.in_proj_weight`` [3 W, W] / ``in_proj_bias`` [3 W] split into
    q | k | v, ``visual.proj`` / ``text_projection`` (stored [width, embed], applied as ``x @ proj``) transposed, the other tensors renamed.
    Strict like ``params_from_state_dict``; ``logit_scale`` and an ``attn_mask`` buffer are ignored."""
    have = {k: v for k, v in state_dict.items() if k not in OPEN_CLIP_IGNORED}
    pairs = _open_clip_pairs(spec)
    want = {oc for oc, _, _ in pairs}
    missing, extra = sorted(want - set(have)), sorted(set(have) - want)
    if missing or extra:
        raise KeyError(f'open_clip state_dict: missing {missing[:4]}{"..." if len(missing) > 4 else ""}, '
                       f'unexpected {extra[:4]}{"..." if len(extra) > 4 else ""}')
    hf: Dict[str, torch.Tensor] = {}
    for oc, ours, how in pairs:
        t = have[oc]
        if how in ('qkvw', 'qkvb'):
            W = (spec.vision if ours.startswith('vision_model') else spec.text).width
            need = (3 * W, W) if how == 'qkvw' else (3 * W,)
            if tuple(t.shape) != need:
                raise ValueError(f'{oc}: checkpoint shape {tuple(t.shape)}, the spec needs {need}')
            for j, n in enumerate('qkv'):
                hf[f'{ours}.{n}_proj.{"weight" if how == "qkvw" else "bias"}'] = t[j * W:(j + 1) * W]
        else:
            hf[ours] = t.t() if how == 't' else t
    return params_from_state_dict(spec, hf)


def to_open_clip(spec: ClipScoreSpec, params) -> Dict[str, torch.Tensor]:
    """The inverse mapping (tests; exporting seed weights in the reference checkpoint's layout)."""
    out: Dict[str, torch.Tensor] = {}
    for oc, ours, how in _open_clip_pairs(spec):
        if how in ('qkvw', 'qkvb'):
            out[oc] = torch.cat([params[f'{ours}.{n}_proj.{"weight" if how == "qkvw" else "bias"}'] for n in 'qkv'], 0).contiguous()
        else:
            out[oc] = (params[ours].t() if how == 't' else params[ours]).contiguous()
    return out


VISION_HEAD_DIM = {1280: 80, 1408: 88, 1664: 104, 352: 88}


def is_open_clip(state_dict) -> bool:
    return 'visual.conv1.weight' in state_dict or 'visual.proj' in state_dict


def spec_from_state_dict(state_dict, act='gelu') -> ClipScoreSpec:
    """Geometry read off the shapes of a HF or open_clip state_dict.  Neither layout stores the head count or the activation: the head size
    is 64 except at the image-tower widths of VISION_HEAD_DIM (open_clip's model table: ViT-H 1280 / 80, ViT-g 1408 / 88, ViT-bigG 1664 / 104;
    352 / 88 is the test geometry)."""
    sd = state_dict
    if is_open_clip(sd):
        conv, vpos, tok = sd['visual.conv1.weight'], sd['visual.positional_embedding'], sd['token_embedding.weight']
        embed = sd['text_projection'].shape[1]
        vffn, tffn = sd['visual.transformer.resblocks.0.mlp.c_fc.weight'].shape[0], sd['transformer.resblocks.0.mlp.c_fc.weight'].shape[0]
        count = lambda p: 1 + max(int(k[len(p):].split('.')[0]) for k in sd if k.startswith(p))
        vl, tl = count('visual.transformer.resblocks.'), count('transformer.resblocks.')
    else:
        conv, vpos = sd['vision_model.embeddings.patch_embedding.weight'], sd['vision_model.embeddings.position_embedding.weight']
        tok, embed = sd['text_model.embeddings.token_embedding.weight'], sd['text_projection.weight'].shape[0]
        vffn, tffn = sd['vision_model.encoder.layers.0.mlp.fc1.weight'].shape[0], sd['text_model.encoder.layers.0.mlp.fc1.weight'].shape[0]
        count = lambda p: 1 + max(int(k[len(p):].split('.')[0]) for k in sd if k.startswith(p))
        vl, tl = count('vision_model.encoder.layers.'), count('text_model.encoder.layers.')
    vw, patch, tw = conv.shape[0], conv.shape[-1], tok.shape[1]
    g = int(round(math.sqrt(vpos.shape[0] - 1)))
    vheads = max(1, vw // VISION_HEAD_DIM.get(vw, 64))
    return clip_score_spec(vision=dict(width=vw, layers=vl, heads=vheads, ffn=vffn), image_size=g * patch, patch=patch,
                           text=dict(width=tw, layers=tl, heads=max(1, tw // 64), ffn=tffn), vocab=tok.shape[0], positions=77,
                           embed=embed, act=act)


def clip_score_flops(spec: ClipScoreSpec):
    """(per image, per prompt) algorithmic FLOPs (2 x MAC): projections + the full attention products."""
    def tower(t, S):
        return t.layers * (2.0 * S * (4 * t.width * t.width + 2 * t.width * t.ffn) + 4.0 * S * S * t.width)
    img = tower(spec.vision, spec.vision_tokens) + 2.0 * (spec.vision_tokens - 1) * spec.patch_k * spec.vision.width + 2.0 * spec.vision.width * spec.embed
    txt = tower(spec.text, spec.positions) + 2.0 * spec.text.width * spec.embed
    return img, txt
