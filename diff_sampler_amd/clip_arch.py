"""Architecture description of the CLIP text encoder behind Stable Diffusion v1.x (``cond_stage_config`` of ``v1-inference.yaml``):
what ``LatentDiffusion.get_learned_conditioning`` runs on a prompt (diff-solvers-main/sample.py:281-289).

The reference wraps transformers' ``CLIPTextModel`` (diff-solvers-main/models/ldm/modules/encoders/modules.py:137-159
``FrozenCLIPEmbedder``: ``self.transformer(input_ids=tokens).last_hidden_state``).  The network is fixed:

    x = token_embedding[ids] + position_embedding                               ids [B, 77]
    12 x   x += out_proj(causal_attention(q, k, v of LayerNorm1(x)))            12 heads of 64, score scale 64^-0.5, mask j <= i only
           x += fc2(quick_gelu(fc1(LayerNorm2(x))))                             quick_gelu(h) = h * sigmoid(1.702 h)
    final LayerNorm                                                             -> [B, 77, 768] fp32

No ``attention_mask`` is passed, so padding positions are ordinary tokens; the pooled output is not used.  ``ClipTextSpec`` is the data
model ``clip_engine.ClipTextEncoder`` compiles its plan from; the parameter table carries the *checkpoint's* key names (relative to
``cond_stage_model.transformer.``), so a real SD ``.ckpt`` binds by name.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict

import torch


@dataclass
class ClipTextSpec:
    vocab: int
    width: int
    layers: int
    heads: int
    ffn: int
    positions: int
    eps: float = 1e-5

    @property
    def head_dim(self):
        return self.width // self.heads


NAMED_CLIP_CONFIGS = {
    # openai/clip-vit-large-patch14 text tower (modules.py:139: the version FrozenCLIPEmbedder names)
    'sd15': dict(vocab=49408, width=768, layers=12, heads=12, ffn=3072, positions=77),
    # same topology at test size (the head size stays 64: the causal attention kernel's)
    'tiny_clip': dict(vocab=512, width=128, layers=2, heads=2, ffn=512, positions=77),
}

CKPT_PREFIX = 'cond_stage_model.transformer.'


def clip_text_spec(vocab=49408, width=768, layers=12, heads=12, ffn=3072, positions=77, eps=1e-5) -> ClipTextSpec:
    if width % heads:
        raise ValueError('width must be a multiple of heads')
    if width % 32 or ffn % 32:
        raise NotImplementedError('the projection kernels need width and ffn to be multiples of 32')
    return ClipTextSpec(int(vocab), int(width), int(layers), int(heads), int(ffn), int(positions), float(eps))


def clip_param_table(spec: ClipTextSpec):
    """[(key, shape, init rule)] of every tensor the encoder reads, keyed like ``cond_stage_model.transformer``'s state_dict."""
    W, F = spec.width, spec.ffn
    keys = [('text_model.embeddings.token_embedding.weight', (spec.vocab, W), ('e',)),
            ('text_model.embeddings.position_embedding.weight', (spec.positions, W), ('e',))]

    def lin(p, cin, cout):
        keys.append((f'{p}.weight', (cout, cin), ('w', cin)))
        keys.append((f'{p}.bias', (cout,), ('b',)))

    def norm(p):
        keys.append((f'{p}.weight', (W,), ('g',)))
        keys.append((f'{p}.bias', (W,), ('b',)))

    for i in range(spec.layers):
        p = f'text_model.encoder.layers.{i}'
        for n in ('k_proj', 'v_proj', 'q_proj', 'out_proj'):
            lin(f'{p}.self_attn.{n}', W, W)
        norm(f'{p}.layer_norm1')
        lin(f'{p}.mlp.fc1', W, F)
        lin(f'{p}.mlp.fc2', F, W)
        norm(f'{p}.layer_norm2')
    norm('text_model.final_layer_norm')
    return keys


def init_clip_params(spec: ClipTextSpec, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Deterministic CPU-generated weights WITH SIGNAL: projection / MLP weights ~ N(0, (1.5 / sqrt(fan_in))^2), biases ~ N(0, 0.1^2),
    embeddings ~ N(0, 0.5^2), norm gains 1 + N(0, 0.1^2).  (With transformers' own 0.02 init every softmax is nearly uniform and neither the
    mask nor the activation would move the output.)"""
    g = torch.Generator(device='cpu').manual_seed(int(seed))
    out: Dict[str, torch.Tensor] = {}
    for key, shape, rule in clip_param_table(spec):
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


def clip_params_from_state_dict(spec: ClipTextSpec, state_dict, prefix=CKPT_PREFIX) -> Dict[str, torch.Tensor]:
    """The encoder's tensors out of a state_dict whose keys start with `prefix` (a whole SD checkpoint: ``cond_stage_model.transformer.``;
    '' for a bare ``CLIPTextModel`` state_dict).  ``embeddings.position_ids`` (a buffer older transformers versions saved) is ignored; any
    other missing or unexpected key below the prefix, or a wrong shape, raises."""
    table = clip_param_table(spec)
    below = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
    below.pop('text_model.embeddings.position_ids', None)
    want = {k for k, _, _ in table}
    missing, extra = sorted(want - set(below)), sorted(set(below) - want)
    if missing or extra:
        raise KeyError(f'text encoder state_dict (prefix {prefix!r}): missing {missing[:4]}{"..." if len(missing) > 4 else ""}, '
                       f'unexpected {extra[:4]}{"..." if len(extra) > 4 else ""}')
    out: Dict[str, torch.Tensor] = {}
    for key, shape, _ in table:
        t = below[key]
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f'{key}: checkpoint shape {tuple(t.shape)}, the spec needs {tuple(shape)}')
        out[key] = t.detach().to(torch.float32).contiguous()
    return out


def split_cond_stage(state_dict, prefix=CKPT_PREFIX):
    """The tensors of a checkpoint below `prefix`, keys unchanged ({} when it carries no text encoder)."""
    return {k: v for k, v in state_dict.items() if k.startswith(prefix)}


def clip_flops_per_prompt(spec: ClipTextSpec) -> float:
    """Algorithmic FLOPs (2 x MAC) of encoding one prompt: projections + the full (unmasked) attention products."""
    S, W, F = spec.positions, spec.width, spec.ffn
    per_layer = 2.0 * S * (4 * W * W + 2 * W * F) + 4.0 * S * S * W
    return spec.layers * per_layer
