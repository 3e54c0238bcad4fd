"""CLIP text encoder on the HIP engine: what the reference's batch loop runs before the sampler for a latent-diffusion model,
``c = net.model.get_learned_conditioning(prompts)`` / ``uc = net.model.get_learned_conditioning([""])`` (diff-solvers-main/sample.py:281-289;
ldm/modules/encoders/modules.py:137-159 ``FrozenCLIPEmbedder`` = transformers ``CLIPTextModel(input_ids).last_hidden_state``) -- token ids
[B, 77] -> states [B, 77, 768] (``clip_arch.ClipTextSpec`` is the data model; ``clip_tokenizer`` makes the ids).

One encode = one flat plan of libdsamd launches over token-major rows (B * 77 rows of `width` floats):

    embeddings          ds_token_embed: table gather + position add
    per layer           LayerNorm -> q | k | v as ONE projection (width -> 3 width) -> ds_attention_causal on the packed output in place
                        -> out_proj (+ residual) -> LayerNorm -> fc1 -> ds_quick_gelu (in place) -> fc2 (+ residual)
    final LayerNorm     into the plan's output buffer

fp32 IN EVERY MODE: the reference encodes its prompts before it enters ``autocast`` (sample.py:286-289 come before :296), so there is no
fp16 form of this network -- the projections are ``ds_conv2d_nhwc`` with taps = 1 on the exact-fp32 matrix pipe, whatever ``--use_fp16`` says.
"""
from __future__ import annotations

from typing import Dict

import torch

from . import _lib, clip_arch
from .ops import pack_linear_weight
from .plan import Builder, Plan, ptr


class ClipTextEncoder:
    """``ClipTextEncoder(tokens) -> [B, positions, width]`` fp32 for int token ids ``tokens`` [B, positions]."""

    def __init__(self, spec: clip_arch.ClipTextSpec, params: Dict[str, torch.Tensor], device='cuda', batch_invariant=False):
        """batch_invariant: every projection carries ds_conv_tune.invariant: same prompt, same bits at any batch (the
        other launches are batch-invariant by construction)."""
        self.spec = spec
        self.device = torch.device(device)
        self.batch_invariant = bool(batch_invariant)
        self.lib = _lib.load()
        self._plans: Dict[int, Plan] = {}
        self._pack(params)

    @classmethod
    def from_config(cls, name_or_kwargs='sd15', seed=0, device='cuda', **kw):
        cfg = clip_arch.NAMED_CLIP_CONFIGS[name_or_kwargs] if isinstance(name_or_kwargs, str) else name_or_kwargs
        spec = clip_arch.clip_text_spec(**cfg)
        return cls(spec, clip_arch.init_clip_params(spec, seed=seed), device, **kw)

    @classmethod
    def from_state_dict(cls, state_dict, prefix=clip_arch.CKPT_PREFIX, name_or_kwargs='sd15', device='cuda', **kw):
        """From a checkpoint's state_dict: the keys below `prefix` (``cond_stage_model.transformer.`` in an SD ``.ckpt``) are the
        ``text_model.*`` tensors of ``CLIPTextModel``; ``embeddings.position_ids`` is ignored, any other missing or unexpected key raises."""
        cfg = clip_arch.NAMED_CLIP_CONFIGS[name_or_kwargs] if isinstance(name_or_kwargs, str) else name_or_kwargs
        spec = clip_arch.clip_text_spec(**cfg)
        return cls(spec, clip_arch.clip_params_from_state_dict(spec, state_dict, prefix), device, **kw)

    # ------------------------------------------------------------------------------------------ weights
    def _pack(self, params):
        spec, dev = self.spec, self.device
        want = {k for k, _, _ in clip_arch.clip_param_table(spec)}
        if set(params) != want:
            raise KeyError(f'text encoder parameters: missing {sorted(want - set(params))[:4]}, unexpected {sorted(set(params) - want)[:4]}')
        g = lambda k: params[k].detach().to(device=dev, dtype=torch.float32).contiguous()
        w: Dict[str, torch.Tensor] = {}
        w['tok'], w['pos'] = g('text_model.embeddings.token_embedding.weight'), g('text_model.embeddings.position_embedding.weight')
        for i in range(spec.layers):
            p = f'text_model.encoder.layers.{i}'
            w[f'{i}.qkv.w'] = pack_linear_weight(torch.cat([g(f'{p}.self_attn.{x}_proj.weight') for x in 'qkv'], 0))
            w[f'{i}.qkv.b'] = torch.cat([g(f'{p}.self_attn.{x}_proj.bias') for x in 'qkv'], 0).contiguous()
            for dst, src in (('o', 'self_attn.out_proj'), ('fc1', 'mlp.fc1'), ('fc2', 'mlp.fc2')):
                w[f'{i}.{dst}.w'], w[f'{i}.{dst}.b'] = pack_linear_weight(g(f'{p}.{src}.weight')), g(f'{p}.{src}.bias')
            for dst, src in (('n1', 'layer_norm1'), ('n2', 'layer_norm2')):
                w[f'{i}.{dst}.g'], w[f'{i}.{dst}.b'] = g(f'{p}.{src}.weight'), g(f'{p}.{src}.bias')
        w['nf.g'], w['nf.b'] = g('text_model.final_layer_norm.weight'), g('text_model.final_layer_norm.bias')
        self.w = w

    # ------------------------------------------------------------------------------------------ plan
    def plan(self, N: int) -> Plan:
        if N in self._plans:
            return self._plans[N]
        spec, w = self.spec, self.w
        S, W, F, H, D = spec.positions, spec.width, spec.ffn, spec.heads, spec.head_dim
        M = N * S
        bd = Builder(self.device, conv_mode=0, autotune=False, invariant=self.batch_invariant, batch=N)
        P = bd.P
        tokens = torch.zeros(M, dtype=torch.int32, device=self.device)
        P.keep.append(tokens)
        P.bufs['tokens'] = tokens
        P.bufs['out'] = bd.new(M, W)
        x = bd.alloc(M, W)
        bd.token_embed(tokens, w['tok'], w['pos'], x, W, N, S, W, spec.vocab, 'embeddings')
        for i in range(spec.layers):
            p = f'layers.{i}'
            n = bd.alloc(M, W)
            bd.layernorm(x, W, w[f'{i}.n1.g'], w[f'{i}.n1.b'], spec.eps, n, W, M, W, p + '.layer_norm1')
            qkv = bd.alloc(M, 3 * W)
            bd.linear(n, W, M, w[f'{i}.qkv.w'], 3 * W, qkv, p + '.qkv', bias=w[f'{i}.qkv.b'])
            bd.free(n)
            ao = bd.alloc(M, W)
            bd.attention_causal(qkv, qkv[:, W:], qkv[:, 2 * W:], ao, p + '.attention', batch=N, heads=H, s=S, d=D, ldq=3 * W, ldk=3 * W,
                                ldv=3 * W, ldo=W, q_bs=S * 3 * W, k_bs=S * 3 * W, v_bs=S * 3 * W, o_bs=S * W, scale=float(D) ** -0.5)
            bd.free(qkv)
            x1 = bd.alloc(M, W)
            bd.linear(ao, W, M, w[f'{i}.o.w'], W, x1, p + '.out_proj', bias=w[f'{i}.o.b'], res=x, res_ld=W)
            bd.free(ao, x)
            n = bd.alloc(M, W)
            bd.layernorm(x1, W, w[f'{i}.n2.g'], w[f'{i}.n2.b'], spec.eps, n, W, M, W, p + '.layer_norm2')
            hid = bd.alloc(M, F)
            bd.linear(n, W, M, w[f'{i}.fc1.w'], F, hid, p + '.fc1', bias=w[f'{i}.fc1.b'])
            bd.free(n)
            bd.quick_gelu(hid, F, hid, F, M, F, p + '.quick_gelu')
            x = bd.alloc(M, W)
            bd.linear(hid, F, M, w[f'{i}.fc2.w'], W, x, p + '.fc2', bias=w[f'{i}.fc2.b'], res=x1, res_ld=W)
            bd.free(hid, x1)
        bd.layernorm(x, W, w['nf.g'], w['nf.b'], spec.eps, P.bufs['out'], W, M, W, 'final_layer_norm')
        bd.free(x)
        self._plans[N] = bd.finish()
        return P

    # ------------------------------------------------------------------------------------------ evaluation
    def flops(self, n_prompts=1):
        return clip_arch.clip_flops_per_prompt(self.spec) * n_prompts

    def check_tokens(self, tokens) -> torch.Tensor:
        """int32 [B, positions] on the host, validated: the kernel clamps, the host refuses."""
        spec = self.spec
        t = torch.as_tensor(tokens)
        if t.dim() != 2 or t.shape[1] != spec.positions or t.is_floating_point() or t.dtype == torch.bool:
            raise ValueError(f'ClipTextEncoder takes integer token ids [B, {spec.positions}], got {tuple(t.shape)} {t.dtype}')
        t = t.detach().cpu().to(torch.int64)
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= spec.vocab):
            raise ValueError(f'token id outside [0, {spec.vocab}): min {int(t.min())}, max {int(t.max())}')
        return t.to(torch.int32).contiguous()

    def raw(self, tokens):
        """Uploads the ids into the plan and runs it; returns (the plan's output buffer viewed [B, positions, width], plan)."""
        t = self.check_tokens(tokens)
        B = t.shape[0]
        plan = self.plan(B)
        plan.bufs['tokens'].copy_(t.reshape(-1), non_blocking=False)
        plan.run(_lib.stream_ptr())
        return plan.bufs['out'].view(B, self.spec.positions, self.spec.width), plan

    def __call__(self, tokens):
        out, _ = self.raw(tokens)
        return out.clone()
