"""Both CLIP towers of the reference's ``clip_score.py`` on the HIP engine (``clip_score_arch.ClipScoreSpec`` is the data model):
``ClipImageEncoder`` = ``model.encode_image`` / transformers ``CLIPModel.get_image_features``, ``ClipPooledTextEncoder`` =
``model.encode_text`` / ``get_text_features`` -- un-normalised [B, embed] features, fp32 in every mode (clip_score.py runs without autocast).

One encode = one flat launch list over token-major rows that MIXES the two libraries: the projections, LayerNorm, token embedding, causal
attention and quick_gelu are libdsamd entry points emitted through ``plan.Builder``; the bidirectional attention at head size 88, the erf-GELU,
the patch rows, the token assembly and the row gathers are libdsmetrics entry points (csrc/metrics/clip_score.hip) appended to the same
list.  ``Plan.run`` (the native walk inside libdsamd) cannot hold foreign launches, so these plans run through ``Plan.run_python``: about ten
ctypes calls per layer, noise next to a ViT-g layer.

    image     dsm_vit_patch_rows -> patch projection (no bias, K padded with zero columns to a multiple of 32) -> dsm_vit_tokens -> pre-LayerNorm
              per layer   LayerNorm -> q | k | v as ONE projection -> attention on the packed output in place (dsm_attention at d = 88,
                          ds_attention at the head sizes that kernel covers) -> out_proj (+ residual) -> LayerNorm -> fc1 -> GELU -> fc2 (+ residual)
              dsm_gather_rows (class row per image) -> post-LayerNorm -> visual_projection
    text      ds_token_embed -> the same layer with ds_attention_causal -> dsm_gather_rows (row of the first argmax(ids) per prompt, computed
              on the host) -> final LayerNorm (a row operation: applied to the B gathered rows only) -> text_projection

``dtype='fp16x3'`` (trailing keyword of both encoders; default ``'fp32'``, whose launch lists it leaves alone): the four projections of every
layer -- q | k | v, out_proj, fc1, fc2 -- become ``dsm_gemm_split`` launches (csrc/metrics/gemm_split.hip: fp32 operands split into two fp16
halves, three products on the fp16 matrix pipe, fp32 accumulation and fp32 results), fc1 carries the GELU in its epilogue (no GELU launch),
out_proj and fc2 the residual.  LayerNorm, attention, the token assembly, the gathers, the patch projection and the pooled head projection
stay on the fp32 kernels above.  Activations must stay inside fp16's range (|x| <= 65504); ``ClipScorer`` checks the features.

Plans build on ``device='cpu'`` without running anything (the launch list is then testable without a GPU); a geometry no kernel covers is a
``NotImplementedError`` at build time, never a fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict

import torch

from . import _lib, _metrics_lib, clip_score_arch as arch
from .ops import pack_linear_weight, pack_linear_weight_split
from .plan import Builder, Plan, ptr


DTYPES = ('fp32', 'fp16x3')


def _pack_layers(w, g, prefix, t, split=False):
    """split: the four projections as split-fp16 operands of dsm_gemm_split (ops.pack_linear_weight_split), their power-of-two shift under '<name>.s'."""
    def pack(dst, m):
        if split:
            w[f'{dst}.w'], w[f'{dst}.s'] = pack_linear_weight_split(m)
        else:
            w[f'{dst}.w'] = pack_linear_weight(m)

    for i in range(t.layers):
        p = f'{prefix}.encoder.layers.{i}'
        pack(f'{i}.qkv', torch.cat([g(f'{p}.self_attn.{x}_proj.weight') for x in 'qkv'], 0))
        w[f'{i}.qkv.b'] = torch.cat([g(f'{p}.self_attn.{x}_proj.bias') for x in 'qkv'], 0).contiguous()
        for dst, src in (('o', 'self_attn.out_proj'), ('fc1', 'mlp.fc1'), ('fc2', 'mlp.fc2')):
            pack(f'{i}.{dst}', g(f'{p}.{src}.weight'))
            w[f'{i}.{dst}.b'] = g(f'{p}.{src}.bias')
        for dst, src in (('n1', 'layer_norm1'), ('n2', 'layer_norm2')):
            w[f'{i}.{dst}.g'], w[f'{i}.{dst}.b'] = g(f'{p}.{src}.weight'), g(f'{p}.{src}.bias')


class _Tower:
    """What the two encoders share: the libraries, the per-batch plan cache, the transformer layer and the foreign launches."""
    prefix = ''

    def __init__(self, spec: arch.ClipScoreSpec, params: Dict[str, torch.Tensor], device='cuda', dtype='fp32'):
        if dtype not in DTYPES:
            raise ValueError(f'dtype must be one of {DTYPES}, got {dtype!r}')
        self.spec = spec
        self.device = torch.device(device)
        self.dtype = dtype
        self.split = dtype == 'fp16x3'
        self.lib = _lib.load()
        self.mlib = _metrics_lib.load()
        self._plans: Dict[int, Plan] = {}
        want = {k for k, _, _ in arch.clip_score_param_table(spec) if k.startswith(self.keys)}
        have = {k for k in params if k.startswith(self.keys)}
        if have != want:
            raise KeyError(f'{type(self).__name__} parameters: missing {sorted(want - have)[:4]}, unexpected {sorted(have - want)[:4]}')
        self._check_geometry()
        self._pack(lambda k: params[k].detach().to(device=self.device, dtype=torch.float32).contiguous())

    # ---- foreign (libdsmetrics) launches, appended to the builder's list -------------------------------------------------------------
    def _gelu(self, bd, x, ld, rows, cols, name):
        if self.spec.act == 'quick_gelu':
            bd.quick_gelu(x, ld, x, ld, rows, cols, name + '.quick_gelu')
        else:
            bd.add(self.mlib.dsm_gelu_rows, (ptr(x), ld, ptr(x), ld, rows, cols), name + '.gelu')

    def _gather(self, bd, x, ldx, x_rows, index, out, ldo, n, cols, name):
        bd.add(self.mlib.dsm_gather_rows, (ptr(x), ldx, x_rows, ptr(index), ptr(out), ldo, n, cols), name)

    def _attention(self, bd, qkv, ao, name, N, H, S, D, W, causal):
        kw = dict(ldq=3 * W, ldk=3 * W, ldv=3 * W, ldo=W, q_bs=S * 3 * W, k_bs=S * 3 * W, v_bs=S * 3 * W, o_bs=S * W, scale=float(D) ** -0.5)
        q, k, v = qkv, qkv[:, W:], qkv[:, 2 * W:]
        if causal:
            bd.attention_causal(q, k, v, ao, name, batch=N, heads=H, s=S, d=D, **kw)
        elif self.lib.ds_attention_supported(D):
            bd.attention(q, k, v, ao, name, batch=N, heads=H, sq=S, skv=S, d=D, **kw)
        else:
            a = _metrics_lib.DsmAttnArgs(ptr(q), ptr(k), ptr(v), ptr(ao), kw['ldq'], kw['ldk'], kw['ldv'], kw['ldo'], kw['q_bs'], kw['k_bs'],
                                         kw['v_bs'], kw['o_bs'], N, H, S, S, D, kw['scale'])
            bd.add(self.mlib.dsm_attention, (C.byref(a),), name, keep=(a,))

    def _split_linear(self, bd, x, k, rows, key, cout, out, name, res=None, act=_metrics_lib.DSM_ACT_NONE):
        """fp16x3: out[rows, cout] = act(x[rows, k] W^T + bias) + res as ONE dsm_gemm_split launch (dense operands)."""
        if not self.mlib.dsm_gemm_split_supported(rows, k, cout):
            raise NotImplementedError(f'{name}: dsm_gemm_split does not cover {rows} rows x {k} -> {cout} (k and cout must be multiples of 32)')
        w = self.w
        a = _metrics_lib.DsmGemmSplitArgs(ptr(x), k, rows, k, ptr(w[key + '.w']), w[key + '.s'], cout, ptr(w[key + '.b']), ptr(res), cout if res is not None else 0,
                                          act, ptr(out), cout)
        bd.add(self.mlib.dsm_gemm_split, (C.byref(a),), name, keep=(a,))

    def _split_ok(self, t, tower):
        """fp16x3 at build time: every projection of the tower's layers must be a geometry dsm_gemm_split takes."""
        if not self.split:
            return
        for name, k, cout in (('qkv', t.width, 3 * t.width), ('out_proj', t.width, t.width), ('fc1', t.width, t.ffn), ('fc2', t.ffn, t.width)):
            if not self.mlib.dsm_gemm_split_supported(1, k, cout):
                raise NotImplementedError(f"{tower} tower: dtype='fp16x3' has no kernel for {name} ({k} -> {cout}): width and ffn must be multiples of 32")

    def _attention_ok(self, D, S, causal):
        if causal:
            return bool(self.lib.ds_attention_causal_supported(D, S))
        return bool(self.lib.ds_attention_supported(D) or self.mlib.dsm_attention_supported(D))

    def _layers(self, bd, x, t, N, S, causal, tag):
        """The transformer layers over the [N * S, width] rows `x` (an alloc() buffer); returns the last layer's output."""
        w, eps = self.w, self.spec.eps
        W, F, H, D = t.width, t.ffn, t.heads, t.head_dim
        M = N * S
        for i in range(t.layers):
            p = f'{tag}.layers.{i}'
            n = bd.alloc(M, W)
            bd.layernorm(x, W, w[f'{i}.n1.g'], w[f'{i}.n1.b'], eps, n, W, M, W, p + '.layer_norm1')
            qkv = bd.alloc(M, 3 * W)
            if self.split:
                self._split_linear(bd, n, W, M, f'{i}.qkv', 3 * W, qkv, p + '.qkv')
            else:
                bd.linear(n, W, M, w[f'{i}.qkv.w'], 3 * W, qkv, p + '.qkv', bias=w[f'{i}.qkv.b'])
            bd.free(n)
            ao = bd.alloc(M, W)
            self._attention(bd, qkv, ao, p + '.attention', N, H, S, D, W, causal)
            bd.free(qkv)
            x1 = bd.alloc(M, W)
            if self.split:
                self._split_linear(bd, ao, W, M, f'{i}.o', W, x1, p + '.out_proj', res=x)
            else:
                bd.linear(ao, W, M, w[f'{i}.o.w'], W, x1, p + '.out_proj', bias=w[f'{i}.o.b'], res=x, res_ld=W)
            bd.free(ao, x)
            n = bd.alloc(M, W)
            bd.layernorm(x1, W, w[f'{i}.n2.g'], w[f'{i}.n2.b'], eps, n, W, M, W, p + '.layer_norm2')
            hid = bd.alloc(M, F)
            if self.split:               # the GELU rides in fc1's epilogue: no pass over [M, F] of its own
                act = _metrics_lib.DSM_ACT_QUICK_GELU if self.spec.act == 'quick_gelu' else _metrics_lib.DSM_ACT_GELU
                self._split_linear(bd, n, W, M, f'{i}.fc1', F, hid, p + '.fc1', act=act)
                bd.free(n)
                x = bd.alloc(M, W)
                self._split_linear(bd, hid, F, M, f'{i}.fc2', W, x, p + '.fc2', res=x1)
            else:
                bd.linear(n, W, M, w[f'{i}.fc1.w'], F, hid, p + '.fc1', bias=w[f'{i}.fc1.b'])
                bd.free(n)
                self._gelu(bd, hid, F, M, F, p)
                x = bd.alloc(M, W)
                bd.linear(hid, F, M, w[f'{i}.fc2.w'], W, x, p + '.fc2', bias=w[f'{i}.fc2.b'], res=x1, res_ld=W)
            bd.free(hid, x1)
        return x

    def _head(self, bd, x, x_rows, index, N, W, ng, nb, proj, name_norm, name_proj):
        """gather one row per item -> LayerNorm -> projection into P.bufs['out'] [N, embed]."""
        E = self.spec.embed
        pooled = bd.alloc(N, W)
        self._gather(bd, x, W, x_rows, index, pooled, W, N, W, 'pool')
        normed = bd.alloc(N, W)
        bd.layernorm(pooled, W, ng, nb, self.spec.eps, normed, W, N, W, name_norm)
        bd.P.bufs['out'] = bd.new(N, E)
        bd.linear(normed, W, N, proj, E, bd.P.bufs['out'], name_proj)
        bd.free(pooled, normed)

    def _builder(self, N):
        return Builder(self.device, conv_mode=0, autotune=False, batch=N)

    def _run(self, plan):
        plan.run_python(_lib.stream_ptr())


class ClipImageEncoder(_Tower):
    """``ClipImageEncoder(images) -> [B, embed]`` fp32 for uint8 (or fp32 in [0, 1]) images [B, 3, size, size]: ``CLIPModel.get_image_features``.
    The CLIP mean / std are applied on the device while the patch rows are formed."""
    keys = ('vision_model.', 'visual_projection.')

    def __init__(self, spec, params, device='cuda', mean=arch.CLIP_MEAN, std=arch.CLIP_STD, dtype='fp32'):
        self.mean, self.std = (C.c_float * 3)(*mean), (C.c_float * 3)(*std)
        super().__init__(spec, params, device, dtype)

    def _check_geometry(self):
        t, S = self.spec.vision, self.spec.vision_tokens
        if not self._attention_ok(t.head_dim, S, False):
            raise NotImplementedError(f'image tower: no attention kernel for head size {t.head_dim}')
        if t.width > 2048:
            raise NotImplementedError('image tower: the LayerNorm row kernel ends at 2048 columns')
        self._split_ok(t, 'image')

    def _pack(self, g):
        spec, w = self.spec, {}
        self.kpad = -(-spec.patch_k // 32) * 32              # the projection kernel contracts whole 32-column slabs: zero columns on both operands
        w['patch.w'] = pack_linear_weight(g('vision_model.embeddings.patch_embedding.weight').reshape(spec.vision.width, -1))
        assert w['patch.w'].shape[1] == self.kpad
        w['cls'], w['pos'] = g('vision_model.embeddings.class_embedding'), g('vision_model.embeddings.position_embedding.weight')
        _pack_layers(w, g, 'vision_model', spec.vision, self.split)
        for dst, src in (('pre', 'pre_layrnorm'), ('post', 'post_layernorm')):
            w[f'{dst}.g'], w[f'{dst}.b'] = g(f'vision_model.{src}.weight'), g(f'vision_model.{src}.bias')
        w['proj'] = pack_linear_weight(g('visual_projection.weight'))
        self.w = w

    def plan(self, N: int, f32=False) -> Plan:
        key = (N, bool(f32))
        if key in self._plans:
            return self._plans[key]
        spec, w, t = self.spec, self.w, self.spec.vision
        S, W, G = spec.vision_tokens, t.width, spec.grid
        M = N * S
        bd = self._builder(N)
        P = bd.P
        images = torch.zeros(N, 3, spec.image_size, spec.image_size, dtype=torch.float32 if f32 else torch.uint8, device=self.device)
        index = (torch.arange(N, dtype=torch.int32) * S).to(self.device)          # the class row of every image
        P.keep += [images, index]
        P.bufs['images'] = images
        rows = bd.alloc(N * G * G, self.kpad)
        bd.add(self.mlib.dsm_vit_patch_rows, (ptr(images), int(f32), N, spec.image_size, spec.patch, self.mean, self.std, ptr(rows), self.kpad),
               'patch_rows')
        pe = bd.alloc(N * G * G, W)
        bd.linear(rows, self.kpad, N * G * G, w['patch.w'], W, pe, 'patch_embedding')
        bd.free(rows)
        x0 = bd.alloc(M, W)
        bd.add(self.mlib.dsm_vit_tokens, (ptr(pe), W, ptr(w['cls']), ptr(w['pos']), ptr(x0), W, N, S, W), 'tokens')
        bd.free(pe)
        x = bd.alloc(M, W)
        bd.layernorm(x0, W, w['pre.g'], w['pre.b'], spec.eps, x, W, M, W, 'pre_layrnorm')
        bd.free(x0)
        x = self._layers(bd, x, t, N, S, False, 'vision')
        P.bufs['hidden'] = x                     # the last layer's output [N * tokens, width]: never recycled (the tests read it)
        self._head(bd, x, M, index, N, W, w['post.g'], w['post.b'], w['proj'], 'post_layernorm', 'visual_projection')
        self._plans[key] = bd.finish()
        return P

    def check_images(self, images) -> torch.Tensor:
        s = self.spec.image_size
        x = torch.as_tensor(images)
        if x.dim() != 4 or tuple(x.shape[1:]) != (3, s, s) or x.dtype not in (torch.uint8, torch.float32):
            raise ValueError(f'ClipImageEncoder takes uint8 (or fp32 in [0, 1]) images [B, 3, {s}, {s}], got {tuple(x.shape)} {x.dtype}')
        return x.contiguous()

    def raw(self, images):
        x = self.check_images(images)
        plan = self.plan(x.shape[0], x.dtype == torch.float32)
        plan.bufs['images'].copy_(x)
        self._run(plan)
        return plan.bufs['out'], plan

    def __call__(self, images):
        return self.raw(images)[0].clone()


def eot_index(tokens: torch.Tensor) -> torch.Tensor:
    """Position of the end-of-text token per prompt: the FIRST occurrence of the largest id (open_clip ``text.argmax(dim=-1)``; the
    end-of-text token has the largest id of the vocabulary), so whatever pads the row behind it is not looked at."""
    t = tokens.to(torch.int64)
    return (t == t.max(dim=1, keepdim=True).values).to(torch.int64).argmax(dim=1)


class ClipPooledTextEncoder(_Tower):
    """``ClipPooledTextEncoder(tokens) -> [B, embed]`` fp32 for int token ids [B, 77]: ``CLIPModel.get_text_features`` with the open_clip
    pooling rule (``eot_index``)."""
    keys = ('text_model.', 'text_projection.')

    def _check_geometry(self):
        t, S = self.spec.text, self.spec.positions
        if not self._attention_ok(t.head_dim, S, True):
            raise NotImplementedError(f'text tower: no causal attention kernel for head size {t.head_dim} over {S} tokens')
        if t.width > 2048:
            raise NotImplementedError('text tower: the LayerNorm row kernel ends at 2048 columns')
        self._split_ok(t, 'text')

    def _pack(self, g):
        spec, w = self.spec, {}
        w['tok'], w['pos'] = g('text_model.embeddings.token_embedding.weight'), g('text_model.embeddings.position_embedding.weight')
        _pack_layers(w, g, 'text_model', spec.text, self.split)
        w['nf.g'], w['nf.b'] = g('text_model.final_layer_norm.weight'), g('text_model.final_layer_norm.bias')
        w['proj'] = pack_linear_weight(g('text_projection.weight'))
        self.w = w

    def plan(self, N: int) -> Plan:
        if N in self._plans:
            return self._plans[N]
        spec, w, t = self.spec, self.w, self.spec.text
        S, W = spec.positions, t.width
        M = N * S
        bd = self._builder(N)
        P = bd.P
        tokens = torch.zeros(M, dtype=torch.int32, device=self.device)
        index = torch.zeros(N, dtype=torch.int32, device=self.device)
        P.keep += [tokens, index]
        P.bufs['tokens'], P.bufs['index'] = tokens, index
        x = bd.alloc(M, W)
        bd.token_embed(tokens, w['tok'], w['pos'], x, W, N, S, W, spec.vocab, 'embeddings')
        x = self._layers(bd, x, t, N, S, True, 'text')
        P.bufs['hidden'] = x
        self._head(bd, x, M, index, N, W, w['nf.g'], w['nf.b'], w['proj'], 'final_layer_norm', 'text_projection')
        self._plans[N] = bd.finish()
        return P

    def check_tokens(self, tokens) -> torch.Tensor:
        spec = self.spec
        t = torch.as_tensor(tokens)
        if t.dim() != 2 or t.shape[1] != spec.positions or t.is_floating_point() or t.dtype == torch.bool:
            raise ValueError(f'ClipPooledTextEncoder takes integer token ids [B, {spec.positions}], got {tuple(t.shape)} {t.dtype}')
        t = t.detach().cpu().to(torch.int64)
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= spec.vocab):
            raise ValueError(f'token id outside [0, {spec.vocab}): min {int(t.min())}, max {int(t.max())}')
        return t

    def raw(self, tokens):
        t = self.check_tokens(tokens)
        B, S = t.shape
        plan = self.plan(B)
        plan.bufs['tokens'].copy_(t.to(torch.int32).reshape(-1))
        plan.bufs['index'].copy_((torch.arange(B) * S + eot_index(t)).to(torch.int32))
        self._run(plan)
        return plan.bufs['out'], plan

    def __call__(self, tokens):
        return self.raw(tokens)[0].clone()
