"""Latent-diffusion denoiser on the HIP engine: drop-in for the reference ``CFGPrecond`` around the ldm ``UNetModel``
(diff-solvers-main/models/networks_edm.py:630-762; ldm/modules/diffusionmodules/openaimodel.py:413-742;
ldm/modules/attention.py:152-260) -- BASELINE config 5 (Stable Diffusion v1.5 latent U-Net, classifier-free guidance).

One evaluation = one flat plan of libdsamd launches over NHWC fp32 workspaces:

    ResBlock            GN stats -> 3x3 conv with GroupNorm+SiLU fused in its loader (+bias +time-embedding row)
                        -> GN stats -> 3x3 conv (fused norm) with the 1x1 skip_connection appended along K (+residual)
    SpatialTransformer  GN -> 1x1 proj_in -> [LN -> packed q|k|v linear -> fused attention -> to_out (+res)]
                        -> [LN -> q linear, context k|v linear -> fused cross-attention -> to_out (+res)]
                        -> [LN -> GEGLU linear with the gate in its epilogue -> linear (+res)] -> 1x1 proj_out (+res)
    Downsample          3x3 stride-2 conv;   Upsample: nearest x2 -> 3x3 conv
    CFG                 the conditional and unconditional halves run as ONE 2B-image evaluation (networks_edm.py:679-683);
                        ``ds_cfg_denoise`` forms F_u + g (F_c - F_u) and D = x - sigma F in one pass.

ResBlock halves, the head and Upsample are emitted by plan.Builder (gn_conv3x3, upsample_conv: shared with the AutoencoderKL decoder, the
routing rules live there); their temporaries are recycled (Builder.alloc / free), layer outputs and the skip stack live as long as the plan.
NHWC makes ``rearrange('b c h w -> b (h w) c')`` free: the transformer consumes the convolution outputs in place, and the
decoder's ``torch.cat([h, hs.pop()])`` is never materialised (dual-source convolutions).  Everything is fp32 (the
reference runs this U-Net under autocast; fp32 is the stricter contract -- DESIGN.md section 2).
"""
from __future__ import annotations

import math
import os
import weakref
from typing import Dict

import torch

from . import _lib, ldm_arch, ops
from ._lib import DS_ACT_GEGLU, DS_ACT_SILU
from .ops import pack_conv_weight, pack_conv_weight_f16, pack_linear_weight, pack_stem_weight
from .plan import FUSE_NORM16_DEFAULT, Builder, Plan, fuse_norm16_value, ptr


class LDMUNetEngine:
    def __init__(self, spec: ldm_arch.LDMUNetSpec, params: Dict[str, torch.Tensor], device='cuda', use_fp16=False, qkv_f16_min_head=40, f16_downsample=True,
                 batch_invariant=False):
        """use_fp16: the reference samples this U-Net under ``autocast("cuda")`` (diff-solvers-main/sample.py:296): convolutions and
        Linear layers multiply fp16 operands (fp32 accumulation here) and emit fp16 tensors.  Here: ResBlock / Upsample convolutions, every
        projection of the transformer blocks and attention on the fp16 kernels, and the activations between layers -- residual stream,
        skip stack, the transformer's x -- stored as fp16 rows wherever a layer runs on the fp16-activation kernels (plan(): per layer);
        norm / softmax arithmetic, the context projections and the time embedding are fp32.  qkv_f16_min_head: q / k / v of the attention
        layers with at least this head size are the fp16 rows their projections emit under autocast (smaller heads: fp32 rows the attention
        kernel rounds itself); f16_downsample: the strided Downsample convolutions read and write the fp16 stream (False: an fp32 copy and the
        generic fp32 kernel, the round-3 routing) -- A/B knobs of benchmarks, the defaults are what the parity goldens were made with.
        batch_invariant: the batch-invariant route in every plan (engine.UNetEngine)."""
        self.batch_invariant = bool(batch_invariant)
        self.qkv_f16_min_head = int(qkv_f16_min_head)
        self.f16_downsample = bool(f16_downsample)
        self.fuse_norm16 = fuse_norm16_value(os.environ.get('DS_FUSE_NORM16', FUSE_NORM16_DEFAULT))     # see engine.UNetEngine.fuse_norm16 ('auto': SD-1.5 has no such layer class)
        self.spec = spec
        self.device = torch.device(device)
        self.use_fp16 = bool(use_fp16)
        self._w16_cache = {}        # fp16 packings of the Linear / 1x1 weights (plan.Builder.linear_w16), shared by every plan
        self.lib = _lib.load()
        self._plans: Dict[tuple, Plan] = {}
        self._pack(params)

    # ------------------------------------------------------------------------------------------ weights
    def _pack(self, params):
        spec, dev = self.spec, self.device
        g = lambda k: params[k].detach().to(device=dev, dtype=torch.float32).contiguous()
        w: Dict[str, torch.Tensor] = {}
        half = spec.model_channels // 2
        w['freqs'] = torch.exp(-math.log(10000) * torch.arange(0, half, dtype=torch.float32) / half).to(dev)   # util.py:162-164
        w['te0.w'], w['te0.b'] = pack_linear_weight(g('time_embed.0.weight')), g('time_embed.0.bias')
        w['te2.w'], w['te2.b'] = pack_linear_weight(g('time_embed.2.weight')), g('time_embed.2.bias')
        aff_w, aff_b, off = [], [], 0
        self.aff_off: Dict[str, int] = {}
        for l in spec.res_layers():                  # every ResBlock's emb_layers Linear, concatenated into one GEMM
            aff_w.append(g(f'{l.key}.emb_layers.1.weight')); aff_b.append(g(f'{l.key}.emb_layers.1.bias'))
            self.aff_off[l.key] = off
            off += l.cout
        self.aff_total = off
        w['aff.w'], w['aff.b'] = pack_linear_weight(torch.cat(aff_w, 0)), torch.cat(aff_b, 0).contiguous()
        if spec.step_condition:
            # SFD's step condition (sfd-main/.../openaimodel.py:563, :234, :298-316): `nfe_embed` next to `time_embed`, and every ResBlock adds
            # emb_nfe_layers(emb_nfe) to emb_layers(emb) (no scale-shift norm in this U-Net) -- one projection of the single step row over the
            # concatenated weights, whose bias carries both layers' and whose output row is the BIAS of the emb_layers launch
            w['ne0.w'], w['ne0.b'] = pack_linear_weight(g('nfe_embed.0.weight')), g('nfe_embed.0.bias')
            w['ne2.w'], w['ne2.b'] = pack_linear_weight(g('nfe_embed.2.weight')), g('nfe_embed.2.bias')
            w['affs.w'] = pack_linear_weight(torch.cat([g(f'{l.key}.emb_nfe_layers.1.weight') for l in spec.res_layers()], 0))
            w['affs.b'] = (w['aff.b'] + torch.cat([g(f'{l.key}.emb_nfe_layers.1.bias') for l in spec.res_layers()], 0)).contiguous()
        for b in spec.blocks:
            for l in b.layers:
                p = l.key
                if l.kind == 'stem':
                    w[f'{p}.w'], w[f'{p}.b'] = pack_stem_weight(g(f'{p}.weight')), g(f'{p}.bias')
                elif l.kind == 'res':
                    for n_, src in (('n0', 'in_layers.0'), ('n1', 'out_layers.0')):
                        w[f'{p}.{n_}.g'], w[f'{p}.{n_}.b'] = g(f'{p}.{src}.weight'), g(f'{p}.{src}.bias')
                    w[f'{p}.c0.w'], w[f'{p}.c0.b'] = pack_conv_weight(g(f'{p}.in_layers.2.weight')), g(f'{p}.in_layers.2.bias')
                    c1 = pack_conv_weight(g(f'{p}.out_layers.3.weight'))
                    b1 = g(f'{p}.out_layers.3.bias')
                    if l.skip_conv:      # 1x1 skip_connection fused into the second conv: extra K columns, biases summed
                        c1 = torch.cat([c1, pack_conv_weight(g(f'{p}.skip_connection.weight'))], dim=1).contiguous()
                        b1 = (b1 + g(f'{p}.skip_connection.bias')).contiguous()
                    w[f'{p}.c1.w'], w[f'{p}.c1.b'] = c1, b1
                    if self.use_fp16 and l.cin % 64 == 0 and l.cout % 64 == 0:
                        w[f'{p}.c0.w16'] = (pack_conv_weight_f16(g(f'{p}.in_layers.2.weight')), 0)
                        w[f'{p}.c1.w16'] = (pack_conv_weight_f16(g(f'{p}.out_layers.3.weight'),
                                                                 g(f'{p}.skip_connection.weight') if l.skip_conv else None), 0)
                elif l.kind == 'st':
                    t = f'{p}.transformer_blocks.0'
                    w[f'{p}.n.g'], w[f'{p}.n.b'] = g(f'{p}.norm.weight'), g(f'{p}.norm.bias')
                    w[f'{p}.pi.w'], w[f'{p}.pi.b'] = pack_conv_weight(g(f'{p}.proj_in.weight')), g(f'{p}.proj_in.bias')
                    w[f'{p}.po.w'], w[f'{p}.po.b'] = pack_conv_weight(g(f'{p}.proj_out.weight')), g(f'{p}.proj_out.bias')
                    w[f'{p}.qkv1.w'] = pack_linear_weight(torch.cat([g(f'{t}.attn1.to_{x}.weight') for x in 'qkv'], 0))
                    w[f'{p}.q2.w'] = pack_linear_weight(g(f'{t}.attn2.to_q.weight'))
                    w[f'{p}.kv2.w'] = pack_linear_weight(torch.cat([g(f'{t}.attn2.to_{x}.weight') for x in 'kv'], 0))
                    for a in ('attn1', 'attn2'):
                        w[f'{p}.{a}.o.w'], w[f'{p}.{a}.o.b'] = pack_linear_weight(g(f'{t}.{a}.to_out.0.weight')), g(f'{t}.{a}.to_out.0.bias')
                    # GEGLU projection with the gate fused into its epilogue: rows reordered so that every 64-row block of
                    # the packed weight = 32 value rows followed by their 32 gate rows (DS_ACT_GEGLU)
                    inner = 4 * l.cin
                    perm = torch.arange(2 * inner, device=dev).reshape(-1, 2, 32)
                    perm = (perm[:, 0] // 64 * 32 + perm[:, 0] % 32).reshape(-1, 1, 32).repeat(1, 2, 1)
                    perm[:, 1] += inner
                    perm = perm.reshape(-1)
                    w[f'{p}.ff0.w'] = pack_linear_weight(g(f'{t}.ff.net.0.proj.weight')[perm])
                    w[f'{p}.ff0.b'] = g(f'{t}.ff.net.0.proj.bias')[perm].contiguous()
                    w[f'{p}.ff2.w'], w[f'{p}.ff2.b'] = pack_linear_weight(g(f'{t}.ff.net.2.weight')), g(f'{t}.ff.net.2.bias')
                    for n_ in ('norm1', 'norm2', 'norm3'):
                        w[f'{p}.{n_}.g'], w[f'{p}.{n_}.b'] = g(f'{t}.{n_}.weight'), g(f'{t}.{n_}.bias')
                elif l.kind == 'down':
                    w[f'{p}.w'], w[f'{p}.b'] = pack_conv_weight(g(f'{p}.op.weight')), g(f'{p}.op.bias')
                    if self.use_fp16 and l.cin % 64 == 0 and l.cout % 64 == 0:
                        w[f'{p}.w16'] = (pack_conv_weight_f16(g(f'{p}.op.weight')), 0)     # [slab][tap][64]: the stride-1 packing, gathered by the GEMM
                elif l.kind == 'up':
                    w[f'{p}.w'], w[f'{p}.b'] = pack_conv_weight(g(f'{p}.conv.weight')), g(f'{p}.conv.bias')
                    if self.use_fp16 and l.cin % 64 == 0:
                        w[f'{p}.w16'] = (pack_conv_weight_f16(g(f'{p}.conv.weight')), 0)
        w['out.g'], w['out.b'] = g('out.0.weight'), g('out.0.bias')
        w['outc.w'], w['outc.b'] = pack_conv_weight(g('out.2.weight')), g('out.2.bias')
        self.w = w

    # ------------------------------------------------------------------------------------------ plan
    def plan(self, N: int, emb_rows: int, ctx_len: int, step: bool = False) -> Plan:
        """N = images in the U-Net batch (2B under classifier-free guidance); emb_rows = 1 (shared sigma) or N.  step: the plan of an
        evaluation with a step condition (a one-float input `bufs['step']`, four more launches); False is the plan of a net without step weights."""
        step = bool(step)
        if step and not self.spec.step_condition:
            raise ValueError('this network was built without step-condition weights (LDMUNetSpec.step_condition)')
        key = (N, emb_rows, ctx_len, self.fuse_norm16) + ((True,) if step else ())
        if key in self._plans:
            return self._plans[key]
        spec, w, lib = self.spec, self.w, self.lib
        bd = Builder(self.device, conv_mode=(1 if self.use_fp16 else 0), w16_cache=self._w16_cache, invariant=self.batch_invariant, batch=N)
        P, new = bd.P, bd.new
        bufs = P.bufs
        R, Cin, MC, E = spec.img_resolution, spec.in_channels, spec.model_channels, spec.time_embed_dim
        if not lib.ds_attention_supported(MC // spec.num_heads):
            raise NotImplementedError(f'attention head size {MC // spec.num_heads} has no kernel instantiation')
        kpad = -(-9 * Cin // 32) * 32
        bufs['x'] = new(N, Cin, R, R)
        bufs['sigma'] = new(emb_rows)
        bufs['c_noise'] = new(emb_rows)
        bufs['context'] = new(N * ctx_len, spec.context_dim)
        bufs['out'] = new(N * R * R, 4)
        bd.coefs = new(N * 3 * max(max(l.cin, l.cout) for b in spec.blocks for l in b.layers))

        # ---- time embedding (openaimodel.py:726-727) and every ResBlock's emb_layers in one GEMM ---------------------------
        pos, e0, emb, aff = new(emb_rows, MC), new(emb_rows, E), new(emb_rows, E), new(emb_rows, self.aff_total)
        bd.add(lib.ds_noise_embed, (ptr(bufs['c_noise']), emb_rows, ptr(w['freqs']), MC, 2, ptr(pos), MC), 'timestep_embedding')
        bd.linear(pos, MC, emb_rows, w['te0.w'], E, e0, 'time_embed.0', bias=w['te0.b'], act=DS_ACT_SILU, emb=True)
        bd.linear(e0, E, emb_rows, w['te2.w'], E, emb, 'time_embed.2', bias=w['te2.b'], act=DS_ACT_SILU, emb=True)   # SiLU of emb_layers[0]
        aff_bias = w['aff.b']
        if step:         # one row serves every image (both halves of a classifier-free evaluation): openaimodel.py:783-786 on the raw step value
            bufs['step'] = new(1)
            spos, s0, semb, srow = new(1, MC), new(1, E), new(1, E), new(1, self.aff_total)
            bd.add(lib.ds_noise_embed, (ptr(bufs['step']), 1, ptr(w['freqs']), MC, 2, ptr(spos), MC), 'step_embedding')
            bd.linear(spos, MC, 1, w['ne0.w'], E, s0, 'nfe_embed.0', bias=w['ne0.b'], act=DS_ACT_SILU, emb=True)
            bd.linear(s0, E, 1, w['ne2.w'], E, semb, 'nfe_embed.2', bias=w['ne2.b'], act=DS_ACT_SILU, emb=True)   # SiLU of emb_nfe_layers[0]
            bd.linear(semb, E, 1, w['affs.w'], self.aff_total, srow, 'emb_nfe_layers_all', bias=w['affs.b'], emb=True)
            bufs['aff_step'] = aff_bias = srow
        bd.linear(emb, E, emb_rows, w['aff.w'], self.aff_total, aff, 'emb_layers_all', bias=aff_bias, emb=True)

        # ---- fp16 residual stream: under torch.autocast (sample.py:293-297) the reference's convolutions and Linear layers emit fp16
        # tensors, so every activation between layers is fp16.  Every ResBlock / SpatialTransformer / upsampling convolution that runs on
        # the fp16-activation kernels stores its output (the residual stream h, the skip stack hs, the transformer's x) as fp16 rows
        # too; arithmetic on them is fp32 (widened on load).  A layer without such a kernel at its geometry reads an fp32 copy
        # (Builder.widen) and writes fp32; every consumer takes a tensor in the dtype it has.
        stream16 = bd.conv_mode == 1
        P.stream16 = stream16
        new_act = (lambda *shape: bd.new16(*shape)) if stream16 else new

        def res_layer(l, x0, c0, x1, c1):
            p, res, cout = l.key, l.res_out, l.cout
            M = N * res * res
            cin = c0 + c1
            f16 = bool(bd.f16_conv_ok(N, res, cin, 0, cout) and bd.f16_conv_ok(N, res, cout, cin if l.skip_conv else 0, cout))
            conv0 = dict(w16=w.get(f'{p}.c0.w16'), f16=f16, fuse_norm16=self.fuse_norm16, cbias=aff[:, self.aff_off[p]:], cbias_ld=self.aff_total, cbias_rows=emb_rows)
            conv1 = dict(w16=w.get(f'{p}.c1.w16'), f16=f16, fuse_norm16=self.fuse_norm16)
            if not l.skip_conv:
                assert x1 is None and c0 == cout
            if f16:
                # the 1x1 skip_connection rides in the second convolution as extra K columns on raw fp16 rows: the input itself when it is
                # one fp16 tensor, both raw sources in place when in_layers normalises its own halo (fuses_norm16), else a raw copy the
                # in_layers pass writes next to the activated tensor
                direct = x1 is None and x0.dtype == torch.float16
                if not l.skip_conv:
                    conv1.update(res=x0, res_ld=cout)
                elif direct:
                    conv1.update(e16=(x0, cin))
                elif bd.fuses_norm16(self.fuse_norm16, res, cout, x0, c0, x1, c1):
                    conv1.update(e16=(x0, c0, x1, c1))
                else:
                    conv0.update(raw16=bd.new16(M, cin))
                    conv1.update(e16=(conv0['raw16'], cin))
            else:
                x0, x1 = bd.widen(x0, c0, N, res, p + '.x0'), bd.widen(x1, c1, N, res, p + '.x1')
                conv1.update(dict(e0=x0, ec0=c0, e1=x1, ec1=c1) if l.skip_conv else dict(res=x0, res_ld=cout))
            h1 = bd.new16(M, cout) if f16 else new(M, cout)      # in_layers output: only read by the out_layers normalisation
            out = new_act(M, cout) if f16 else new(M, cout)
            bd.gn_conv3x3(x0, c0, x1, c1, N, res, w[f'{p}.n0.g'], w[f'{p}.n0.b'], w[f'{p}.c0.w'], w[f'{p}.c0.b'], cout, h1, cout, p + '.in_layers',
                          **conv0)
            bd.gn_conv3x3(h1, cout, None, 0, N, res, w[f'{p}.n1.g'], w[f'{p}.n1.b'], w[f'{p}.c1.w'], w[f'{p}.c1.b'], cout, out, cout,
                          p + '.out_layers', **conv1)
            return out, cout

        def st_layer(l, x_in, c):
            p, res, hd = l.key, l.res_out, l.heads
            S = res * res
            M = N * S
            d = c // hd
            L = ctx_len
            # fp16 mode: tensors that are only the operand of the next projection -- the GroupNorm output, the three LayerNorm outputs,
            # both attention outputs, the GEGLU product -- are stored as fp16 rows and streamed by the fp16-activation GEMM
            # (csrc/gemm_f16dma.hip); with the fp16 stream (`ts`) so is the transformer's residual stream t0 .. t3; q / k / v stay fp32
            h16 = bool(lib.ds_attention_f16_supported(d) and all(bd.gemm16_ok(M, k, o) for k, o in ((c, c), (c, 3 * c), (c, 8 * c), (4 * c, c))))
            mk = bd.new16 if h16 else new
            ts = new_act if h16 else new                     # the transformer's residual stream t0 .. t3 and its output
            if not h16:
                x_in = bd.widen(x_in, c, N, res, p + '.x')
            n2, t0, ln, ao = mk(M, c), ts(M, c), mk(M, c), mk(M, c)
            bd.norm('stats', x_in, c, c, N, res, res, p + '.norm.stats', groups=32, eps=1e-6)
            bd.norm('apply', x_in, c, c, N, res, res, p + '.norm', groups=32, eps=1e-6, gamma=w[f'{p}.n.g'], beta=w[f'{p}.n.b'],
                    out=n2, out_ld=c, out_f16=h16)
            bd.conv(n2, c, c, N, res, res, w[f'{p}.pi.w'], c, t0, c, 1, p + '.proj_in', bias=w[f'{p}.pi.b'])
            # self-attention
            # fp16 mode: q | k | v as the fp16 rows the projections emit under autocast.  Round 3 kept fp32 rows at d = 40 (S = 4 096), where the
            # attention kernel was 10 % slower on fp16 rows; that was the lockstep of a lone workgroup per CU, removed in round 4
            # (profiles/r4_attn_f16_occupancy_ab.txt: 1.73 vs 1.70 ms at 32 images), and the halved output of the 320 -> 960 projection (HBM-bound:
            # 503 -> 252 MB at 32 images) is worth more than that
            mq = mk if d >= self.qkv_f16_min_head else new
            qkv, t1 = mq(M, 3 * c), ts(M, c)
            bd.layernorm(t0, c, w[f'{p}.norm1.g'], w[f'{p}.norm1.b'], 1e-5, ln, c, M, c, p + '.norm1')
            bd.linear(ln, c, M, w[f'{p}.qkv1.w'], 3 * c, qkv, p + '.attn1.qkv')
            bd.attention(qkv, qkv[:, c:], qkv[:, 2 * c:], ao, p + '.attn1', batch=N, heads=hd, sq=S, skv=S, d=d, ldq=3 * c, ldk=3 * c,
                         ldv=3 * c, ldo=c, q_bs=S * 3 * c, k_bs=S * 3 * c, v_bs=S * 3 * c, o_bs=S * c, scale=d ** -0.5)
            bd.linear(ao, c, M, w[f'{p}.attn1.o.w'], c, t1, p + '.attn1.to_out', bias=w[f'{p}.attn1.o.b'], res=t0, res_ld=c)
            # cross-attention over the context tokens
            q2, kv2, t2 = mq(M, c), new(N * L, 2 * c), ts(M, c)          # the context's k | v (fp32 projection of fp32 states, once per context) stay fp32
            bd.layernorm(t1, c, w[f'{p}.norm2.g'], w[f'{p}.norm2.b'], 1e-5, ln, c, M, c, p + '.norm2')
            bd.linear(ln, c, M, w[f'{p}.q2.w'], c, q2, p + '.attn2.q')
            bd.linear(bufs['context'], spec.context_dim, N * L, w[f'{p}.kv2.w'], 2 * c, kv2, p + '.attn2.kv')
            bd.attention(q2, kv2, kv2[:, c:], ao, p + '.attn2', batch=N, heads=hd, sq=S, skv=L, d=d, ldq=c, ldk=2 * c, ldv=2 * c, ldo=c,
                         q_bs=S * c, k_bs=L * 2 * c, v_bs=L * 2 * c, o_bs=S * c, scale=d ** -0.5)
            bd.linear(ao, c, M, w[f'{p}.attn2.o.w'], c, t2, p + '.attn2.to_out', bias=w[f'{p}.attn2.o.b'], res=t1, res_ld=c)
            # GEGLU feed-forward
            gg, t3 = mk(M, 4 * c), ts(M, c)
            bd.layernorm(t2, c, w[f'{p}.norm3.g'], w[f'{p}.norm3.b'], 1e-5, ln, c, M, c, p + '.norm3')
            bd.linear(ln, c, M, w[f'{p}.ff0.w'], 8 * c, gg, p + '.ff.proj_geglu', out_ld=4 * c, bias=w[f'{p}.ff0.b'], act=DS_ACT_GEGLU)
            bd.linear(gg, 4 * c, M, w[f'{p}.ff2.w'], c, t3, p + '.ff.out', bias=w[f'{p}.ff2.b'], res=t2, res_ld=c)
            out = ts(M, c)
            bd.conv(t3, c, c, N, res, res, w[f'{p}.po.w'], c, out, c, 1, p + '.proj_out', bias=w[f'{p}.po.b'], res=x_in, res_ld=c,
                    stats=True)
            return out, c

        cur = None
        skips = []
        for b in spec.blocks:
            x1, c1 = (None, 0)
            if b.pops_skip:
                x1, c1 = skips.pop()
                assert c1 == b.skip_cin
            for l in b.layers:
                p = l.key
                if l.kind == 'stem':
                    col = new(N * R * R, kpad)
                    bd.add(lib.ds_stem_im2col, (ptr(bufs['x']), ptr(bufs['sigma']), emb_rows, 1.0, N, Cin, R, R, ptr(col), kpad),
                           'stem_im2col')      # c_in = 1/sqrt(sigma^2 + 1): EDM's c_in with sigma_data = 1
                    out = new(N * R * R, l.cout)
                    bd.conv(col, kpad, kpad, N, R, R, w[f'{p}.w'], l.cout, out, l.cout, 1, p, bias=w[f'{p}.b'], stats=True)
                    cur = (out, l.cout)
                elif l.kind == 'res':
                    cur = res_layer(l, cur[0], cur[1], x1, c1)
                    x1, c1 = None, 0
                elif l.kind == 'st':
                    cur = st_layer(l, cur[0], cur[1])
                elif l.kind == 'down':
                    # fp16 mode, input on the fp16 stream: the strided convolution is the fp16-activation GEMM with a gathered A tile
                    # (csrc/gemm_f16dma.hip, GATHER) and its output joins the fp16 stream (under autocast the reference's Downsample
                    # conv emits fp16, openaimodel.py:146-148); otherwise an fp32 copy of the input and the generic fp32 kernel
                    f16dn = bool(self.f16_downsample and w.get(f'{p}.w16') is not None and stream16 and cur[0].dtype == torch.float16
                                 and bd.stride2_ok(N, l.res_out, l.cin, l.cout))
                    if f16dn:
                        out = new_act(N * l.res_out ** 2, l.cout)
                        bd.conv(cur[0], l.cin, l.cin, N, l.res_out, l.res_out, w[f'{p}.w'], l.cout, out, l.cout, 9, p + '.op',
                                bias=w[f'{p}.b'], stride=2, stats=True, w16=w[f'{p}.w16'], in_f16=True)
                    else:
                        out = new(N * l.res_out ** 2, l.cout)
                        cur = (bd.widen(cur[0], l.cin, N, l.res_in, p), l.cin)      # the strided convolution reads fp32 rows
                        bd.conv(cur[0], l.cin, l.cin, N, l.res_out, l.res_out, w[f'{p}.w'], l.cout, out, l.cout, 9, p + '.op',
                                bias=w[f'{p}.b'], stride=2, stats=True)
                    cur = (out, l.cout)
                elif l.kind == 'up':
                    cur = (bd.upsample_conv(cur[0], l.cin, N, l.res_in, w[f'{p}.w'], w[f'{p}.b'], l.cout, p, w16=w.get(f'{p}.w16')), l.cout)
                bufs[p] = cur[0]
            if b.pushes_skip:
                skips.append(cur)
        assert not skips
        bd.gn_conv3x3(cur[0], cur[1], None, 0, N, R, w['out.g'], w['out.b'], w['outc.w'], w['outc.b'], spec.out_channels, bufs['out'], 4, 'out')
        bd.finish()
        # The cross-attention key / value projections (ldm/modules/attention.py:168-176: to_k(context), to_v(context)) depend on the text
        # context only -- not on x or sigma -- so they form their own small plan that CFGDenoiser runs once per context, not once per
        # network evaluation (16 launches of 361 at SD-1.5 size)
        P.ctx = Plan()
        P.ctx.ops = [op for op in P.ops if op.name.endswith('.attn2.kv')]
        P.ops = [op for op in P.ops if not op.name.endswith('.attn2.kv')]
        P.ctx_key = None
        self._plans[key] = P
        return P

    def flops(self, n_images, ctx_len=77):
        return ldm_arch.ldm_flops_per_image(self.spec, ctx_len) * n_images


def _interp(x, xp, yp):
    """Piecewise-linear through (xp ascending, yp), linearly extended beyond both ends (CFGPrecond.interpolate_fn,
    networks_edm.py:716-759)."""
    K = xp.shape[0]
    i = torch.searchsorted(xp, x.contiguous()).clamp(1, K - 1) - 1
    return yp[i] + (x - xp[i]) * (yp[i + 1] - yp[i]) / (xp[i + 1] - xp[i])


def ldm_spec_from_module(unet, img_resolution, params=None):
    """Recover the LDMUNetSpec of a live reference ``UNetModel`` (duck-typed) from the constructor arguments it keeps as attributes
    (openaimodel.py:540-553) and from its state dict `params` (default: ``unet.state_dict()``): the context width is ``attn2.to_k``'s, and
    ``step_condition`` is read off ``nfe_embed`` / ``emb_nfe_layers`` (SFD's distilled U-Net) -- one group without the other raises, and so does
    a state dict that is not the spec's key list: nothing is dropped or left unset without a word."""
    params = dict(unet.state_dict()) if params is None else params
    ctx = [v.shape[1] for k, v in params.items() if k.endswith('.attn2.to_k.weight')]
    if not ctx:
        raise NotImplementedError('UNetModel without cross-attention (use_spatial_transformer=False) is not supported')
    has_embed = any(k.startswith('nfe_embed.') for k in params)
    has_layers = any('.emb_nfe_layers.' in k for k in params)
    if has_embed != has_layers:
        raise ValueError(f'inconsistent step-condition layers: nfe_embed {"present" if has_embed else "absent"}, emb_nfe_layers '
                         f'{"present" if has_layers else "absent"}')
    spec = ldm_arch.ldm_unet_spec(img_resolution=int(img_resolution), in_channels=int(unet.in_channels), out_channels=int(unet.out_channels),
                                  model_channels=int(unet.model_channels), attention_resolutions=tuple(int(v) for v in unet.attention_resolutions),
                                  num_res_blocks=int(unet.num_res_blocks), channel_mult=tuple(int(v) for v in unet.channel_mult),
                                  num_heads=int(unet.num_heads), context_dim=int(ctx[0]), step_condition=has_embed)
    want = {k: tuple(shape) for k, shape, _ in ldm_arch.ldm_param_table(spec)}
    got = {k: tuple(v.shape) for k, v in params.items()}
    if want != got:
        odd = sorted(set(want) ^ set(got)) or sorted(k for k in want if want[k] != got[k])
        raise NotImplementedError(f'the U-Net\'s state dict is not that of the recovered spec ({len(odd)} entries differ: {odd[:4]} ...)')
    return spec


class CFGSchedule:
    """The host side of ``CFGPrecond`` (networks_edm.py:654-661, 692-714): sigma(t), its inverse and the schedule end points,
    piecewise-linear over the ``alphas_cumprod`` table, evaluated in fp32 with the reference's formulas.  Pure host code."""

    def __init__(self, spec: ldm_arch.LDMUNetSpec):
        log_alphas = 0.5 * torch.log(ldm_arch.alphas_cumprod(spec))
        self.M = len(log_alphas)
        self.t_array = torch.linspace(0., 1., self.M + 1)[1:]
        self.log_alpha_array = log_alphas
        self.sigma_min = float(self.sigma(spec.epsilon_t))
        self.sigma_max = float(self.sigma(1))

    def sigma(self, t):
        dev = t.device if isinstance(t, torch.Tensor) else None
        t = torch.as_tensor(t, dtype=torch.float32).detach().cpu().reshape(-1)
        lmc = _interp(t, self.t_array, self.log_alpha_array)
        out = torch.sqrt(1. - torch.exp(2. * lmc)) / torch.exp(lmc)
        return out.to(dev) if dev is not None else out

    def sigma_inv(self, sigma):
        dev = sigma.device if isinstance(sigma, torch.Tensor) else None
        sigma = torch.as_tensor(sigma, dtype=torch.float32).detach().cpu().reshape(-1)
        log_alpha = -0.5 * torch.logaddexp(torch.zeros((1,)), -2. * (-(sigma.log())))
        out = _interp(log_alpha, torch.flip(self.log_alpha_array, [0]), torch.flip(self.t_array, [0]))
        return out.to(dev) if dev is not None else out

    def round_sigma(self, sigma):
        return torch.as_tensor(sigma)


class CFGDenoiser(CFGSchedule):
    """Drop-in for the reference ``CFGPrecond`` object (networks_edm.py:630-762): ``net(x, sigma, condition=...,
    unconditional_condition=...)`` -> denoised latents NCHW fp32, plus the attributes and methods the samplers and
    ``get_schedule('discrete')`` read (``guidance_type, guidance_rate, img_resolution, img_channels, label_dim, sigma_min,
    sigma_max, sigma(), sigma_inv(), round_sigma()``)."""
    host_sigma_ok = True       # solvers._Run: pass sigma as a Python float (c_noise is host math; nothing to copy or sync)

    def __init__(self, spec: ldm_arch.LDMUNetSpec, params: Dict[str, torch.Tensor], device='cuda', guidance_rate=None,
                 guidance_type=None, use_fp16=False, batch_invariant=False, decoder=None, text_encoder=None, **engine_kw):
        """batch_invariant: same seed, same bits at any batch (LDMUNetEngine).
        decoder: optional vae_engine.VAEDecoder -- the first stage that turns this denoiser's latents into images (``net.decoder(z)``, the
        reference's ``net.model.decode_first_stage``); not used by the denoiser itself.
        text_encoder: optional clip_engine.ClipTextEncoder -- the conditioning stage (``net.text_encoder(tokens)``, the reference's
        ``net.model.get_learned_conditioning`` after its tokenizer); not used by the denoiser itself either."""
        self.spec = spec
        self.decoder = decoder
        self.text_encoder = text_encoder
        self.engine = LDMUNetEngine(spec, params, device, use_fp16=use_fp16, batch_invariant=batch_invariant, **engine_kw)
        self.batch_invariant = bool(batch_invariant)
        self.device = self.engine.device
        self.guidance_rate = spec.guidance_rate if guidance_rate is None else guidance_rate
        self.guidance_type = spec.guidance_type if guidance_type is None else guidance_type
        self.img_resolution, self.img_channels, self.label_dim = spec.img_resolution, spec.in_channels, True
        CFGSchedule.__init__(self, spec)                                    # host tables (networks_edm.py:654-658)
        self.use_fp16 = bool(use_fp16)      # the reference's autocast mode (sample.py:296); fixed at construction
        self.cache_context = True           # cross-attention K / V projections once per context tensor, not once per evaluation
        self._last = None                   # (plan, B, doubled) of the last evaluation (block_output, bottleneck_mean)
        self._log_alpha_dev = None          # the log_alpha table on the device (DS_OP_CFG_SIGMA_ROWS), uploaded on first use

    @classmethod
    def from_config(cls, name_or_kwargs, seed=0, device='cuda', step_condition=False, **kw):
        cfg = ldm_arch.NAMED_LDM_CONFIGS[name_or_kwargs] if isinstance(name_or_kwargs, str) else name_or_kwargs
        if step_condition:       # SFD's step-conditioned U-Net: nfe_embed + emb_nfe_layers (LDMUNetSpec.step_condition)
            cfg = dict(cfg, step_condition=True)
        spec = ldm_arch.ldm_unet_spec(**cfg)
        return cls(spec, ldm_arch.init_ldm_params(spec, seed=seed), device, **kw)

    def eval(self):
        return self

    def to(self, *a, **k):
        return self

    def invalidate_context_cache(self):
        """Forget which context the plans' cross-attention K / V buffers hold.  For callers that write conditions through raw pointers
        (no `_version` bump) and for graph.GraphedSampler, whose replays overwrite those buffers behind the cache's back."""
        for P in self.engine._plans.values():
            P.ctx_key = None
            P.ctx_capture_key = None

    # -- evaluation ----------------------------------------------------------------------------------------------------------
    def _step_value(self, step_condition, skip_tuning=False):
        """ops.step_value for this net: the evaluation's step condition as a host float, or None."""
        from . import ops
        return ops.step_value(step_condition, self.spec.step_condition, skip_tuning)

    def raw(self, x, sigma, condition=None, unconditional_condition=None, device_sigma=False, step_condition=None, skip_tuning=False):
        """Runs the plan; returns (F rows NHWC [N*H*W, 4], plan, doubled).
        device_sigma: `sigma` is an fp32 device tensor [B] and stays there -- sigma and c_noise rows of both halves are written by one
        DS_OP_CFG_SIGMA_ROWS launch instead of the host interpolation of ``sigma_inv`` (a D2H copy, CPU math and an H2D copy per evaluation:
        the AMED samplers evaluate at per-sample device sigmas in every step).  Off (the default) keeps the host path and its bits."""
        step = self._step_value(step_condition, skip_tuning)          # (refused before anything touches the device)
        lib = self.engine.lib
        st = _lib.stream_ptr()
        B = x.shape[0]
        doubled = (self.guidance_type == 'classifier-free' and self.guidance_rate != 1. and unconditional_condition is not None)
        if self.guidance_type != 'uncond' and condition is None:
            raise ValueError('CFGDenoiser needs `condition` (text-encoder states [B, L, context_dim])')
        N = 2 * B if doubled else B
        host_scalar = isinstance(sigma, (int, float)) or (isinstance(sigma, torch.Tensor) and sigma.numel() == 1)
        if device_sigma:
            if not (isinstance(sigma, torch.Tensor) and sigma.is_cuda and sigma.dtype == torch.float32 and sigma.numel() == B
                    and sigma.is_contiguous()):
                raise ValueError('device_sigma=True takes a contiguous fp32 device tensor of B sigmas')
            host_scalar = False
        emb_rows = 1 if host_scalar else N
        cond = condition if condition is not None else torch.zeros(B, 1, self.spec.context_dim, device=self.device)
        L = cond.shape[1]
        plan = self.engine.plan(N, emb_rows, L, step is not None)
        bufs = plan.bufs
        if step is not None:
            _lib.check(lib.ds_fill(ptr(bufs['step']), step, 1, st), 'fill step')
        x = x.to(torch.float32).contiguous()
        per = x[0].numel()
        for half in range(2 if doubled else 1):
            _lib.check(lib.ds_copy_rows(ptr(x), per, ptr(bufs['x'][half * B:]), per, B, per, st), 'copy x')
        if device_sigma:
            if self._log_alpha_dev is None:
                self._log_alpha_dev = self.log_alpha_array.to(device=self.device, dtype=torch.float32).contiguous()
            ops.cfg_sigma_rows(sigma, B, self._log_alpha_dev, 2 if doubled else 1, bufs['sigma'], bufs['c_noise'])
        elif host_scalar:
            s = float(sigma)
            cn = float(self.M * self.sigma_inv(torch.tensor(s, dtype=torch.float32)) - 1.)
            _lib.check(lib.ds_fill(ptr(bufs['sigma']), s, 1, st), 'fill sigma')
            _lib.check(lib.ds_fill(ptr(bufs['c_noise']), cn, 1, st), 'fill c_noise')
        else:
            sg = torch.as_tensor(sigma, dtype=torch.float32, device=self.device).reshape(-1)
            cn = (self.M * self.sigma_inv(sg) - 1.).to(torch.float32)
            if doubled:
                sg, cn = torch.cat([sg, sg]), torch.cat([cn, cn])
            bufs['sigma'].copy_(sg)
            bufs['c_noise'].copy_(cn)
        cd = self.spec.context_dim
        parts = [unconditional_condition, cond] if doubled else [cond]
        # context -> plan buffer and its key / value projections: once per context.  The cache key is (weak reference to the caller's
        # tensor, its address, shape and in-place-modification counter): a weak reference, so the cache pins nothing of the caller's, and a
        # dead one never matches.  NEVER skipped while the stream is capturing: a hipGraph must contain the copy and the projections (its
        # replays read whatever the static condition buffers hold THEN), and a capture executes nothing, so afterwards the plan's K / V
        # buffers are not those of `key` either.
        capturing = torch.cuda.is_current_stream_capturing()
        key = tuple((weakref.ref(t), t.data_ptr(), tuple(t.shape), t._version) for t in parts)
        old_key = plan.ctx_key
        same = (self.cache_context and not capturing and old_key is not None and len(old_key) == len(key)
                and all(a[0]() is t and a[1:] == b[1:] for a, b, t in zip(old_key, key, parts)))
        if capturing:
            # inside ONE capture the first evaluation records the context copy and the projections; later evaluations of the same capture
            # on the same condition tensors skip them -- a replay then pays them once per graph, not once per denoiser evaluation.  The key
            # is scoped to the capture: invalidate_context_cache() (graph.GraphedSampler calls it right after capturing and after every
            # replay) clears it, and an eager call never matches it.
            # (round 6) ... and it carries the id of THIS capture (hipStreamGetCaptureInfo): a capture made by someone else's
            # torch.cuda.graph, one aborted by an exception, or two captures in a row on the same static tensors never match each other
            cap_key = ('capture', _lib.capture_id()) + tuple((t.data_ptr(), tuple(t.shape), t._version) for t in parts)
            same = self.cache_context and getattr(plan, 'ctx_capture_key', None) == cap_key
            plan.ctx_capture_key = cap_key
        else:
            plan.ctx_capture_key = None          # an eager evaluation ends every capture scope
        if not same:
            for i, c_ in enumerate(parts):
                c_ = c_.to(device=self.device, dtype=torch.float32)
                if c_.shape[0] == 1 and B > 1:
                    c_ = c_.expand(B, -1, -1)
                c_ = c_.contiguous()
                assert c_.shape == (B, L, cd), (c_.shape, (B, L, cd))
                _lib.check(lib.ds_copy_rows(ptr(c_), cd, ptr(bufs['context'][i * B * L:]), cd, B * L, cd, st), 'copy context')
            plan.ctx.run(st)
            plan.ctx_key = None if capturing else key
        plan.run(st)
        self._last = (plan, B, doubled)
        return bufs['out'], plan, doubled

    def __call__(self, x, sigma, condition=None, unconditional_condition=None, force_fp32=False, device_sigma=False, step_condition=None,
                 skip_tuning=False, **kwargs):
        B, Cc, H, W = x.shape
        f, plan, doubled = self.raw(x, sigma, condition, unconditional_condition, device_sigma=device_sigma, step_condition=step_condition,
                                    skip_tuning=skip_tuning)
        out = torch.empty(B, Cc, H, W, dtype=torch.float32, device=self.device)
        rows = plan.bufs['sigma'].numel()
        ops.cfg_denoise(plan.bufs['x'], f, 4, plan.bufs['sigma'], 1 if rows == 1 else B, self.guidance_rate, doubled, B, Cc, H, W, out)
        return out

    # -- the AMED tap: the reference hooks net.model.model.diffusion_model.middle_block (amed-solver-main/solvers_amed.py:11-12) -----------
    bottleneck_name = 'middle_block.2'

    def tap_shape(self, name=None):
        """(channels, resolution) of block `name`'s output (default: the AMED tap), from the spec: known before any launch."""
        name = self.bottleneck_name if name is None else name
        for b in self.spec.blocks:
            for l in b.layers:
                if l.key == name:
                    return l.cout, l.res_out
        raise KeyError(name)

    def block_output(self, name):
        """Output of layer ``name`` ('middle_block.2', 'input_blocks.1.0', ...) of the LAST evaluation as the NCHW fp32 tensor
        ``[N, C, h, w]`` a forward hook on that module of the reference would see -- all N images: under classifier-free guidance N = 2B,
        unconditional half first (networks_edm.py:687-689).  A copy: the plan's own buffer is overwritten by the next evaluation."""
        plan, B, doubled = self._last
        N = 2 * B if doubled else B
        t = plan.bufs[name].float()          # fp16 residual stream (fp16 mode): widened for the caller
        hw = t.shape[0] // N
        h = int(round(hw ** 0.5))
        assert h * h == hw, (name, tuple(t.shape), N)
        return t.reshape(N, h, h, t.shape[1]).permute(0, 3, 1, 2).contiguous()

    def bottleneck_mean(self, plan, B, doubled):
        """Channel mean of the AMED tap, [B, h, w] fp32 (solvers_amed.py:23-28): of the conditional half -- rows [B h w, 2 B h w) of the
        plan's NHWC buffer -- when the evaluation was doubled, of the whole batch otherwise.  Reads the rows in place, fp32 or fp16."""
        t = plan.bufs[self.bottleneck_name]
        N = 2 * B if doubled else B
        c = t.shape[1]
        hw = t.shape[0] // N
        h = int(round(hw ** 0.5))
        assert h * h == hw and t.shape[0] == N * hw and t.stride(0) == c, (tuple(t.shape), N)
        rows = t[B * hw:] if doubled else t
        out = torch.empty(B, h, h, dtype=torch.float32, device=self.device)
        (ops.channel_mean_f16 if t.dtype == torch.float16 else ops.channel_mean)(rows, c, c, B * hw, out)
        return out
