"""``AutoencoderKL`` decoder on the HIP engine: what the reference's batch loop runs after the sampler for a latent-diffusion model,
``images = net.model.decode_first_stage(images)`` (diff-solvers-main/sample.py:299; ddpm.py:706-734; autoencoder.py:330-332;
ldm/modules/diffusionmodules/model.py:535-568) -- SD-1.5 latents [B, 4, 64, 64] -> images [B, 3, 512, 512].

One decode = one flat plan of libdsamd launches over NHWC workspaces (``vae_arch.VAEDecoderSpec`` is the data model):

    z / scale_factor, post_quant_conv, conv_in   ONE GEMM: ds_stem_im2col of [z | 1] (K = 9 x 5 -> 64) times the composed weight
                        W_in[tap] . W_pq / scale_factor; the ones plane carries post_quant_conv's bias through conv_in's zero padding
                        exactly (a border pixel sees the bias only under the taps that lie inside the image)
    ResnetBlock         GN statistics (from the producer's epilogue column sums where it left them) -> GroupNorm + swish pass -> 3x3 conv
                        -> the same again -> 3x3 conv (+ residual); nin_shortcut = a 1x1 convolution whose output is that residual
    AttnBlock           GroupNorm pass -> q | k | v as one 1x1 projection -> fused attention, ONE head of C channels (C = 512: the
                        channel-split block of csrc/attention.hip) -> 1x1 proj_out (+ residual)
    Upsample            nearest x2 pass -> 3x3 conv
    norm_out, swish, conv_out   one launch of the thin head kernel (csrc/conv3x3_thin.hip), writing planar NCHW

use_fp16 (the reference decodes inside the sampler's ``autocast`` block): every 3x3 convolution whose channel counts are multiples of 64
runs on the fp16-activation matrix kernels -- csrc/conv3x3_f16dma.hip up to 64 pixels wide, csrc/conv3x3_f16wide.hip (4 x 64 patches,
kernel id 2575) above -- and the tensors between them are fp16 rows; GroupNorm statistics, softmax and every accumulation are fp32.
The tensors around the mid-block attention and the input of the head stay fp32 rows (their consumers read fp32).  use_fp16=False: fp32
everywhere; above 64 pixels wide that is the generic gather kernel.

Workspaces belong to the plan and are recycled as soon as their last reader is emitted (launches of a plan are serial): a decode keeps
about three full-resolution tensors alive, not one per layer.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict

import torch

from . import _lib, vae_arch
from ._lib import DS_ACT_SILU, DS_RESAMPLE_UP
from .ops import pack_conv_weight, pack_conv_weight_f16, pack_stem_weight
from .plan import Builder, Plan, ptr

KERNEL_ID_F16WIDE = 2575        # ds_conv_kernel_id of csrc/conv3x3_f16wide.hip
EPS = 1e-6                      # model.py:38-39


class _Pool:
    """Workspace recycling on top of plan.Builder: alloc() hands out a freed buffer of the same dtype that is large enough (the smallest
    such), else a new plan-owned tensor; free() makes a buffer available to LATER launches."""

    def __init__(self, bd: Builder):
        self.bd = bd
        self.free_list = []     # base tensors (1-D)
        self.base = {}          # data_ptr of a view -> its base tensor

    def alloc(self, rows, cols, f16=False):
        dt = torch.float16 if f16 else torch.float32
        n = rows * cols
        fit = [t for t in self.free_list if t.dtype == dt and t.numel() >= n]
        if fit:
            b = min(fit, key=lambda t: t.numel())
            self.free_list = [t for t in self.free_list if t is not b]
        else:
            b = (self.bd.new16 if f16 else self.bd.new)(n)
        v = b[:n].view(rows, cols)
        self.base[v.data_ptr()] = b
        return v

    def free(self, *views):
        for v in views:
            if v is None:
                continue
            b = self.base.pop(v.data_ptr(), None)
            if b is not None:
                self.bd.stats_of.pop(v.data_ptr(), None)       # column sums of a recycled tensor describe nothing
                self.free_list.append(b)


class VAEDecoder:
    """``VAEDecoder(z) -> [B, 3, 8 R, 8 R]`` fp32 NCHW for latents ``z`` [B, 4, R, R] (R = spec.latent_resolution): the reference's
    ``decode_first_stage`` (z / scale_factor -> post_quant_conv -> Decoder)."""

    def __init__(self, spec: vae_arch.VAEDecoderSpec, params: Dict[str, torch.Tensor], device='cuda', use_fp16=False, batch_invariant=False):
        """batch_invariant: every launch carries ds_conv_tune.invariant: same latent, same bits at any batch."""
        self.spec = spec
        self.device = torch.device(device)
        self.use_fp16 = bool(use_fp16)
        self.batch_invariant = bool(batch_invariant)
        self.lib = _lib.load()
        self._w16_cache = {}
        self._plans: Dict[int, Plan] = {}
        self._pack(params)

    @classmethod
    def from_config(cls, name_or_kwargs='sd15', seed=0, device='cuda', **kw):
        cfg = vae_arch.NAMED_VAE_CONFIGS[name_or_kwargs] if isinstance(name_or_kwargs, str) else name_or_kwargs
        spec = vae_arch.vae_decoder_spec(**cfg)
        return cls(spec, vae_arch.init_vae_params(spec, seed=seed), device, **kw)

    @classmethod
    def from_state_dict(cls, state_dict, name_or_kwargs='sd15', device='cuda', **kw):
        """From a checkpoint's state_dict (``first_stage_model.decoder.*`` / ``first_stage_model.post_quant_conv.*``, with or without the
        ``first_stage_model.`` prefix)."""
        cfg = vae_arch.NAMED_VAE_CONFIGS[name_or_kwargs] if isinstance(name_or_kwargs, str) else name_or_kwargs
        spec = vae_arch.vae_decoder_spec(**cfg)
        return cls(spec, vae_arch.vae_params_from_state_dict(spec, state_dict), device, **kw)

    # ------------------------------------------------------------------------------------------ weights
    def _pack(self, params):
        spec, dev = self.spec, self.device
        g = lambda k: params[k].detach().to(device=dev, dtype=torch.float32).contiguous()
        w: Dict[str, torch.Tensor] = {}

        def conv3(dst, src, cin, cout):
            w[f'{dst}.w'], w[f'{dst}.b'] = pack_conv_weight(g(f'{src}.weight')), g(f'{src}.bias')
            if self.use_fp16 and cin % 64 == 0 and cout % 64 == 0:
                w[f'{dst}.w16'] = (pack_conv_weight_f16(g(f'{src}.weight')), 0)

        for l in spec.layers:
            p = l.key
            if l.kind == 'conv_in':
                # conv_in(pad(post_quant_conv(z / s))) as one matrix over the im2col of [z | 1]: column (tap, c < 4) = W_in[tap] W_pq[:, c] / s,
                # column (tap, 4) = W_in[tap] b_pq.  Composed in fp64 on the host, once.
                wi = params[f'{p}.weight'].detach().double().cpu()                              # [cout, zc, 3, 3]
                wq = params['post_quant_conv.weight'].detach().double().cpu()[:, :, 0, 0]       # [zc, embed]
                bq = params['post_quant_conv.bias'].detach().double().cpu()
                comp = torch.einsum('omyx,mc->ocyx', wi, wq) / spec.scale_factor
                ones = torch.einsum('omyx,m->oyx', wi, bq)[:, None]
                w[f'{p}.w'] = pack_stem_weight(torch.cat([comp, ones], 1).to(torch.float32).to(dev), k_pad=64)
                w[f'{p}.b'] = g(f'{p}.bias')
            elif l.kind == 'res':
                for n_, src in (('n1', 'norm1'), ('n2', 'norm2')):
                    w[f'{p}.{n_}.g'], w[f'{p}.{n_}.b'] = g(f'{p}.{src}.weight'), g(f'{p}.{src}.bias')
                conv3(f'{p}.c1', f'{p}.conv1', l.cin, l.cout)
                conv3(f'{p}.c2', f'{p}.conv2', l.cout, l.cout)
                if l.cin != l.cout:
                    w[f'{p}.nin.w'], w[f'{p}.nin.b'] = pack_conv_weight(g(f'{p}.nin_shortcut.weight')), g(f'{p}.nin_shortcut.bias')
            elif l.kind == 'attn':
                w[f'{p}.n.g'], w[f'{p}.n.b'] = g(f'{p}.norm.weight'), g(f'{p}.norm.bias')
                w[f'{p}.qkv.w'] = pack_conv_weight(torch.cat([g(f'{p}.{x}.weight') for x in 'qkv'], 0))
                w[f'{p}.qkv.b'] = torch.cat([g(f'{p}.{x}.bias') for x in 'qkv'], 0).contiguous()
                w[f'{p}.po.w'], w[f'{p}.po.b'] = pack_conv_weight(g(f'{p}.proj_out.weight')), g(f'{p}.proj_out.bias')
            elif l.kind == 'up':
                conv3(p, f'{p}.conv', l.cin, l.cout)
            elif l.kind == 'conv_out':
                w['out.g'], w['out.b'] = g('decoder.norm_out.weight'), g('decoder.norm_out.bias')
                w[f'{p}.w'], w[f'{p}.b'] = pack_conv_weight(g(f'{p}.weight')), g(f'{p}.bias')
        self.w = w

    # ------------------------------------------------------------------------------------------ plan
    def _f16_conv_ok(self, N, side, cin, cout):
        """Does this 3x3 layer run on an fp16-activation kernel (use_fp16 only)?  Up to 64 pixels wide: conv3x3_f16dma's own rule; above:
        the patch kernel's (power-of-two sides, whole 64-channel slabs and column tiles)."""
        if not self.use_fp16 or cin % 64 or cout % 64:
            return False
        if side > 64:
            return side & (side - 1) == 0
        if self.batch_invariant and (side * side) % 256:
            return False            # 8 x 8 images: whole 256-pixel tiles only at batches that are multiples of four (plan.Builder.f16_level)
        return bool(self.lib.ds_conv_f16dma_supported(N, side, side, cin, 0, cout))

    def plan(self, N: int) -> Plan:
        if N in self._plans:
            return self._plans[N]
        spec, w, lib = self.spec, self.w, self.lib
        bd = Builder(self.device, conv_mode=(1 if self.use_fp16 else 0), w16_cache=self._w16_cache, autotune=False,
                     invariant=self.batch_invariant, batch=N)
        P, new = bd.P, bd.new
        pool = _Pool(bd)
        bufs = P.bufs
        R, RO = spec.latent_resolution, spec.img_resolution
        zc = spec.z_channels
        bufs['x'] = new(N, zc + 1, R, R, zero=True)
        bufs['x'][:, zc] = 1.0                       # the ones plane (see _pack); written once, the latents go to planes [0, zc)
        bufs['one'] = new(1, zero=True)              # ds_stem_im2col scales by 1 / sqrt(sigma^2 + sigma_data^2): sigma 0, sigma_data 1
        bufs['out'] = new(N, spec.out_ch, RO, RO)
        cmax = max(max(l.cin, l.cout) for l in spec.layers)
        ncoef = new(N * 3 * cmax)
        layers = spec.layers

        def widen(t, c, side, name):
            if t.dtype != torch.float16:
                return t
            wide = pool.alloc(N * side * side, c)
            bd.norm('apply', t, c, c, N, side, side, name + '.widen', use_stats=False, out=wide, out_ld=c)
            pool.free(t)
            return wide

        def gn_conv(x, cin, side, gk, bk, wkey, cout, out, name, f16, res=None):
            """GroupNorm(32) + swish + 3x3 conv (+ residual).  f16: the pass writes the activated tensor as fp16 rows and the convolution is an
            fp16-activation matrix kernel; else fp32, the normalisation fused into the LDS-halo kernel's loader where that kernel exists."""
            M = N * side * side
            kw = dict(bias=w[f'{wkey}.b'], stats=True)
            if res is not None:
                kw.update(res=res, res_ld=cout)
            if f16:
                bd.norm('stats', x, cin, cin, N, side, side, name + '.gn.stats', groups=32, eps=EPS, gamma=gk, beta=bk, coefs=ncoef)
                a16 = pool.alloc(M, cin, f16=True)
                bd.norm('apply', x, cin, cin, N, side, side, name + '.gn', groups=32, eps=EPS, use_stats=False, act=DS_ACT_SILU, out=a16,
                        out_ld=cin, out_f16=True, coefs=ncoef, in_f16=(x.dtype == torch.float16))
                bd.conv(a16, cin, cin, N, side, side, w[f'{wkey}.w'], cout, out, cout, 9, name, w16=w[f'{wkey}.w16'], in_f16=True,
                        out_f16=(out.dtype == torch.float16), **kw)
                pool.free(a16)
            elif lib.ds_conv3x3_halo_supported(side, side):
                bd.norm('stats', x, cin, cin, N, side, side, name + '.gn.stats', groups=32, eps=EPS, gamma=gk, beta=bk, coefs=ncoef)
                bd.conv(x, cin, cin, N, side, side, w[f'{wkey}.w'], cout, out, cout, 9, name, norm_coefs=ncoef, norm_act=DS_ACT_SILU, **kw)
            else:
                tmp = pool.alloc(M, cin)
                bd.norm('stats', x, cin, cin, N, side, side, name + '.gn.stats', groups=32, eps=EPS)
                bd.norm('apply', x, cin, cin, N, side, side, name + '.gn', groups=32, eps=EPS, gamma=gk, beta=bk, act=DS_ACT_SILU,
                        out=tmp, out_ld=cin)
                bd.conv(tmp, cin, cin, N, side, side, w[f'{wkey}.w'], cout, out, cout, 9, name, **kw)
                pool.free(tmp)

        def res_layer(l, x, out_f32):
            p, side, cin, cout = l.key, l.res_out, l.cin, l.cout
            M = N * side * side
            f16 = self._f16_conv_ok(N, side, cin, cout) and self._f16_conv_ok(N, side, cout, cout)
            if not f16:
                x = widen(x, cin, side, p + '.x')
            h1 = pool.alloc(M, cout, f16=f16)
            gn_conv(x, cin, side, w[f'{p}.n1.g'], w[f'{p}.n1.b'], f'{p}.c1', cout, h1, p + '.conv1', f16)
            short = x
            if cin != cout:         # nin_shortcut (model.py:135-139): a 1x1 convolution of the raw input, added by conv2's epilogue
                s16 = f16 and x.dtype == torch.float16 and bool(lib.ds_gemm_f16dma_supported(M, cin, cout))
                if f16 and x.dtype == torch.float16 and not s16:
                    raise NotImplementedError(f'{p}.nin_shortcut: no fp16-activation GEMM for {M} x {cin} -> {cout}')
                short = pool.alloc(M, cout, f16=s16)
                bd.conv(x, cin, cin, N, side, side, w[f'{p}.nin.w'], cout, short, cout, 1, p + '.nin_shortcut', bias=w[f'{p}.nin.b'])
                pool.free(x)
            out = pool.alloc(M, cout, f16=(f16 and not out_f32))
            gn_conv(h1, cout, side, w[f'{p}.n2.g'], w[f'{p}.n2.b'], f'{p}.c2', cout, out, p + '.conv2', f16, res=short)
            pool.free(h1, short)
            return out

        def attn_layer(l, x):
            p, side, c = l.key, l.res_out, l.cin
            S = side * side
            M = N * S
            if not lib.ds_attention_supported(c):
                raise NotImplementedError(f'attention head size {c} has no kernel instantiation')
            x = widen(x, c, side, p + '.x')
            h16 = bool(self.use_fp16 and lib.ds_gemm_f16dma_supported(M, c, 3 * c))
            n = pool.alloc(M, c, f16=h16)
            bd.norm('stats', x, c, c, N, side, side, p + '.norm.stats', groups=32, eps=EPS)
            bd.norm('apply', x, c, c, N, side, side, p + '.norm', groups=32, eps=EPS, gamma=w[f'{p}.n.g'], beta=w[f'{p}.n.b'], out=n, out_ld=c,
                    out_f16=h16)
            qkv = pool.alloc(M, 3 * c)
            bd.conv(n, c, c, N, side, side, w[f'{p}.qkv.w'], 3 * c, qkv, 3 * c, 1, p + '.qkv', bias=w[f'{p}.qkv.b'])
            pool.free(n)
            ao = pool.alloc(M, c)
            bd.attention(qkv, qkv[:, c:], qkv[:, 2 * c:], ao, p + '.attention', batch=N, heads=1, sq=S, skv=S, d=c, ldq=3 * c, ldk=3 * c,
                         ldv=3 * c, ldo=c, q_bs=S * 3 * c, k_bs=S * 3 * c, v_bs=S * 3 * c, o_bs=S * c, scale=float(c) ** -0.5)
            pool.free(qkv)
            out = pool.alloc(M, c)
            bd.conv(ao, c, c, N, side, side, w[f'{p}.po.w'], c, out, c, 1, p + '.proj_out', bias=w[f'{p}.po.b'], res=x, res_ld=c, stats=True)
            pool.free(ao, x)
            return out

        cur = None
        for i, l in enumerate(layers):
            p = l.key
            nxt = layers[i + 1].kind if i + 1 < len(layers) else None
            out_f32 = nxt in ('attn', 'conv_out')            # their kernels read fp32 rows
            if l.kind == 'conv_in':
                col = pool.alloc(N * R * R, 64)
                bd.add(lib.ds_stem_im2col, (ptr(bufs['x']), ptr(bufs['one']), 1, 1.0, N, zc + 1, R, R, ptr(col), 64), 'post_quant_conv.im2col')
                cur = pool.alloc(N * R * R, l.cout)
                bd.conv(col, 64, 64, N, R, R, w[f'{p}.w'], l.cout, cur, l.cout, 1, p, bias=w[f'{p}.b'], stats=True)
                pool.free(col)
            elif l.kind == 'res':
                cur = res_layer(l, cur, out_f32)
            elif l.kind == 'attn':
                cur = attn_layer(l, cur)
            elif l.kind == 'up':
                side, M = l.res_out, N * l.res_out ** 2
                f16 = self._f16_conv_ok(N, side, l.cin, l.cout)
                up = pool.alloc(M, l.cin, f16=f16)          # nearest x2 of the raw tensor (model.py:54)
                bd.norm('apply', cur, l.cin, l.cin, N, l.res_in, l.res_in, p + '.nearest', use_stats=False, resample=DS_RESAMPLE_UP,
                        out=up, out_ld=l.cin, out_f16=f16)
                pool.free(cur)
                cur = pool.alloc(M, l.cout, f16=(f16 and not out_f32))
                bd.conv(up, l.cin, l.cin, N, side, side, w[f'{p}.w'], l.cout, cur, l.cout, 9, p + '.conv', bias=w[f'{p}.b'], stats=True,
                        **(dict(w16=w[f'{p}.w16'], in_f16=True) if f16 else {}))
                pool.free(up)
            elif l.kind == 'conv_out':
                side = l.res_out
                cur = widen(cur, l.cin, side, p + '.x')
                bd.norm('stats', cur, l.cin, l.cin, N, side, side, 'decoder.norm_out.stats', groups=32, eps=EPS, gamma=w['out.g'],
                        beta=w['out.b'], coefs=ncoef)
                bd.conv(cur, l.cin, l.cin, N, side, side, w[f'{p}.w'], l.cout, bufs['out'], 4, 9, p, bias=w[f'{p}.b'], norm_coefs=ncoef,
                        norm_act=DS_ACT_SILU, out_nchw=1)
                pool.free(cur)
        # a missing kernel is an error at plan time, not at the first decode
        P.kernel_ids = {}
        for op in P.ops:
            if op.fn is lib.ds_conv2d_nhwc:
                kid = lib.ds_conv_kernel_id(C.byref(op.keep[0]))
                if kid < 0:
                    _lib.check(kid, f'VAEDecoder plan: no kernel for {op.name}')
                P.kernel_ids[op.name] = kid
        self._plans[N] = P
        return P

    # ------------------------------------------------------------------------------------------ evaluation
    def flops(self, n_images=1):
        """Algorithmic FLOPs (2 x MAC) of decoding n_images latents."""
        return vae_arch.vae_flops_per_image(self.spec) * n_images

    def raw(self, z):
        """Copies the latents into the plan and runs it; returns (the plan's output buffer [B, 3, H, W], plan)."""
        spec = self.spec
        B = z.shape[0]
        R = spec.latent_resolution
        if tuple(z.shape[1:]) != (spec.z_channels, R, R):
            raise ValueError(f'VAEDecoder was built for latents [B, {spec.z_channels}, {R}, {R}], got {tuple(z.shape)}')
        plan = self.plan(B)
        st = _lib.stream_ptr()
        z = z.to(device=self.device, dtype=torch.float32).contiguous()
        per = spec.z_channels * R * R
        _lib.check(self.lib.ds_copy_rows(ptr(z), per, ptr(plan.bufs['x']), per + R * R, B, per, st), 'copy z')
        plan.run(st)
        return plan.bufs['out'], plan

    def __call__(self, z):
        out, _ = self.raw(z)
        return out.clone()
