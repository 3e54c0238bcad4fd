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

The blocks are emitted by plan.Builder (gn_conv3x3, upsample_conv, widen, attention), shared with the latent U-Net.  Workspaces belong to
the plan and are recycled as soon as their last reader is emitted (Builder.alloc / free; launches of a plan are serial): a decode keeps
about three full-resolution tensors alive, not one per layer.
"""
from __future__ import annotations

from typing import Dict

import torch

from . import _lib, vae_arch
from ._lib import DS_ACT_SILU
from .ops import pack_conv_weight, pack_conv_weight_f16, pack_stem_weight
from .plan import Builder, Plan, ptr

KERNEL_ID_F16WIDE = 2575        # ds_conv_kernel_id of csrc/conv3x3_f16wide.hip
EPS = 1e-6                      # model.py:38-39


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
    def plan(self, N: int) -> Plan:
        if N in self._plans:
            return self._plans[N]
        spec, w, lib = self.spec, self.w, self.lib
        bd = Builder(self.device, conv_mode=(1 if self.use_fp16 else 0), w16_cache=self._w16_cache, autotune=False,
                     invariant=self.batch_invariant, batch=N)
        P, new = bd.P, bd.new
        bufs = P.bufs
        R, RO = spec.latent_resolution, spec.img_resolution
        zc = spec.z_channels
        bufs['x'] = new(N, zc + 1, R, R, zero=True)
        bufs['x'][:, zc] = 1.0                       # the ones plane (see _pack); written once, the latents go to planes [0, zc)
        bufs['one'] = new(1, zero=True)              # ds_stem_im2col scales by 1 / sqrt(sigma^2 + sigma_data^2): sigma 0, sigma_data 1
        bufs['out'] = new(N, spec.out_ch, RO, RO)
        bd.coefs = new(N * 3 * max(max(l.cin, l.cout) for l in spec.layers))
        layers = spec.layers
        # This decoder's own rule, on top of Builder.f16_conv_ok: in the invariant mode its 8 x 8 layers (images that do not fill a 256-pixel
        # tile) stay on the fp32 kernels.  The denoisers run such layers on the fp16-activation kernels in that mode too.
        fp32_only = lambda side: self.batch_invariant and (side * side) % 256

        def fp32_rows(t, c, side, name):
            """`t` as fp32 rows: an fp16 tensor is widened and recycled."""
            wide = bd.widen(t, c, N, side, name)
            if wide is not t:
                bd.free(t)
            return wide

        def res_layer(l, x, out_f32):
            p, side, cin, cout = l.key, l.res_out, l.cin, l.cout
            M = N * side * side
            f16 = bool(not fp32_only(side) and bd.f16_conv_ok(N, side, cin, 0, cout, wide=True) and bd.f16_conv_ok(N, side, cout, 0, cout, wide=True))
            if not f16:
                x = fp32_rows(x, cin, side, p + '.x')
            h1 = bd.alloc(M, cout, f16=f16)
            bd.gn_conv3x3(x, cin, None, 0, N, side, w[f'{p}.n1.g'], w[f'{p}.n1.b'], w[f'{p}.c1.w'], w[f'{p}.c1.b'], cout, h1, cout, p + '.conv1',
                          eps=EPS, w16=w.get(f'{p}.c1.w16') if f16 else None, f16=f16)
            short = x
            if cin != cout:         # nin_shortcut (model.py:135-139): a 1x1 convolution of the raw input, added by conv2's epilogue
                s16 = f16 and x.dtype == torch.float16 and bd.gemm16_ok(M, cin, cout)
                if f16 and x.dtype == torch.float16 and not s16:
                    raise NotImplementedError(f'{p}.nin_shortcut: no fp16-activation GEMM for {M} x {cin} -> {cout}')
                short = bd.alloc(M, cout, f16=s16)
                bd.conv(x, cin, cin, N, side, side, w[f'{p}.nin.w'], cout, short, cout, 1, p + '.nin_shortcut', bias=w[f'{p}.nin.b'])
                bd.free(x)
            out = bd.alloc(M, cout, f16=(f16 and not out_f32))
            bd.gn_conv3x3(h1, cout, None, 0, N, side, w[f'{p}.n2.g'], w[f'{p}.n2.b'], w[f'{p}.c2.w'], w[f'{p}.c2.b'], cout, out, cout, p + '.conv2',
                          eps=EPS, w16=w.get(f'{p}.c2.w16') if f16 else None, f16=f16, res=short, res_ld=cout)
            bd.free(h1, short)
            return out

        def attn_layer(l, x):
            p, side, c = l.key, l.res_out, l.cin
            S = side * side
            M = N * S
            if not lib.ds_attention_supported(c):
                raise NotImplementedError(f'attention head size {c} has no kernel instantiation')
            x = fp32_rows(x, c, side, p + '.x')
            h16 = bd.gemm16_ok(M, c, 3 * c)
            n = bd.alloc(M, c, f16=h16)
            bd.norm('stats', x, c, c, N, side, side, p + '.norm.stats', groups=32, eps=EPS)
            bd.norm('apply', x, c, c, N, side, side, p + '.norm', groups=32, eps=EPS, gamma=w[f'{p}.n.g'], beta=w[f'{p}.n.b'], out=n, out_ld=c,
                    out_f16=h16)
            qkv = bd.alloc(M, 3 * c)
            bd.conv(n, c, c, N, side, side, w[f'{p}.qkv.w'], 3 * c, qkv, 3 * c, 1, p + '.qkv', bias=w[f'{p}.qkv.b'])
            bd.free(n)
            ao = bd.alloc(M, c)
            bd.attention(qkv, qkv[:, c:], qkv[:, 2 * c:], ao, p + '.attention', batch=N, heads=1, sq=S, skv=S, d=c, ldq=3 * c, ldk=3 * c,
                         ldv=3 * c, ldo=c, q_bs=S * 3 * c, k_bs=S * 3 * c, v_bs=S * 3 * c, o_bs=S * c, scale=float(c) ** -0.5)
            bd.free(qkv)
            out = bd.alloc(M, c)
            bd.conv(ao, c, c, N, side, side, w[f'{p}.po.w'], c, out, c, 1, p + '.proj_out', bias=w[f'{p}.po.b'], res=x, res_ld=c, stats=True)
            bd.free(ao, x)
            return out

        cur = None
        for i, l in enumerate(layers):
            p = l.key
            nxt = layers[i + 1].kind if i + 1 < len(layers) else None
            out_f32 = nxt in ('attn', 'conv_out')            # their kernels read fp32 rows
            if l.kind == 'conv_in':
                col = bd.alloc(N * R * R, 64)
                bd.add(lib.ds_stem_im2col, (ptr(bufs['x']), ptr(bufs['one']), 1, 1.0, N, zc + 1, R, R, ptr(col), 64), 'post_quant_conv.im2col')
                cur = bd.alloc(N * R * R, l.cout)
                bd.conv(col, 64, 64, N, R, R, w[f'{p}.w'], l.cout, cur, l.cout, 1, p, bias=w[f'{p}.b'], stats=True)
                bd.free(col)
            elif l.kind == 'res':
                cur = res_layer(l, cur, out_f32)
            elif l.kind == 'attn':
                cur = attn_layer(l, cur)
            elif l.kind == 'up':            # nearest x2 of the raw tensor (model.py:54) -> 3x3 conv
                cur = bd.upsample_conv(cur, l.cin, N, l.res_in, w[f'{p}.w'], w[f'{p}.b'], l.cout, p,
                                       w16=None if fp32_only(l.res_out) else w.get(f'{p}.w16'), wide=True, out_f32=out_f32, free_src=True)
            elif l.kind == 'conv_out':
                side = l.res_out
                cur = fp32_rows(cur, l.cin, side, p + '.x')
                bd.norm('stats', cur, l.cin, l.cin, N, side, side, 'decoder.norm_out.stats', groups=32, eps=EPS, gamma=w['out.g'],
                        beta=w['out.b'], coefs=bd.coefs)
                bd.conv(cur, l.cin, l.cin, N, side, side, w[f'{p}.w'], l.cout, bufs['out'], 4, 9, p, bias=w[f'{p}.b'], norm_coefs=bd.coefs,
                        norm_act=DS_ACT_SILU, out_nchw=1)
                bd.free(cur)
        self._plans[N] = bd.finish()
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
