"""Denoiser engine: compiles a ``UNetSpec`` + reference-keyed weights into a flat launch plan of libdsamd kernels.

What it replaces: ``EDMPrecond.forward`` -> ``SongUNet/DhariwalUNet.forward`` -> ``UNetBlock.forward``
(diff-solvers-main/models/networks_edm.py:482-496, :312-355, :427-453, :158-179), i.e. the ~600 ATen launches per
network evaluation of the reference, by ~10 hand-written launches per block:

    GN stats -> normalise+SiLU(+resample) -> 3x3 implicit GEMM (+bias +emb) -> GN stats -> normalise+SiLU
      -> 3x3 implicit GEMM (+bias +skip +scale)   [+ attention: GN, packed 1x1 q|k|v, fused softmax(QK^T)V kernel, 1x1 proj]

Activations are NHWC fp32 and live in engine-owned workspaces (allocated once per batch size through torch, which
is only the allocator here); the decoder's ``torch.cat`` is never materialised (both sources are read in place).
``UNetEngine.plan`` is a short driver: embedding path, then per block ``_block16`` (fp16-activation kernels) or ``_block32`` (fp32 routes)
up to conv1's arguments, conv1, ``_attention``, and ``_head``; the launches are marshalled by ``plan.Builder``, scratch is preallocated once
per plan (``_workspaces``).  The plan is a list of (C function, prebuilt argument struct): running it is a tight ctypes loop, and because no
pointer changes between calls it can be captured in a hipGraph (see ``graph.py``).

``EDMDenoiser`` is the drop-in for the reference ``net`` object: same call signature and attributes
(``img_resolution, img_channels, label_dim, sigma_min, sigma_max``) plus the raw fast path the fused solvers use.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from types import SimpleNamespace
from typing import Dict

import numpy as np
import torch

from . import _lib, arch
from ._lib import DS_ACT_SILU, DS_RESAMPLE_NONE, DS_RESAMPLE_DOWN, DS_RESAMPLE_UP
from .ops import pack_conv_weight, pack_conv_weight_f16, pack_conv_weight_split, pack_conv_weight_up2, pack_conv_weight_wino, pack_linear_weight, pack_stem_weight
from .plan import FUSE_NORM16_DEFAULT, Builder, Plan as _Plan, fuse_norm16_here, fuse_norm16_value, ptr as _ptr


class UNetEngine:
    def __init__(self, spec: arch.UNetSpec, params: Dict[str, torch.Tensor], device='cuda', use_fp16=False, split_fp16=False,
                 batch_invariant=False, up_phase=True, winograd=True, wide16=True):
        """wide16 (fp16 mode only): blocks whose output is wider than 64 pixels run their 3x3 convolutions on fp16 rows too, on the patch kernel
        (csrc/conv3x3_f16wide.hip, kernel ids 2575 / 2576) -- with them the whole plan of a 256-pixel net keeps the fp16 stream.  False: such
        blocks keep the fp32 routes (A/B runs).  No named EDM config has a layer above 64 pixels: their plans are the same either way.
        winograd (exact fp32 mode only, never with batch_invariant): the stride-1 3x3 layers the library would run on its 256 x 256 tiles
        run in the Winograd form F(2x2, 3x3) instead (ds_conv_args.wino, csrc/conv3x3_wino.hip: 2.25 x fewer fp32 multiply-adds, weights
        transformed once per build; the same launches, the same kernel ids) wherever the library takes the layer; layers it refuses -- and
        every layer with False -- are emitted as the direct form, bit for bit.  Results differ from the direct form in rounding only (~1e-6
        of a layer's output absmax; the per-evaluation bound of DESIGN.md section 2 is unchanged).
        up_phase (exact fp32 mode only): conv0 of an up block, conv3x3(nearest_x2(silu(norm0(x)))), runs on the LOW-RES activated tensor as
        four 2x2 phase convolutions with weights folded at load time (ds_conv_args.in_up2: 4 taps per output pixel instead of 9, and the
        upsampled tensor is never written) wherever the library takes the layer; False = the upsampling pass and the 9-tap convolution
        (A/B runs, tests/test_hip_upconv.py).
        batch_invariant: every plan takes the batch-invariant route: an image's output bits depend on its own
        inputs, the weights and the mode only -- not on the batch size, the other images or the sigma form.
        split_fp16: fp32 EMULATED on the fp16 matrix pipe in the 3x3 convolutions -- every operand as fp16 hi + lo, three MFMA
        products per multiplication, fp32 accumulation (ds_conv_args.wgt_f16 == 2); 2**-22 relative per product, i.e. inside every
        fp32 tolerance of this engine, at 16/3 of the fp32 matrix rate.  Not a reduced-precision mode: it is tested against the same
        fp32 goldens and tolerances as the exact fp32 path.
        use_fp16: the reference's reduced-precision mode (networks_edm.py:486: the U-Net body on x.to(float16)).  3x3 convolutions,
        1x1 / Linear layers over image rows and attention multiply fp16 operands on the fp16 matrix pipe with fp32 accumulation, and the
        activations between layers -- the activated GroupNorm outputs, conv0 outputs, the residual stream and the skip stack -- are
        stored in fp16 where the fp16-activation kernels take the geometry (plan(): `stream16`); GroupNorm / SiLU / softmax arithmetic,
        q / k / v and the embedding path are fp32.  DESIGN.md section 2 states the bounds, tests/test_hip_fp16.py enforces them."""
        self.spec = spec
        self.device = torch.device(device)
        if spec.ncsnpp and (use_fp16 or split_fp16 or batch_invariant):
            # the FIR resampler and the aux-residual pyramid (csrc/metrics/fir_resample.hip) are fp32 launches outside libdsamd: no fp16
            # storage form, no split-fp16 convolution and no batch-invariant route is defined for them
            raise NotImplementedError('NCSN++ options (fourier embedding / residual encoder / [1,3,3,1] filter) run in the exact fp32 mode only: '
                                      'use_fp16, split_fp16 and batch_invariant are not supported with them')
        self.fir = tuple(spec.resample_filter) != (1, 1)      # up / down blocks resample through dsm_fir_resample, not ds_norm_act
        self.use_fp16 = bool(use_fp16)
        self.split_fp16 = bool(split_fp16) and not self.use_fp16
        self.batch_invariant = bool(batch_invariant)
        self.up_phase = bool(up_phase) and not self.use_fp16 and not self.split_fp16
        self.winograd = bool(winograd) and not self.use_fp16 and not self.split_fp16 and not self.batch_invariant
        self.wide16 = bool(wide16) and self.use_fp16
        # CM nets: the output of middle_block (the spec's dec.RxR_in1) is the AMED tap: it gets a buffer of its own instead of a turn in the
        # decoder's ping-pong pair, so that it outlives the evaluation like the encoder outputs the EDM nets tap
        self.tap_block = next((b.name for b in spec.blocks if b.name.startswith('dec.') and b.name.endswith('_in1')), None) if spec.cm_noise else None
        # fp16 mode: GroupNorm apply + SiLU inside the fp16-activation convolution's LDS halo instead of a ds_norm_act pass (plan(): fz0 / fz1;
        # bit-identical results).  An attribute, not an argument, so that A/B runs flip it per engine: DS_FUSE_NORM16 sets the default.
        self.fuse_norm16 = fuse_norm16_value(os.environ.get('DS_FUSE_NORM16', FUSE_NORM16_DEFAULT))
        self._w16_cache = {}
        self.conv_mode = 1 if self.use_fp16 else (2 if self.split_fp16 else 0)      # ds_conv_args.wgt_f16 of the eligible 3x3 layers
        self.lib = _lib.load()
        self._plans: Dict[tuple, _Plan] = {}
        self._pack(params)

    # ------------------------------------------------------------------------------------------ weights
    def _pack(self, params):
        spec, dev = self.spec, self.device
        g = lambda k: params[k].detach().to(device=dev, dtype=torch.float32)
        w: Dict[str, torch.Tensor] = {}
        m = 'model'
        song = spec.model_type == 'SongUNet'
        # embedding MLP
        half = spec.noise_channels // 2
        freqs = torch.arange(0, half, dtype=torch.float32)
        freqs = freqs / (half - (1 if spec.pos_endpoint else 0))
        freqs = (1 / spec.pos_max_positions) ** freqs            # exactly networks_edm.py:193-195, on the host
        if spec.cm_noise:                                        # timestep_embedding of the CM nets (models/cm/nn.py): the same numbers in its own rounding
            freqs = torch.exp(-math.log(spec.pos_max_positions) * torch.arange(0, half, dtype=torch.float32) / half)
        if spec.embedding_type == 'fourier':                     # FourierEmbedding: the reference's own expression on its fp32 buffer (networks_edm.py:210)
            freqs = (2 * np.pi * params[f'{m}.map_noise.freqs'].detach().to(device='cpu', dtype=torch.float32)).to(torch.float32)
            assert freqs.shape == (half,), (tuple(freqs.shape), half)
        w['freqs'] = freqs.contiguous().to(dev)
        w['map0.w'] = pack_linear_weight(g(f'{m}.map_layer0.weight')); w['map0.b'] = g(f'{m}.map_layer0.bias')
        w['map1.w'] = pack_linear_weight(g(f'{m}.map_layer1.weight')); w['map1.b'] = g(f'{m}.map_layer1.bias')
        if spec.label_dim:
            wl = g(f'{m}.map_label.weight')
            if song:
                wl = wl * math.sqrt(spec.label_dim)              # class_labels * sqrt(in_features), networks_edm.py:320
            w['label.w'] = pack_linear_weight(wl)
            w['label.b'] = g(f'{m}.map_label.bias') if f'{m}.map_label.bias' in params else None
        # per-block affine layers, concatenated into one GEMM
        aff_w, aff_b, off = [], [], 0
        self.aff_off: Dict[str, int] = {}
        for b in spec.blocks:
            if b.kind != 'block':
                continue
            p = f'{m}.{b.name}'
            aff_w.append(g(f'{p}.affine.weight')); aff_b.append(g(f'{p}.affine.bias'))
            self.aff_off[b.name] = off
            off += aff_w[-1].shape[0]
        self.aff_total = off
        w['aff.w'] = pack_linear_weight(torch.cat(aff_w, 0)); w['aff.b'] = torch.cat(aff_b, 0).contiguous()
        if spec.step_condition:
            self._pack_step(params, w, g)
        # blocks
        for b in spec.blocks:
            p = f'{m}.{b.name}'
            if b.kind == 'conv':
                w[f'{b.name}.w'] = pack_stem_weight(g(f'{p}.weight')); w[f'{b.name}.b'] = g(f'{p}.bias')
                continue
            if b.kind == 'aux':      # the first aux layer reads the network input through ds_stem_im2col, like the stem
                pack = pack_stem_weight if b.res_in == spec.img_resolution else pack_conv_weight
                w[f'{b.name}.w'] = pack(g(f'{p}.weight')); w[f'{b.name}.b'] = g(f'{p}.bias')
                continue
            for leaf in ('norm0', 'norm1'):
                w[f'{b.name}.{leaf}.g'] = g(f'{p}.{leaf}.weight'); w[f'{b.name}.{leaf}.b'] = g(f'{p}.{leaf}.bias')
            w[f'{b.name}.conv0.w'] = pack_conv_weight(g(f'{p}.conv0.weight')); w[f'{b.name}.conv0.b'] = g(f'{p}.conv0.bias')
            w[f'{b.name}.conv1.w'] = pack_conv_weight(g(f'{p}.conv1.weight')); w[f'{b.name}.conv1.b'] = g(f'{p}.conv1.bias')
            if self.up_phase and b.up and b.cin % 32 == 0 and not self.fir:
                w[f'{b.name}.conv0.wup'] = pack_conv_weight_up2(g(f'{p}.conv0.weight'))      # the four folded phase matrices, once per build
            if self.winograd and b.cin % 32 == 0 and b.cout % 256 == 0:
                # Winograd-transformed weights, once per build (a fused skip projection's 1x1 columns follow them untransformed)
                w[f'{b.name}.conv0.wwino'] = pack_conv_weight_wino(g(f'{p}.conv0.weight'))
                w[f'{b.name}.conv1.wwino'] = pack_conv_weight_wino(g(f'{p}.conv1.weight'), g(f'{p}.skip.weight') if b.skip_conv else None)
            if self.conv_mode == 1 and b.cin % 64 == 0 and b.cout % 64 == 0:
                w[f'{b.name}.conv0.w16'] = (pack_conv_weight_f16(g(f'{p}.conv0.weight')), 0)
                w[f'{b.name}.conv1.w16'] = (pack_conv_weight_f16(g(f'{p}.conv1.weight'), g(f'{p}.skip.weight') if b.skip_conv else None), 0)
            elif self.conv_mode == 2 and b.cin % 32 == 0 and b.cout % 32 == 0:
                # ineligible layers (channel counts that are not 32-multiples: tiny / custom nets) keep the exact fp32 kernel
                w[f'{b.name}.conv0.w16'] = pack_conv_weight_split(g(f'{p}.conv0.weight'))
                w[f'{b.name}.conv1.w16'] = pack_conv_weight_split(g(f'{p}.conv1.weight'), g(f'{p}.skip.weight') if b.skip_conv else None)
            if b.skip_conv:
                # skip projection fused into conv1: [3x3 columns | 1x1 columns] along K, biases summed
                w[f'{b.name}.conv1s.w'] = torch.cat([w[f'{b.name}.conv1.w'], pack_conv_weight(g(f'{p}.skip.weight'))], dim=1).contiguous()
                w[f'{b.name}.conv1s.b'] = (g(f'{p}.conv1.bias') + g(f'{p}.skip.bias')).contiguous()
                del w[f'{b.name}.conv1.w']
            if b.heads:
                c, h = b.cout, b.heads
                ch = c // h
                w[f'{b.name}.norm2.g'] = g(f'{p}.norm2.weight'); w[f'{b.name}.norm2.b'] = g(f'{p}.norm2.bias')
                # reference layout of the 3C output channels: index = (head*ch + c)*3 + {q,k,v}  (networks_edm.py:174)
                wq = g(f'{p}.qkv.weight').reshape(h, ch, 3, c)
                bq = g(f'{p}.qkv.bias').reshape(h, ch, 3)
                # q | k | v column blocks, each head-major (head*ch + c): the fused attention kernel reads them in place
                w[f'{b.name}.qkv.w'] = pack_linear_weight(torch.cat([wq[:, :, i].reshape(c, c) for i in range(3)], 0))
                w[f'{b.name}.qkv.b'] = torch.cat([bq[:, :, i].reshape(c) for i in range(3)], 0).contiguous()
                w[f'{b.name}.proj.w'] = pack_conv_weight(g(f'{p}.proj.weight')); w[f'{b.name}.proj.b'] = g(f'{p}.proj.bias')
        w['out.g'] = g(f'{m}.{spec.out_norm}.weight'); w['out.b'] = g(f'{m}.{spec.out_norm}.bias')
        w['outc.w'] = pack_conv_weight(g(f'{m}.{spec.out_conv}.weight')); w['outc.b'] = g(f'{m}.{spec.out_conv}.bias')
        if self.conv_mode == 2 and g(f'{m}.{spec.out_conv}.weight').shape[1] % 32 == 0:
            w['outc.w16'] = pack_conv_weight_split(g(f'{m}.{spec.out_conv}.weight'))
        self.w = w

    def _pack_step(self, params, w, g):
        """The step-condition path of SFD's distilled nets (sfd-main/models/networks_edm.py:290-292 / :438-440, :153): its own embedding MLP and
        every block's `affine_step`, concatenated into one projection of the single step row in the column layout of `aff`.
        Non-adaptive blocks add the two projections (:188): the row is the BIAS of the affine launch, so its own bias carries both layers'.
        Adaptive blocks apply them one after the other (:176-179): the row keeps its own bias and DS_OP_AFFINE_COMPOSE folds it into `aff`
        through `step.pairs`, the table of {scale column, shift column} per four channels of every block."""
        spec, m = self.spec, 'model'
        w['freqs_step'] = w['freqs']
        if spec.embedding_type == 'fourier':                     # map_step is a FourierEmbedding with a buffer of its own
            fs = (2 * np.pi * params[f'{m}.map_step.freqs'].detach().to(device='cpu', dtype=torch.float32)).to(torch.float32)
            assert fs.shape == w['freqs'].shape
            w['freqs_step'] = fs.contiguous().to(self.device)
        for i in (0, 1):
            w[f'mstep{i}.w'] = pack_linear_weight(g(f'{m}.map_step_layer{i}.weight')); w[f'mstep{i}.b'] = g(f'{m}.map_step_layer{i}.bias')
        blocks = [b for b in spec.blocks if b.kind == 'block']
        w['affs.w'] = pack_linear_weight(torch.cat([g(f'{m}.{b.name}.affine_step.weight') for b in blocks], 0))
        bias = torch.cat([g(f'{m}.{b.name}.affine_step.bias') for b in blocks], 0)
        adaptive = {b.adaptive_scale for b in blocks}
        assert len(adaptive) == 1 and bias.numel() == self.aff_total
        self.step_adaptive = adaptive.pop()
        if self.step_adaptive:
            pairs = [(self.aff_off[b.name] + j, self.aff_off[b.name] + b.cout + j) for b in blocks for j in range(0, b.cout, 4)]
            assert all(b.cout % 4 == 0 and self.aff_off[b.name] % 4 == 0 for b in blocks) and self.aff_total % 4 == 0
            w['step.pairs'] = torch.tensor(pairs, dtype=torch.int32).to(self.device).contiguous()
        else:
            bias = w['aff.b'] + bias
        w['affs.b'] = bias.contiguous()

    # ------------------------------------------------------------------------------------------ plan
    def plan(self, B: int, emb_rows: int, step: bool = False) -> _Plan:
        """step: the plan of an evaluation with a step condition (a one-float input `bufs['step']` and the launches of _embedding's step path);
        False is launch for launch the plan of a net without step weights."""
        step = bool(step)
        if step and not self.spec.step_condition:
            raise ValueError('this network was built without step-condition weights (UNetSpec.step_condition)')
        key = (B, emb_rows, self.fuse_norm16) + ((True,) if step else ()) + (('narrow16',) if self.use_fp16 and not self.wide16 else ())
        if key in self._plans:
            return self._plans[key]
        spec, w, lib = self.spec, self.w, self.lib
        bd = Builder(self.device, conv_mode=self.conv_mode, w16_cache=self._w16_cache,       # owns the plan, its workspaces and the emitters
                     invariant=self.batch_invariant, batch=B)
        P, new, bufs = bd.P, bd.new, bd.P.bufs
        R, Bs = spec.img_resolution, emb_rows
        kpad = -(-9 * spec.in_channels // 32) * 32
        bufs['x'] = new(B, spec.in_channels, R, R)           # NCHW, un-scaled (c_in is applied by the stem)
        bufs['sigma'] = new(B)                                # per-sample sigma (row 0 only when Bs == 1 and scalar)
        bufs['sigma_rows'] = torch.zeros(1, dtype=torch.int32, device=self.device)
        bufs['out'] = new(B, spec.out_channels, R, R)         # raw network output F, channel-planar (NCHW) like the user tensors
        if spec.label_dim:
            bufs['labels'] = torch.zeros(Bs, -(-spec.label_dim // 32) * 32, dtype=torch.float32, device=self.device)
        ws = self._workspaces(bd, B, Bs, kpad)
        ws.aff = self._embedding(bd, Bs, step)
        # ---- fp16 residual stream -------------------------------------------------------------------------------
        # The reference's fp16 mode keeps EVERY activation of the U-Net body in fp16 (networks_edm.py:486 `x.to(dtype)`, :165-179 run in
        # that dtype): when every block of this plan runs on the fp16-activation kernels, block outputs (the residual stream, the skip
        # stack) are stored as fp16 rows too -- half the bytes of every epilogue and normalisation pass.  Arithmetic on them is fp32
        # (values are widened when loaded).  Otherwise the stream stays fp32 (the mixed layout of smaller / unusual geometries).
        P.stream16 = ws.stream16 = self.conv_mode == 1 and all(self._dma16(bd, B, b) for b in spec.blocks if b.kind == 'block')
        P.f16_views = []          # (address, bytes) of fp32-typed storage that some launches use as fp16 rows (tests/test_plan_cpu.py's dtype lint)
        x_cur, skips, aux = None, [], None
        for b in spec.blocks:
            nm, Ho, cout = b.name, b.res_out, b.cout
            if b.kind == 'aux':
                # x = skips[-1] = aux = (x + aux_residual(aux)) / sqrt(2)  (networks_edm.py:335): the down block's own output stays in bufs
                out = self._aux_residual(bd, ws, b, aux, x_cur[0])
                x_cur = aux = skips[-1] = (out, cout)
                bufs[nm] = out
                continue
            if b.kind == 'conv':
                bd.add(lib.ds_stem_im2col, (_ptr(bufs['x']), _ptr(bufs['sigma']), Bs, spec.sigma_data, B, spec.in_channels, R, R,
                                            _ptr(ws.act), kpad), 'stem_im2col')
                out = new(B * Ho * Ho, cout)
                bd.conv(ws.act, kpad, kpad, B, R, R, w[f'{nm}.w'], cout, out, cout, 1, nm, bias=w[f'{nm}.b'], stats=True)
            else:
                x0, c0 = x_cur
                x1, c1 = (None, 0)
                if b.pops_skip:
                    x1, c1 = skips.pop()
                    assert c1 == b.skip_cin and c0 + c1 == b.cin
                # a block whose attention runs on the fp32 kernels keeps fp32 outputs; every consumer reads a tensor in the dtype it has
                f16_out = ws.stream16 and (not b.heads or self._attn16(bd, B, b))
                block = self._block16 if self._dma16(bd, B, b) else self._block32
                c1_in, c1_w, c1_kw = block(bd, ws, b, x0, c0, x1, c1)
                out = self._block_out(bd, ws, b, f16_out)
                c1_kw = dict(scale=b.skip_scale, stats=True, w16=w.get(f'{nm}.conv1.w16'), **c1_kw)
                c1_w = self._wino_pick(bd, c1_in, cout, cout, B, Ho, c1_w, w.get(f'{nm}.conv1.wwino'), cout, out, c1_kw)
                bd.conv(c1_in, cout, cout, B, Ho, Ho, c1_w, cout, out, cout, 9, nm + '.conv1', **c1_kw)
                if b.heads:
                    out = self._attention(bd, ws, b, out, f16_out)
            x_cur = (out, cout)
            bufs[nm] = out
            if b.kind == 'conv' or b.pushes_skip:
                skips.append(x_cur)
        assert not skips
        self._head(bd, ws, *x_cur)
        self._plans[key] = bd.finish()
        return P

    def _workspaces(self, bd, B, Bs, kpad):
        """The scratch every block of a plan shares (launches are serial), sized for the largest layer and allocated once."""
        spec, new = self.spec, bd.new
        max_act, max_h, max_attn = kpad * spec.img_resolution ** 2, 0, 0
        for b in spec.blocks:
            hw = b.res_out ** 2
            max_h = max(max_h, b.cout * hw)
            if b.kind == 'block':
                max_act = max(max_act, b.cin * hw, b.cout * hw)
                max_h = max(max_h, b.cin * hw)
                if b.heads:
                    max_attn = max(max_attn, 2 * b.cout * hw)
        ws = SimpleNamespace(B=B, Bs=Bs, max_h=max_h, dec_pp=[None, None], dec_i=0)
        ws.act, ws.hbuf = new(B * max_act), new(B * max_h)
        ws.sres = new(B * max_h)            # resampled skip-path input
        if self.fir:                        # FIR-resampled activated tensor (conv0's input); norm0 of a down block writes ws.act at the INPUT size
            assert max_act >= max(b.cin * b.res_in ** 2 for b in spec.blocks if b.kind == 'block')
            ws.fir = new(B * max_act)
        ws.sproj = new(B * max_h)           # projected skip
        bd.coefs = new(B * 3 * max(max(b.cin, b.cout) for b in spec.blocks))      # {mu, A, B} planes of the fused GroupNorm
        if self.conv_mode == 1:          # fp16 activated tensors: norm0 output, norm1 output, raw copy for the fused skip projection, conv0 output
            ws.a16, ws.b16, ws.r16, ws.h16 = (bd.new16(B * max_act) for _ in range(4))
        if max_attn:
            ws.n2, ws.qk, ws.ao = new(B * max_attn // 2), new(B * max_attn // 2 * 3), new(B * max_attn // 2)
            if self.conv_mode == 1:
                ws.n2_16, ws.ao_16, ws.qk_16 = bd.new16(B * max_attn // 2), bd.new16(B * max_attn // 2), bd.new16(B * max_attn // 2 * 3)
        bd.P.bufs.update(act=ws.act, hbuf=ws.hbuf, sres=ws.sres, sproj=ws.sproj)
        return ws

    def _embedding(self, bd, Bs, step=False):
        """Embedding path (networks_edm.py:314-324 / :429-439) and every block's affine layer in one GEMM; returns its output [Bs, aff_total].
        step: plus the step path on ONE row -- embedding of the raw value, two Linear + SiLU, every `affine_step` in one projection -- whose
        result is the affine launch's bias (non-adaptive blocks) or is folded into its output by one more launch (adaptive blocks)."""
        spec, w, new, bufs = self.spec, self.w, bd.new, bd.P.bufs
        E, NC = spec.emb_channels, spec.noise_channels
        aff_bias = w['aff.b']
        if step:
            bufs['step'] = new(1)
            spos, s0, semb, srow = new(1, NC), new(1, E), new(1, E), new(1, self.aff_total)
            bd.add(self.lib.ds_noise_embed, (_ptr(bufs['step']), 1, _ptr(w['freqs_step']), NC, int(spec.swap_sincos) | 2, _ptr(spos), NC), 'step_embed')
            bd.linear(spos, NC, 1, w['mstep0.w'], E, s0, 'map_step_layer0', bias=w['mstep0.b'], act=DS_ACT_SILU, emb=True)
            bd.linear(s0, E, 1, w['mstep1.w'], E, semb, 'map_step_layer1', bias=w['mstep1.b'], act=DS_ACT_SILU, emb=True)
            bd.linear(semb, E, 1, w['affs.w'], self.aff_total, srow, 'affine_step_all', bias=w['affs.b'], emb=True)
            bufs['aff_step'] = srow
            if not self.step_adaptive:
                aff_bias = srow
        pos, e0, emb, aff = new(Bs, NC), new(Bs, E), new(Bs, E), new(Bs, self.aff_total)
        lab = bufs.get('labels')
        lpad = lab.shape[1] if lab is not None else 0
        # cm_noise (bit 2): the embedding of 1000 * c_noise (CMPrecond, networks_edm.py:540-541)
        bd.add(self.lib.ds_noise_embed, (_ptr(bufs['sigma']), Bs, _ptr(w['freqs']), NC, int(spec.swap_sincos) | (4 if spec.cm_noise else 0), _ptr(pos), NC),
               'noise_embed')
        if spec.model_type == 'SongUNet':
            src = pos
            if lab is not None:
                src = new(Bs, NC)
                bd.linear(lab, lpad, Bs, w['label.w'], NC, src, 'map_label', bias=w['label.b'], res=pos, res_ld=NC, emb=True)
            bd.linear(src, NC, Bs, w['map0.w'], E, e0, 'map_layer0', bias=w['map0.b'], act=DS_ACT_SILU, emb=True)
            bd.linear(e0, E, Bs, w['map1.w'], E, emb, 'map_layer1', bias=w['map1.b'], act=DS_ACT_SILU, emb=True)
        else:
            bd.linear(pos, NC, Bs, w['map0.w'], E, e0, 'map_layer0', bias=w['map0.b'], act=DS_ACT_SILU, emb=True)
            lab_e = None
            if lab is not None:
                lab_e = new(Bs, E)
                bd.linear(lab, lpad, Bs, w['label.w'], E, lab_e, 'map_label', bias=w['label.b'], emb=True)
            bd.linear(e0, E, Bs, w['map1.w'], E, emb, 'map_layer1', bias=w['map1.b'], res=lab_e, res_ld=E, act=DS_ACT_SILU, emb=True)
        bd.linear(emb, E, Bs, w['aff.w'], self.aff_total, aff, 'affine_all', bias=aff_bias, emb=True)
        if step and self.step_adaptive:
            bd.affine_compose(aff, self.aff_total, Bs, self.aff_total, srow, w['step.pairs'], 'affine_compose')
        bufs.update(emb=emb, aff=aff)
        return aff

    def _dma16(self, bd, B, b):
        """Do both 3x3 convolutions of the block run on the fp16-activation kernels (conv1 with the fused skip projection's columns)?"""
        wide = self.wide16 and b.res_out > 64       # the patch kernel: no fused normalisation (Builder.fuses_norm16 ends at 64 pixels)
        return bool(bd.f16_conv_ok(B, b.res_out, b.cin, 0, b.cout, wide=wide) and
                    bd.f16_conv_ok(B, b.res_out, b.cout, b.cin if b.skip_conv else 0, b.cout, wide=wide))

    def _attn16(self, bd, B, b):
        """Attention block on the fp16 kernels end to end (CIFAR-10's single 256-wide head is not: fp32 kernel)?"""
        M = B * b.res_out ** 2
        return bool(self.lib.ds_attention_f16_supported(b.cout // b.heads) and bd.gemm16_ok(M, b.cout, 3 * b.cout) and bd.gemm16_ok(M, b.cout, b.cout))

    def _emb_kw(self, ws, b):
        """(conv0's per-image embedding bias, norm1's adaptive scale / shift) of a block: one of the two is empty."""
        off = self.aff_off[b.name]
        if b.adaptive_scale:
            return {}, dict(scale=ws.aff[:, off:], shift=ws.aff[:, off + b.cout:], ss_ld=self.aff_total, ss_rows=ws.Bs)
        return dict(cbias=ws.aff[:, off:], cbias_ld=self.aff_total, cbias_rows=ws.Bs), {}

    def _block16(self, bd, ws, b, x0, c0, x1, c1):
        """norm0 .. norm1 of a block on the fp16-activation kernels; returns (input, weights, keywords) of its conv1.
        fp16 mode, the reference's storage (networks_edm.py:486 runs the body on x.to(float16)): norm + SiLU (+ resample, + the decoder's
        concatenation) are ONE pass that writes the activated tensor in fp16, and the convolution is a pure matrix kernel on fp16
        activations (csrc/conv3x3_f16dma.hip).  Norm arithmetic is fp32; the block output is fp16 under `stream16`."""
        w, nm, n, Hin, Ho, cin, cout, ncoef = self.w, b.name, ws.B, b.res_in, b.res_out, b.cin, b.cout, bd.coefs
        M = n * Ho * Ho
        G_in, G_out = arch.num_groups(cin), arch.num_groups(cout)
        rs = DS_RESAMPLE_DOWN if b.down else (DS_RESAMPLE_UP if b.up else DS_RESAMPLE_NONE)
        cb, ss = self._emb_kw(ws, b)
        a16, b16 = ws.a16[:M * cin].view(M, cin), ws.b16[:M * cout].view(M, cout)
        h16 = ws.h16[:M * cout].view(M, cout)       # conv0 output: only read by norm1 -> stored in fp16 (networks_edm.py:486)
        # raw (un-normalised) fp16 copy of the block input: operand of the fused 1x1 skip projection, and -- fp16 stream -- the
        # resampled identity skip.  Not needed when the input already is one fp16 tensor of the right geometry.
        direct = ws.stream16 and x1 is None and rs == DS_RESAMPLE_NONE and x0.dtype == torch.float16
        need_raw = (b.skip_conv and not direct) or (ws.stream16 and not b.skip_conv and rs != DS_RESAMPLE_NONE)
        r16 = ws.r16[:M * cin].view(M, cin) if need_raw else None
        # `fuse_norm16`: where every source of a convolution is a raw fp16 tensor of the layer's own geometry, the GroupNorm affine + SiLU
        # is applied by the convolution itself to its LDS halo (conv3x3_f16dma NORM: same arithmetic, same bits) and the ds_norm_act pass
        # -- with it the materialised concatenation and the raw copy for the skip projection -- disappears; the statistics launch
        # (ds_gn_finalize over the producers' column sums) stays.  Resampling blocks keep the pass for conv0.
        fz0 = bool(ws.stream16 and Ho <= 64 and rs == DS_RESAMPLE_NONE and bd.fuses_norm16(self.fuse_norm16, Ho, cout, x0, c0, x1, c1))
        fz1 = bool(ws.stream16 and Ho <= 64 and bd.fuses_norm16(self.fuse_norm16, Ho, cout, h16, cout))
        conv0 = dict(bias=w[f'{nm}.conv0.b'], stats=True, w16=w[f'{nm}.conv0.w16'], in_f16=True, out_f16=True, **cb)
        bd.norm('stats', x0, c0, c0, n, Hin, Hin, nm + '.norm0.stats', x1=x1, c1=c1, ld1=c1, groups=G_in, eps=b.eps,
                gamma=w[f'{nm}.norm0.g'], beta=w[f'{nm}.norm0.b'], coefs=ncoef)
        if fz0:
            r16 = None
            bd.conv(x0, c0, c0, n, Ho, Ho, w[f'{nm}.conv0.w'], cout, h16, cout, 9, nm + '.conv0', x1=x1, c1=c1, ld1=c1, norm_coefs=ncoef,
                    norm_act=DS_ACT_SILU, **conv0)
        else:
            bd.norm('apply', x0, c0, c0, n, Hin, Hin, nm + '.norm0', x1=x1, c1=c1, ld1=c1, groups=G_in, eps=b.eps, use_stats=False,
                    act=DS_ACT_SILU, resample=rs, out=a16, out_ld=cin, out_f16=True, raw_out=r16, raw_ld=cin, coefs=ncoef)
            bd.conv(a16, cin, cin, n, Ho, Ho, w[f'{nm}.conv0.w'], cout, h16, cout, 9, nm + '.conv0', **conv0)
        bd.norm('stats', h16, cout, cout, n, Ho, Ho, nm + '.norm1.stats', groups=G_out, eps=b.eps, gamma=w[f'{nm}.norm1.g'],
                beta=w[f'{nm}.norm1.b'], coefs=ncoef, **ss)             # from conv0's epilogue sums (fp32), incl. the adaptive scale / shift
        if fz1:
            c1_in, kw = h16, dict(in_f16=True, norm_coefs=ncoef, norm_act=DS_ACT_SILU)
        else:
            bd.norm('apply', h16, cout, cout, n, Ho, Ho, nm + '.norm1', groups=G_out, eps=b.eps, use_stats=False, act=DS_ACT_SILU,
                    out=b16, out_ld=cout, out_f16=True, in_f16=True, coefs=ncoef)
            c1_in, kw = b16, dict(in_f16=True)
        if b.skip_conv:          # 1x1 skip projection fused into conv1 as extra K columns on the raw (resampled) fp16 input
            if fz0 and fz1:      # both raw sources straight from the stream: nothing was copied
                kw.update(e0=x0, ec0=c0, e1=x1, ec1=c1)
            else:
                kw.update(e0=x0 if direct else r16, ec0=cin)
            return c1_in, w[f'{nm}.conv1s.w'], dict(kw, bias=w[f'{nm}.conv1s.b'])
        if ws.stream16 and rs != DS_RESAMPLE_NONE:
            kw.update(res=r16, res_ld=cout)          # resampled raw input, already written by the norm0 pass
        else:
            s0 = x0
            if rs != DS_RESAMPLE_NONE:
                bd.norm('apply', x0, c0, c0, n, Hin, Hin, nm + '.skip.resample', x1=x1, c1=c1, ld1=c1, use_stats=False,
                        resample=rs, out=ws.sres, out_ld=cin)
                s0 = ws.sres
            assert x1 is None and c0 == cout
            kw.update(res=s0, res_ld=cout)
        return c1_in, w[f'{nm}.conv1.w'], dict(kw, bias=w[f'{nm}.conv1.b'])

    def _wino_pick(self, bd, x0, c0, ld0, n, side, wgt, wwino, cout, out, kw):
        """Weights of a 3x3 launch bd.conv(x0, ..., **kw): the Winograd-transformed ones -- and kw['wino'] = True -- where this engine has
        them and the library takes the layer in that form (Builder.wino_ok), else `wgt` and kw untouched."""
        if wwino is not None and kw.get('w16') is None and bd.wino_ok(x0, c0, ld0, n, side, side, wwino, cout, out, cout, **kw):
            kw['wino'] = True
            return wwino
        return wgt

    def _block32(self, bd, ws, b, x0, c0, x1, c1):
        """norm0 .. norm1 and the skip path of a block on fp32 activations; returns (input, weights, keywords) of its conv1.  GroupNorm +
        SiLU ride in the 3x3 convolution's halo loader where the LDS-halo kernel takes the shape, else they are a pass (always for a
        resampling norm0)."""
        w, nm, n, Hin, Ho, cin, cout, ncoef = self.w, b.name, ws.B, b.res_in, b.res_out, b.cin, b.cout, bd.coefs
        G_in, G_out = arch.num_groups(cin), arch.num_groups(cout)
        rs = DS_RESAMPLE_DOWN if b.down else (DS_RESAMPLE_UP if b.up else DS_RESAMPLE_NONE)
        cb, ss = self._emb_kw(ws, b)
        src = dict(x1=x1, c1=c1, ld1=c1)
        w16_0 = w.get(f'{nm}.conv0.w16')
        # GroupNorm+SiLU applied by the conv's halo loader -- not where split-fp16 operands come without the fused normalisation: a pass there
        fuse = bd.halo_ok(n, Ho) and not (w16_0 is not None and bd.split_needs_pass(n, Ho, cin))
        conv0 = dict(bias=w[f'{nm}.conv0.b'], stats=True, w16=w16_0, **cb)      # (+ per-image embedding for the non-adaptive variant)
        wup = w.get(f'{nm}.conv0.wup') if b.up and w16_0 is None else None
        if self.fir and rs != DS_RESAMPLE_NONE:
            # resample_filter [1,3,3,1] (networks_edm.py:74-79): activate at the input size, filter (x2 up / stride-2 down, padding 1), convolve
            assert x1 is None and c0 == cin
            M = n * Ho * Ho
            act, rsd = ws.act[:n * Hin * Hin * cin].view(-1, cin), ws.fir[:M * cin].view(M, cin)
            bd.norm('stats', x0, c0, c0, n, Hin, Hin, nm + '.norm0.stats', groups=G_in, eps=b.eps)
            bd.norm('apply', x0, c0, c0, n, Hin, Hin, nm + '.norm0', groups=G_in, eps=b.eps, gamma=w[f'{nm}.norm0.g'], beta=w[f'{nm}.norm0.b'],
                    act=DS_ACT_SILU, resample=DS_RESAMPLE_NONE, out=act, out_ld=cin)
            bd.fir_resample(act, cin, n, Hin, Hin, cin, rsd, cin, nm + '.conv0.fir', up=b.up, taps=self.spec.resample_filter)
            kw0 = dict(conv0)
            w0 = self._wino_pick(bd, rsd, cin, cin, n, Ho, w[f'{nm}.conv0.w'], w.get(f'{nm}.conv0.wwino'), cout, ws.hbuf, kw0)
            bd.conv(rsd, cin, cin, n, Ho, Ho, w0, cout, ws.hbuf, cout, 9, nm + '.conv0', **kw0)
        elif wup is not None and bd.up2_ok(ws.act, cin, cin, n, Ho, Ho, wup, cout, ws.hbuf, cout, **conv0):
            # up block: the pass activates at the input resolution and the convolution reads it through the x2 upsampling (four 2x2 phase
            # convolutions on the low-res rows); the launches are those of the other route, the upsampled tensor is never written
            bd.norm('stats', x0, c0, c0, n, Hin, Hin, nm + '.norm0.stats', groups=G_in, eps=b.eps, **src)
            bd.norm('apply', x0, c0, c0, n, Hin, Hin, nm + '.norm0', groups=G_in, eps=b.eps, gamma=w[f'{nm}.norm0.g'], beta=w[f'{nm}.norm0.b'],
                    act=DS_ACT_SILU, resample=DS_RESAMPLE_NONE, out=ws.act, out_ld=cin, **src)
            bd.conv(ws.act, cin, cin, n, Ho, Ho, wup, cout, ws.hbuf, cout, 9, nm + '.conv0', in_up2=True, **conv0)
        elif fuse and rs == DS_RESAMPLE_NONE:
            bd.norm('stats', x0, c0, c0, n, Hin, Hin, nm + '.norm0.stats', groups=G_in, eps=b.eps, gamma=w[f'{nm}.norm0.g'],
                    beta=w[f'{nm}.norm0.b'], coefs=ncoef, **src)
            kw0 = dict(norm_coefs=ncoef, norm_act=DS_ACT_SILU, **src, **conv0)
            w0 = self._wino_pick(bd, x0, c0, c0, n, Ho, w[f'{nm}.conv0.w'], w.get(f'{nm}.conv0.wwino'), cout, ws.hbuf, kw0)
            bd.conv(x0, c0, c0, n, Ho, Ho, w0, cout, ws.hbuf, cout, 9, nm + '.conv0', **kw0)
        else:
            bd.norm('stats', x0, c0, c0, n, Hin, Hin, nm + '.norm0.stats', groups=G_in, eps=b.eps, **src)
            bd.norm('apply', x0, c0, c0, n, Hin, Hin, nm + '.norm0', groups=G_in, eps=b.eps, gamma=w[f'{nm}.norm0.g'], beta=w[f'{nm}.norm0.b'],
                    act=DS_ACT_SILU, resample=rs, out=ws.act, out_ld=cin, **src)
            kw0 = dict(conv0)
            w0 = self._wino_pick(bd, ws.act, cin, cin, n, Ho, w[f'{nm}.conv0.w'], w.get(f'{nm}.conv0.wwino'), cout, ws.hbuf, kw0)
            bd.conv(ws.act, cin, cin, n, Ho, Ho, w0, cout, ws.hbuf, cout, 9, nm + '.conv0', **kw0)
        # norm1 (+adaptive scale/shift) + silu
        if fuse:
            bd.norm('stats', ws.hbuf, cout, cout, n, Ho, Ho, nm + '.norm1.stats', groups=G_out, eps=b.eps, gamma=w[f'{nm}.norm1.g'],
                    beta=w[f'{nm}.norm1.b'], coefs=ncoef, **ss)
            c1_in, kw = ws.hbuf, dict(norm_coefs=ncoef, norm_act=DS_ACT_SILU)
        else:
            bd.norm('stats', ws.hbuf, cout, cout, n, Ho, Ho, nm + '.norm1.stats', groups=G_out, eps=b.eps)
            bd.norm('apply', ws.hbuf, cout, cout, n, Ho, Ho, nm + '.norm1', groups=G_out, eps=b.eps, gamma=w[f'{nm}.norm1.g'],
                    beta=w[f'{nm}.norm1.b'], act=DS_ACT_SILU, out=ws.act, out_ld=cout, **ss)
            c1_in, kw = ws.act, {}
        # skip path: raw (resampled) input, projected by a 1x1 that is fused into conv1 as extra K columns
        s0, sc0, s1, sc1 = x0, c0, x1, c1
        if self.fir and rs != DS_RESAMPLE_NONE:
            bd.fir_resample(x0, c0, n, Hin, Hin, cin, ws.sres, cin, nm + '.skip.fir', up=b.up, taps=self.spec.resample_filter)
            s0, sc0, s1, sc1 = ws.sres, cin, None, 0
        elif rs != DS_RESAMPLE_NONE:
            bd.norm('apply', x0, c0, c0, n, Hin, Hin, nm + '.skip.resample', use_stats=False, resample=rs, out=ws.sres, out_ld=cin, **src)
            s0, sc0, s1, sc1 = ws.sres, cin, None, 0
        if b.skip_conv:
            return c1_in, w[f'{nm}.conv1s.w'], dict(kw, bias=w[f'{nm}.conv1s.b'], e0=s0, ec0=sc0, e1=s1, ec1=sc1)
        assert s1 is None and sc0 == cout
        return c1_in, w[f'{nm}.conv1.w'], dict(kw, bias=w[f'{nm}.conv1.b'], res=s0, res_ld=cout)

    def _aux_residual(self, bd, ws, b, aux, x):
        """enc.RxR_aux_residual (networks_edm.py:283, :335; Conv2d.forward's fused down form, :70-72): conv2d(aux, w, padding=2) as the padding-1
        3x3 convolution on the zero-ringed input (its ring of outputs is computed, not zero), then ONE launch for the stride-2 [1,3,3,1]
        filter, the layer's bias, the down block's output `x` and the 1/sqrt(2).  aux None: the network input c_in x (channel-planar), read
        through ds_stem_im2col like the stem; else (tensor, channels) of the previous level's aux in NHWC rows."""
        spec, w, nm, n, R, cout = self.spec, self.w, b.name, ws.B, b.res_in, b.cout
        Rp, bufs = R + 2, bd.P.bufs
        conv = bd.new(n * Rp * Rp, cout)
        if aux is None:
            kpad = -(-9 * spec.in_channels // 32) * 32
            ring, cols = bd.new(n, spec.in_channels, Rp, Rp), bd.new(n * Rp * Rp, kpad)
            bd.zero_border(bufs['x'], ring, n * spec.in_channels, R, R, 1, 1, nm + '.ring')
            bd.add(self.lib.ds_stem_im2col, (_ptr(ring), _ptr(bufs['sigma']), ws.Bs, spec.sigma_data, n, spec.in_channels, Rp, Rp, _ptr(cols), kpad),
                   nm + '.im2col')
            bd.conv(cols, kpad, kpad, n, Rp, Rp, w[f'{nm}.w'], cout, conv, cout, 1, nm + '.conv')
        else:
            t, caux = aux
            assert caux == b.cin
            ring = bd.new(n * Rp * Rp, caux)
            bd.zero_border(t, ring, n, R, R, caux, 1, nm + '.ring')
            bd.conv(ring, caux, caux, n, Rp, Rp, w[f'{nm}.w'], cout, conv, cout, 9, nm + '.conv')
        out = bd.new(n * b.res_out ** 2, cout)
        bd.fir_resample(conv, cout, n, Rp, Rp, cout, out, cout, nm + '.fir', pad=0, taps=spec.resample_filter, bias=w[f'{nm}.b'], res=x, res_ld=cout,
                        scale=b.skip_scale)
        return out

    def _block_out(self, bd, ws, b, f16):
        """Output buffer of a block (and of its attention): encoder outputs are kept for the skip stack, decoder outputs ping-pong between two
        fp32-sized buffers that blocks use in either dtype."""
        M = ws.B * b.res_out ** 2
        if b.pushes_skip or b.name == self.tap_block:
            return bd.new16(M, b.cout) if f16 else bd.new(M, b.cout)
        t = ws.dec_pp[ws.dec_i]
        if t is None:
            t = ws.dec_pp[ws.dec_i] = bd.new(ws.B * ws.max_h)
        ws.dec_i ^= 1
        if f16:
            bd.P.f16_views.append((t.data_ptr(), t.numel() * 2))
            return t.view(torch.float16)[:t.numel()]
        return t

    def _attention(self, bd, ws, b, x, f16_out):
        """GroupNorm -> packed q | k | v 1x1 -> fused attention (networks_edm.py:171-176: softmax(Q K^T / sqrt(ch)) V per (image, head), scores
        kept on chip) -> 1x1 proj (+ residual) on the block's conv1 output `x`; returns the block output."""
        w, nm, n, Ho, cout, hd = self.w, b.name, ws.B, b.res_out, b.cout, b.heads
        S, ch = Ho * Ho, cout // hd
        M = n * S
        G = arch.num_groups(cout)
        # fp16 mode: the GroupNorm output and the attention output are only operands of the qkv / proj 1x1s, and q | k | v are the rows the
        # reference's qkv projection emits (networks_edm.py:171-173) -> fp16 rows, streamed by the fp16-activation GEMM (csrc/gemm_f16dma.hip)
        if self._attn16(bd, n, b):
            n2, ao, qk = ws.n2_16[:M * cout].view(M, cout), ws.ao_16[:M * cout].view(M, cout), ws.qk_16
        else:
            n2, ao, qk = ws.n2, ws.ao, ws.qk
        bd.norm('stats', x, cout, cout, n, Ho, Ho, nm + '.norm2.stats', groups=G, eps=b.eps)
        bd.norm('apply', x, cout, cout, n, Ho, Ho, nm + '.norm2', groups=G, eps=b.eps, gamma=w[f'{nm}.norm2.g'], beta=w[f'{nm}.norm2.b'],
                out=n2, out_ld=cout, out_f16=(n2.dtype == torch.float16))
        bd.conv(n2, cout, cout, n, Ho, Ho, w[f'{nm}.qkv.w'], 3 * cout, qk, 3 * cout, 1, nm + '.qkv', bias=w[f'{nm}.qkv.b'])
        bd.attention(qk, qk[cout:], qk[2 * cout:], ao, nm + '.attention', batch=n, heads=hd, sq=S, skv=S, d=ch, ldq=3 * cout, ldk=3 * cout,
                     ldv=3 * cout, ldo=cout, q_bs=S * 3 * cout, k_bs=S * 3 * cout, v_bs=S * 3 * cout, o_bs=S * cout, scale=1.0 / math.sqrt(ch))
        out = self._block_out(bd, ws, b, f16_out)
        bd.conv(ao, cout, cout, n, Ho, Ho, w[f'{nm}.proj.w'], cout, out, cout, 1, nm + '.proj', bias=w[f'{nm}.proj.b'], res=x, res_ld=cout,
                scale=b.skip_scale, stats=True)
        return out

    def _head(self, bd, ws, xo, co):
        """Output head: GroupNorm + SiLU + 3x3 conv to the channel-planar network output, with the solver update fused where it can be."""
        spec, w, lib, P = self.spec, self.w, self.lib, bd.P
        B, R, G = ws.B, spec.img_resolution, arch.num_groups(co)
        if bd.halo_ok(B, R) and xo.dtype == torch.float32:
            bd.norm('stats', xo, co, co, B, R, R, 'out.norm.stats', groups=G, eps=spec.out_eps, gamma=w['out.g'], beta=w['out.b'], coefs=bd.coefs)
            bd.conv(xo, co, co, B, R, R, w['outc.w'], spec.out_channels, P.bufs['out'], 4, 9, 'out.conv', bias=w['outc.b'],
                    norm_coefs=bd.coefs, norm_act=DS_ACT_SILU, out_nchw=1, w16=w.get('outc.w16'))
        else:
            bd.norm('stats', xo, co, co, B, R, R, 'out.norm.stats', groups=G, eps=spec.out_eps)
            bd.norm('apply', xo, co, co, B, R, R, 'out.norm', groups=G, eps=spec.out_eps, gamma=w['out.g'], beta=w['out.b'], act=DS_ACT_SILU,
                    out=ws.act, out_ld=co)
            bd.conv(ws.act, co, co, B, R, R, w['outc.w'], spec.out_channels, P.bufs['out'], 4, 9, 'out.conv', bias=w['outc.b'], out_nchw=1)
        # ---- the solver update fused into the head (ds_conv_args.update): the head launch carries a pointer to ONE persistent
        # ds_update_args of this plan; EDMDenoiser.raw(update=...) fills it before a run and clears its outputs afterwards (x_out == m_out ==
        # NULL = plain head).  Possible where the head runs on conv3x3_thin_kernel with a channel-planar output (ds_conv_kernel_id 2570).
        head = P.ops[-1].keep[0]
        P.head_update = _lib.UpdateArgs()
        P.head_fusable = bool(head.out_nchw and not head.wgt_f16 and lib.ds_conv_kernel_id(C.byref(head)) == 2570)
        if P.head_fusable:
            head.update = C.cast(C.pointer(P.head_update), C.c_void_p)

    def flops(self, B):
        return arch.flops_per_image(self.spec) * B


class EDMDenoiser:
    """Drop-in for the reference ``EDMPrecond`` object (networks_edm.py:460-499) backed by the HIP engine.

    ``net(x, sigma, class_labels=None)`` -> denoised NCHW fp32, like the reference.  The fused solvers bypass
    the final ``c_skip x + c_out F`` pass and read the raw output through ``raw()`` instead.
    """
    edm_raw_output = True      # solvers._Run: ds_solver_update applies the EDM preconditioning to the raw output itself

    def __init__(self, spec: arch.UNetSpec, params: Dict[str, torch.Tensor], device='cuda', use_fp16=False, split_fp16=False,
                 batch_invariant=False, up_phase=True, winograd=True, wide16=True):
        """batch_invariant: same seed, same bits at any batch (UNetEngine).  up_phase, winograd, wide16: UNetEngine."""
        self.spec = spec
        self.engine = UNetEngine(spec, params, device, use_fp16=use_fp16, split_fp16=split_fp16, batch_invariant=batch_invariant,
                                 up_phase=up_phase, winograd=winograd, wide16=wide16)
        self.batch_invariant = bool(batch_invariant)
        self.device = self.engine.device
        self.img_resolution = spec.img_resolution
        self.img_channels = spec.in_channels
        self.label_dim = spec.label_dim
        self.sigma_min = spec.sigma_min
        self.sigma_max = spec.sigma_max
        self.sigma_data = spec.sigma_data
        self.use_fp16 = bool(use_fp16)   # read-only after construction (weights are packed for the mode), like net.use_fp16 of the reference
        self._last = None                # (plan, batch) of the last __call__ evaluation (block_output)
        self.bottleneck_name = None      # set by the AMED path: 'enc.8x8_block3' / 'enc.8x8_block2'

    @classmethod
    def from_config(cls, name_or_kwargs, seed=0, mode='signal', device='cuda', use_fp16=False, split_fp16=False, batch_invariant=False,
                    up_phase=True, winograd=True, step_condition=False, wide16=True):
        """step_condition: the net with SFD's step-condition weights (arch.UNetSpec.step_condition)."""
        kw = arch.NAMED_CONFIGS[name_or_kwargs] if isinstance(name_or_kwargs, str) else name_or_kwargs
        if step_condition:
            kw = dict(kw, step_condition=True)
        spec = arch.edm_precond_spec(**kw)
        return cls(spec, arch.init_params(spec, seed=seed, mode=mode), device, use_fp16=use_fp16, split_fp16=split_fp16,
                   batch_invariant=batch_invariant, up_phase=up_phase, winograd=winograd, wide16=wide16)

    @classmethod
    def from_reference_module(cls, net, device='cuda', use_fp16=None, batch_invariant=False):
        """Build from a live reference ``EDMPrecond`` instance (duck-typed: pickled EDM classes are exec'd from
        source, so ``isinstance`` is useless -- persistence.py:222-233).  ``use_fp16`` None: follow the module's own flag
        (networks_edm.py:472, :486 -- the public ImageNet-64 checkpoint carries use_fp16=True)."""
        spec = spec_from_module(net)
        if use_fp16 is None:
            use_fp16 = bool(getattr(net, 'use_fp16', False))
        params = {k: v for k, v in net.state_dict().items() if 'resample_filter' not in k}
        known = {k for k, _, _ in arch.param_table(spec)}
        extra = sorted(set(params) - known)
        if extra:               # a layer the engine would not evaluate must not be dropped without a word
            raise NotImplementedError(f'{len(extra)} state-dict entries of the module have no place in the recovered spec: {extra[:4]} ...')
        return cls(spec, params, device, use_fp16=use_fp16, batch_invariant=batch_invariant)

    def eval(self):
        return self

    def to(self, *a, **k):
        return self

    # -- raw evaluation: fills plan inputs, runs the plan, returns (F_nhwc4, plan) -----------------------------------
    def _step_value(self, step_condition, skip_tuning=False):
        """ops.step_value for this net: the evaluation's step condition as a host float, or None."""
        from . import ops
        return ops.step_value(step_condition, self.spec.step_condition, skip_tuning)

    def _prepare(self, x, sigma, class_labels, step=None):
        B = x.shape[0]
        lib = self.engine.lib
        st = _lib.stream_ptr()
        host_scalar = isinstance(sigma, (int, float))
        if host_scalar:
            emb_rows = B if self.label_dim else 1
        else:
            sigma = torch.as_tensor(sigma, dtype=torch.float32, device=self.device).reshape(-1).contiguous()
            emb_rows = B if (sigma.numel() > 1 or self.label_dim) else 1
        plan = self.engine.plan(B, emb_rows, step is not None)
        if step is not None:     # written by a kernel, like a host-scalar sigma
            _lib.check(lib.ds_fill(_ptr(plan.bufs['step']), step, 1, st), 'fill step')
        xb = plan.bufs['x']
        if x.data_ptr() != xb.data_ptr():
            assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
            _lib.check(lib.ds_copy_rows(_ptr(x), x[0].numel(), _ptr(xb), x[0].numel(), B, x[0].numel(), st), 'copy x')
        sb = plan.bufs['sigma']
        if host_scalar:      # no H2D copy: the sigma rows are written by a kernel
            _lib.check(lib.ds_fill(_ptr(sb), float(sigma), emb_rows, st), 'fill sigma')
        elif sigma.data_ptr() != sb.data_ptr():
            if sigma.numel() == 1 and emb_rows > 1:
                sigma = sigma.expand(emb_rows).contiguous()
            _lib.check(lib.ds_copy_rows(_ptr(sigma), 1, _ptr(sb), 1, emb_rows, 1, st), 'copy sigma')
        if self.label_dim:
            lb = plan.bufs['labels']
            if class_labels is None:
                lb.zero_()
            else:
                cl = class_labels.to(torch.float32).reshape(-1, self.label_dim).contiguous()
                if cl.shape[0] == 1 and B > 1:
                    cl = cl.expand(B, -1).contiguous()
                _lib.check(lib.ds_copy_rows(_ptr(cl), self.label_dim, _ptr(lb), lb.shape[1], B, self.label_dim, st), 'copy labels')
        return plan, emb_rows

    def raw(self, x, sigma, class_labels=None, update=None, step_condition=None):
        """F(c_in x; c_noise), the raw network output, as an NCHW [B, C, H, W] tensor.  Engine-owned, overwritten by the
        next evaluation at the same batch size.
        update: a filled ``_lib.UpdateArgs`` (raw = 1, f ignored): the network head applies that solver update in its epilogue -- no update
        launch (``head_update_ok(B, ...)`` says whether this plan's head can; csrc/conv3x3_thin.hip).
        A plan is SINGLE-STREAM state: its workspaces, its input buffers and the one ``head_update`` struct the head launch points at are
        written here and read by the launches that follow, so two threads / streams must not evaluate the same (denoiser, batch) plan
        concurrently -- build one denoiser per stream (the reference's module has the same contract: one process, one stream per rank)."""
        plan, _ = self._prepare(x, sigma, class_labels, self._step_value(step_condition))
        if update is None:
            plan.run(_lib.stream_ptr())
            return plan.bufs['out'], plan
        if not plan.head_fusable:
            raise _lib.DsError('this plan\'s head does not run on the kernel that can fuse the solver update')
        hu = plan.head_update
        C.memmove(C.byref(hu), C.byref(update), C.sizeof(hu))
        try:
            plan.run(_lib.stream_ptr())
        finally:
            hu.x_out, hu.m_out = None, None                      # the next plain evaluation must not update anything
        return plan.bufs['out'], plan

    def head_update_ok(self, B, sigma, class_labels=None, step_condition=None):
        """True when an evaluation at this batch / sigma form can carry a fused solver update (solvers._Run asks before it defers)."""
        host_scalar = isinstance(sigma, (int, float))
        emb_rows = (B if self.label_dim else 1) if host_scalar else (B if (torch.as_tensor(sigma).numel() > 1 or self.label_dim) else 1)
        return bool(self.engine.plan(B, emb_rows, self._step_value(step_condition) is not None).head_fusable)

    def __call__(self, x, sigma, class_labels=None, force_fp32=False, step_condition=None, skip_tuning=False, **kwargs):
        """step_condition: None (the plain evaluation, also on a step-capable net) or the one value of this evaluation (_step_value)."""
        from . import ops
        B, Cc, H, W = x.shape
        x = x.to(torch.float32).contiguous()
        plan, emb_rows = self._prepare(x, sigma, class_labels, self._step_value(step_condition, skip_tuning))
        plan.run(_lib.stream_ptr())
        self._last = (plan, B)
        out = torch.empty_like(x)
        # D = c_skip x + c_out F, evaluated by the update kernel with cx = 0, cm = 1, store_d = 0 (m = D)
        args = ops.make_update_args(plan.bufs['x'], plan.bufs['x'], plan.bufs['out'], B, Cc, H, W, None, raw=True, f_ld=0,
                                    coefs=self._sigma_coefs(plan, emb_rows), coef_rows=(B if emb_rows > 1 else 1),
                                    sigma_data=self.sigma_data, m_out=out, store_d=False)
        ops.solver_update(args)
        return out

    def _sigma_coefs(self, plan, emb_rows):
        """[rows][8] coefficient rows carrying sigma in slot 6 (and t = 1 in slot 5)."""
        rows = emb_rows
        key = ('sigcoef', rows)
        if key not in plan.bufs:
            plan.bufs[key] = torch.zeros(rows, 8, dtype=torch.float32, device=self.device)
            plan.bufs[key][:, 5] = 1.0
        cf = plan.bufs[key]
        lib = self.engine.lib
        _lib.check(lib.ds_copy_rows(_ptr(plan.bufs['sigma']), 1, _ptr(cf[:, 6:]), 8, rows, 1, _lib.stream_ptr()), 'sigma->coefs')
        return cf

    def block_output(self, name):
        """Output of block ``name`` ('enc.8x8_block3', 'enc.16x16_block0', ...) of the LAST ``net(x, sigma, ...)`` evaluation, as the
        NCHW tensor ``[B, C, h, w]`` a forward hook on that block of the reference module would see (solvers_amed.py:7-18 taps
        ``net.model.enc['8x8_block3']``).  A copy: the plan's own buffer is overwritten by the next evaluation."""
        plan, B = self._last
        t = plan.bufs[name].float()          # fp16 residual stream (fp16 mode): widened for the caller
        hw = t.shape[0] // B
        h = int(round(hw ** 0.5))
        assert h * h == hw, (name, tuple(t.shape), B)
        return t.reshape(B, h, h, t.shape[1]).permute(0, 3, 1, 2).contiguous()

    def bottleneck_mean(self, plan, B, class_cond):
        """Channel mean of the AMED bottleneck tap, [B, 8, 8] (solvers_amed.py:16-17, :24-28)."""
        from . import ops
        name = 'enc.8x8_block2' if class_cond else 'enc.8x8_block3'
        t = plan.bufs[name].float()
        c = t.shape[1]
        out = torch.empty(B, 8, 8, dtype=torch.float32, device=self.device)
        ops.channel_mean(t, c, c, B * 64, out)
        return out


def spec_from_module(net) -> arch.UNetSpec:
    """Recover the UNetSpec of a live reference EDMPrecond by attribute inspection."""
    model = net.model
    names = list(model.enc.keys())
    song = any('aux' in k for k in model.dec.keys())
    first = model.enc[names[0]]
    res0 = int(net.img_resolution)
    # SFD's step-conditioned nets carry map_step_layer{0,1} and an affine_step in every block (sfd-main/models/networks_edm.py:291, :153)
    every_block = [blk for part in (model.enc, model.dec) for blk in part.values() if getattr(blk, 'affine', None) is not None]
    with_step = [getattr(blk, 'affine_step', None) is not None for blk in every_block]
    step = getattr(model, 'map_step_layer0', None) is not None
    if any(with_step) != step or (any(with_step) and not all(with_step)):
        raise ValueError(f'inconsistent step-condition layers: map_step_layer0 {"present" if step else "absent"}, affine_step in '
                         f'{sum(with_step)} of {len(with_step)} blocks')
    mc_emb = model.map_layer0.weight.shape[0]
    blocks = [k for k in names if 'block' in k]
    levels = sorted({int(k.split('x')[0]) for k in names}, reverse=True)
    num_blocks = sum(1 for k in blocks if k.startswith(f'{res0}x{res0}_block'))
    if song:
        # the three NCSN++ options are recovered from what they leave in the tree (networks_edm.py:261, :279-284, :56-58); the encoder /
        # decoder variants the engine does not evaluate are refused here -- their layers would otherwise be dropped without a word
        every = [f'enc.{k}' for k in names] + [f'dec.{k}' for k in model.dec.keys()]
        odd = [k for k in every if any(t in k for t in ('aux_down', 'aux_skip', 'aux_up'))]
        if odd:
            raise NotImplementedError(f'SongUNet with encoder_type / decoder_type "skip" is not supported (layers {odd[:3]} ...)')
        fourier = getattr(getattr(model, 'map_noise', None), 'freqs', None) is not None
        residual = any('aux_residual' in k for k in names)
        taps = [1, 1]
        for k in names:
            f = getattr(getattr(model.enc[k], 'conv0', None), 'resample_filter', None) if k.endswith('_down') else None
            if f is not None:
                if f.shape[-1] not in (2, 4):
                    raise NotImplementedError(f'resample_filter of {tuple(f.shape)} in enc.{k}: only [1,1] and [1,3,3,1] are supported')
                taps = [1, 1] if f.shape[-1] == 2 else [1, 3, 3, 1]
                break
        model_channels = first.out_channels
        mult = [model.enc[f'{r}x{r}_block0'].out_channels // model_channels for r in levels]
        attn = [r for r in levels if getattr(model.enc[f'{r}x{r}_block0'], 'num_heads', 0)]
        spec = arch.song_unet_spec(res0, net.img_channels, net.img_channels, label_dim=net.label_dim,
                                   augment_dim=(model.map_augment.weight.shape[1] if getattr(model, 'map_augment', None) is not None else 0),
                                   model_channels=model_channels, channel_mult=mult, channel_mult_emb=mc_emb // model_channels,
                                   num_blocks=num_blocks, attn_resolutions=attn,
                                   channel_mult_noise=model.map_layer0.weight.shape[1] // model_channels,
                                   embedding_type='fourier' if fourier else 'positional', encoder_type='residual' if residual else 'standard',
                                   resample_filter=taps, step_condition=step)
    else:
        model_channels = model.map_layer0.weight.shape[1]
        mult = [model.enc[f'{r}x{r}_block0'].out_channels // model_channels for r in levels]
        attn = [r for r in levels if getattr(model.enc[f'{r}x{r}_block0'], 'num_heads', 0)]
        spec = arch.dhariwal_unet_spec(res0, net.img_channels, net.img_channels, label_dim=net.label_dim,
                                       augment_dim=(model.map_augment.weight.shape[1] if getattr(model, 'map_augment', None) is not None else 0),
                                       model_channels=model_channels, channel_mult=mult, channel_mult_emb=mc_emb // model_channels,
                                       num_blocks=num_blocks, attn_resolutions=attn, step_condition=step)
    spec.sigma_data = float(getattr(net, 'sigma_data', 0.5))
    spec.sigma_min = float(getattr(net, 'sigma_min', 0.002))
    spec.sigma_max = float(getattr(net, 'sigma_max', 80.0))
    return spec
