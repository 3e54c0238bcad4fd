"""Launch plans: a flat list of (C entry point, prebuilt argument struct) over engine-owned workspaces.

A plan is compiled once per (network, batch size); running it is a tight ctypes loop, and because no pointer changes
between runs it can be captured into a hipGraph (``graph.py``).  ``Builder`` is the small DSL the engines use to emit
launches; it only marshals arguments -- every operation is a libdsamd kernel (or, for the NCSN++ networks, one of the two libdsmetrics
launches of ``fir_resample`` / ``zero_border``: such a plan is ``foreign`` and runs through ``run_python``).  Two levels: one launch (``conv``, ``norm``,
``attention``, ...) and the blocks more than one network is made of (``gn_conv3x3``, ``upsample_conv``, ``widen``), which decide WHICH
launches a block becomes and take their temporaries from the builder's recycling allocator (``alloc`` / ``free``); ``finish`` ends
every plan build.
"""
from __future__ import annotations

import ctypes as C
import os
from types import SimpleNamespace
from typing import Dict, List

import torch

from . import _lib
from ._lib import AttnArgs, ConvArgs, ConvRouteInfo, GemmArgs, GnFinalizeArgs, NormArgs, DS_ACT_NONE, DS_ACT_SILU, DS_RESAMPLE_NONE, DS_RESAMPLE_UP


SPLITK_WORKSPACE_FLOATS = 64 << 20      # 256 MiB per plan

# ---- Tile shapes of the fp16-activation kernels, MEASURED per layer shape when a plan is built on the GPU ------------------------------
# csrc/conv3x3_f16dma.hip and csrc/gemm_f16dma.hip choose the column-tile width (64 * nb, nb = 1..4) and, for the GEMM, 128- or 256-row
# tiles (nw = 4 / 8) from a small cost model.  The A/B sessions of rounds 3 and 4 (docs/HISTORY.md D, E.7) found that model wrong by
# 5 - 20 % on individual shapes in both directions -- the regime is latency-bound and no static rule survived two boxes.  So the planner
# measures: the first time a shape is planned in this process, the launch itself (the plan's own buffers, inputs filled with random fp16
# values, the L2 / MALL flushed before every timed launch so that weights come from HBM as they do inside a network, the library's own
# choice timed first AND last because the first launches after host-side work run on a clock that is still ramping) is timed under every
# (nb, nw) candidate, and the winner travels in ds_conv_args.tune -- per call, the library keeps no state.  A candidate must beat the
# library's own choice by 3 % to replace it.  Only launches whose every output bit is independent of the tile shape are measured
# (_tile_neutral): each output element is the same K-ordered fp32 sum under any tile, the epilogue arithmetic is per element, and the
# GroupNorm column sums of the store-from-accumulators epilogue are taken per 64-row block whatever the width; the STAGED epilogue's
# column sums follow its pass geometry (32- vs 64-column blocks), so layers that leave column sums through it keep the cost-model tile.
# Results are therefore bit-identical with or without the measurement (tests/test_hip_fp16.py).  The split-K factor, which does
# change the order of the fp32 sums, stays rule-based (conv3x3_f16dma_splits: a function of the layer alone; ds_conv_route reports it).
# DS_AUTOTUNE=0 in the environment, or Builder(autotune=False), switches it off; launches whose tune words a test / benchmark has set are left alone; nothing
# is measured during a stream capture.  Measured gain on whole sampler calls (session r7a, alternating in one process): SD-1.5 fp16
# +1.5 %, ImageNet-64 fp16 +0.6 %.
AUTOTUNE = os.environ.get('DS_AUTOTUNE', '1') != '0'
FOLD_FINALIZE = os.environ.get('DS_FOLD_GN_FINALIZE', '0') == '1'       # Builder._fold_finalize: OFF by default (measured a wash, see there)
_TUNE_CACHE: Dict[tuple, tuple] = {}     # (device, layer signature) -> (nb, nw, {candidate: ms}): the table's entries + what this process measured
_MEASURED: Dict[str, list] = {}          # table keys measured in THIS process (misses of the persisted table): save_tile_table() writes them
_FLUSH: Dict[int, torch.Tensor] = {}     # device index -> the 512 MiB scratch written before every timed launch; freed by release_tuning_scratch()

# ---- The measured table is PERSISTED (round 5; package data since round 6: diff_sampler_amd/data/tile_table.json travels with an installed or
# relocated package), keyed by layer signature and tied to the hash of the two kernel
# translation units it was measured on.  A plan build looks a shape up there first and measures only on a miss, so (a) two runs of the
# same tree choose identical tiles -- routing is reproducible, where an on-box timing race was not --, (b) building the benchmarked
# plans costs no measurement launches (bench.py's setup_s), and (c) the profiler sees no tuning launches.  The table is regenerated on
# a GPU box by `python tools/make_tile_table.py` (it builds the benchmarked plans with the table ignored and writes what it measured);
# a table whose kernel hashes differ from the current sources, or that was measured on another device (architecture name + CU count), is
# ignored -- stale or foreign measurements never steer a kernel -- and the miss is reported ONCE (RuntimeWarning): routing then falls back to
# on-box measurement (+5 ... 9 s per network on first use, tiles no longer reproducible run to run).  DS_TILE_TABLE=<path> | off overrides.
TILE_TABLE_FILE = os.environ.get('DS_TILE_TABLE', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'data', 'tile_table.json'))
WIDE_EXTRA = 131072             # ds_conv_tune.variant bit 17
TILE_TABLE_KERNELS = ('conv3x3_f16dma.hip', 'gemm_f16dma.hip')
_TABLE = {'loaded': False, 'entries': {}, 'why': None}

# default of the engines' fuse_norm16: '0' never, '1' every eligible layer, 'auto' the layer classes where the per-layer A/B of round 5 found the
# fusion faster than pass + convolution (profiles/r5_conv_f16dma_fused_norm_per_layer.txt): 64x64 images and one column tile (cout <= 192).
# Whole-net A/B of '1' against '0': profiles/r5_conv_f16dma_fused_norm_ab.txt (ImageNet-64 +0.4 %, SD-1.5 -6.8 %).
FUSE_NORM16_DEFAULT = 'auto'


def fuse_norm16_value(text):
    """'0' / '1' / 'auto' (DS_FUSE_NORM16, or the engines' attribute) -> False / True / 'auto'."""
    return {'0': False, '1': True}.get(str(text), 'auto')


def fuse_norm16_here(mode, side, cout):
    """Does the 3x3 convolution of this geometry normalise its own LDS halo (conv3x3_f16dma NORM) under `mode`?"""
    return mode is True or (mode == 'auto' and side == 64 and cout <= 192)


def _table_hashes():
    from . import build
    return {tu: build.source_sha256(tu) for tu in TILE_TABLE_KERNELS}


def _device_tag():
    """'gfx950:sramecc+:xnack-/256' of the current GPU, or None without one (CPU-side tests read the table without a device check)."""
    if not torch.cuda.is_available():
        return None
    pr = torch.cuda.get_device_properties(torch.cuda.current_device())
    return f'{pr.gcnArchName}/{pr.multi_processor_count}'


def load_tile_table(path=None, force=False):
    """Entries {key string: [nb, nw, {"nb,nw": ms}]} of the persisted table, or {} (with _TABLE['why']) when it is absent / stale / measured on
    another device / switched off by DS_TILE_TABLE=off."""
    if _TABLE['loaded'] and not force and path is None:
        return _TABLE['entries']
    _TABLE.update(loaded=True, entries={}, why=None)
    f = path or TILE_TABLE_FILE
    if f == 'off':
        _TABLE['why'] = 'switched off (DS_TILE_TABLE=off)'
        return _TABLE['entries']
    try:
        import json
        with open(f) as fh:
            z = json.load(fh)
        then, now = z['meta']['kernel_source_sha256'], _table_hashes()
        here, there = _device_tag(), z['meta'].get('device')
        if any(then.get(tu) != now[tu] for tu in TILE_TABLE_KERNELS):
            _TABLE['why'] = f'{os.path.basename(f)} was measured on other kernel sources: ignored'
        elif here is not None and there is not None and '/' in str(there) and there != here:
            _TABLE['why'] = f'{os.path.basename(f)} was measured on {there}, this device is {here}: ignored'
        else:
            _TABLE['entries'] = dict(z['entries'])
    except (OSError, KeyError, ValueError) as e:
        _TABLE['why'] = f'no usable tile table ({type(e).__name__}: {e})'
    if _TABLE['why'] and torch.cuda.is_available():
        import warnings
        warnings.warn(f'diff_sampler_amd: {_TABLE["why"]} -- fp16 tile shapes will be measured on this box (slower first plan build, routing not '
                      f'reproducible run to run); regenerate with tools/make_tile_table.py', RuntimeWarning, stacklevel=2)
    return _TABLE['entries']


def save_tile_table(path, session=''):
    """Write the persisted entries merged with what this process measured (tools/make_tile_table.py)."""
    import json
    entries = dict(load_tile_table())
    entries.update(_MEASURED)
    meta = dict(kernel_source_sha256=_table_hashes(), session=session,
                device=_device_tag(),
                note='keys: Builder._tune_key; values: [nb, nw, {"nb,nw": ms per launch, cold operands}]; (0, 0) = the library\'s own choice')
    with open(path, 'w') as fh:
        json.dump(dict(meta=meta, entries=entries), fh, indent=0, sort_keys=True)
    return len(entries)


def release_tuning_scratch():
    """Free the L2 / MALL flush buffers the tile measurement allocated (512 MiB per device): called when a plan build is finished."""
    _FLUSH.clear()


def _tile_neutral(a):
    """True when no output bit of this fp16-activation launch depends on its tile shape (see AUTOTUNE): no GroupNorm column sums, or column
    sums through the store-from-accumulators epilogue -- the host-side mirror of epi_direct_ok (csrc/epi_direct.h) for the 3x3 kernels."""
    if not a.stats_out:
        return True
    if a.taps == 1 or not a.out_f16:
        return False
    if a.res and (not a.res_f16 or a.cbias):
        return False
    if a.cbias and not (a.cbias_rows == 1 or (a.h * a.w) % 32 == 0):
        return False
    return True


def tune_report():
    """{layer signature: (nb, nw, {(nb, nw): ms})} measured so far in this process (tools / bench.py print it)."""
    return dict(_TUNE_CACHE)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


# Stand-ins for a tensor where a layer is known by its shape alone (Builder.shape_args): a dtype and a 16-byte-aligned address -- ds_conv_route
# asks of a pointer only whether it is set and aligned, and launches nothing
F32, F16 = (SimpleNamespace(dtype=d, data_ptr=lambda: 16) for d in (torch.float32, torch.float16))
HALO_IDS = (128, 256, 1284, 2565, 2568)          # ds_conv_kernel_id of the LDS-halo family (csrc/conv3x3_halo.hip)


class Op:
    """One launch: C entry point + argument tuple (struct by reference or scalars)."""
    __slots__ = ('fn', 'args', 'name', 'keep')

    def __init__(self, fn, args, name, keep=()):
        self.fn, self.args, self.name, self.keep = fn, args, name, keep


class Plan:
    """The launches of one network evaluation.  ``run`` hands the whole list to the library in ONE call (``ds_plan_run`` walks a
    native copy of the argument structs in C -- include/ds_engine.h "Native launch plans"); ``run_python`` issues the same launches
    one ctypes call at a time (instrumented replays in bench.py, and the reference for the native walk in the tests)."""

    def __init__(self):
        self.ops: List[Op] = []
        self.bufs: Dict[str, torch.Tensor] = {}
        self.keep: List[torch.Tensor] = []      # every workspace tensor the launch arguments point into
        self._native = None                     # (ds_plan*, number of ops it was built from)
        self.foreign = False                    # launches outside libdsamd in the list (Builder.fir_resample / zero_border): no native walk

    def run_python(self, stream):
        for op in self.ops:
            rc = op.fn(*op.args, stream)
            if rc:
                _lib.check(rc, op.name)

    def native(self):
        """The ds_plan handle of this op list (built on first use, rebuilt if launches were appended since)."""
        if self._native is None or self._native[1] != len(self.ops):
            self.close()
            self._native = (_native_plan(self.ops), len(self.ops))
        return self._native[0]

    def run(self, stream):
        if self.foreign:                        # ds_plan_run walks libdsamd's own launches only (the NCSN++ plans; the CLIP-score towers do the same)
            return self.run_python(stream)
        h = self.native()
        lib = _lib.load()
        rc = lib.ds_plan_run(h, stream)
        if rc:
            i = lib.ds_plan_last_failed(h)
            _lib.check(rc, self.ops[i].name if 0 <= i < len(self.ops) else 'ds_plan_run')

    def graph_capture(self, stream):
        """Record one run into a hipGraph owned by the native plan (ds_plan_graph_capture; `stream` must not be the default stream)."""
        if self.foreign:
            raise _lib.DsError('a plan with launches outside libdsamd has no native hipGraph: capture the call through graph.GraphedSampler')
        _lib.check(_lib.load().ds_plan_graph_capture(self.native(), stream), 'ds_plan_graph_capture')

    def graph_launch(self, stream):
        _lib.check(_lib.load().ds_plan_graph_launch(self.native(), stream), 'ds_plan_graph_launch')

    def close(self):
        if self._native is not None:
            _lib.load().ds_plan_destroy(self._native[0])
            self._native = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _native_plan(ops):
    """ds_plan_create + one ds_plan_add per launch (the library copies the argument structs)."""
    lib = _lib.load()
    by_ref = {id(lib.ds_conv2d_nhwc): _lib.DS_OP_CONV2D, id(lib.ds_gemm_nt_batched): _lib.DS_OP_GEMM, id(lib.ds_gn_stats): _lib.DS_OP_GN_STATS,
              id(lib.ds_norm_act): _lib.DS_OP_NORM_ACT, id(lib.ds_gn_finalize): _lib.DS_OP_GN_FINALIZE,
              id(lib.ds_attention): _lib.DS_OP_ATTENTION, id(lib.ds_attention_f16): _lib.DS_OP_ATTENTION_F16,
              id(lib.ds_attention_causal): _lib.DS_OP_ATTENTION_CAUSAL, id(_lib.affine_compose): _lib.DS_OP_AFFINE_COMPOSE}
    by_val = {id(lib.ds_layernorm_rows): (_lib.DS_OP_LAYERNORM, _lib.LayerNormArgs), id(lib.ds_geglu): (_lib.DS_OP_GEGLU, _lib.GegluArgs),
              id(lib.ds_noise_embed): (_lib.DS_OP_NOISE_EMBED, _lib.NoiseEmbedArgs), id(lib.ds_stem_im2col): (_lib.DS_OP_STEM_IM2COL, _lib.StemIm2colArgs),
              id(lib.ds_layernorm_rows_f16): (_lib.DS_OP_LAYERNORM_F16, _lib.LayerNormArgs),
              id(lib.ds_layernorm_rows_f16io): (_lib.DS_OP_LAYERNORM_F16IO, _lib.LayerNormArgs),
              id(lib.ds_token_embed): (_lib.DS_OP_TOKEN_EMBED, _lib.TokenEmbedArgs), id(lib.ds_quick_gelu): (_lib.DS_OP_QUICK_GELU, _lib.QuickGeluArgs)}
    h = C.c_void_p()
    _lib.check(lib.ds_plan_create(C.byref(h)), 'ds_plan_create')
    try:
        for op in ops:
            k = id(op.fn)
            if k in by_ref:
                code, st = by_ref[k], op.keep[0]              # the struct the launch passes by reference
            elif k in by_val:
                code, cls = by_val[k]
                st = cls(*op.args)
            else:
                raise _lib.DsError(f'launch {op.name!r} has no ds_plan op code')
            _lib.check(lib.ds_plan_add(h, code, C.byref(st), C.sizeof(st)), 'ds_plan_add ' + op.name)
    except Exception:
        lib.ds_plan_destroy(h)
        raise
    return h


class Builder:
    def __init__(self, device, conv_mode=0, w16_cache=None, autotune=True, invariant=False, batch=None):
        """w16_cache: dict owned by the engine (it outlives the per-batch plans): data_ptr of a row-padded fp32 1x1 / Linear weight
        -> its fp16 packing, made on first use when conv_mode == 1.  autotune: measure the tile shapes of the fp16-activation kernels
        (see AUTOTUNE above).  invariant: the batch-invariant mode: every convolution carries ds_conv_tune.invariant
        and no rule of this builder looks at the batch -- `batch` (images of the plan) tells the per-image row count of a Linear layer."""
        self.autotune = bool(autotune)
        self.invariant = bool(invariant)
        self.batch = batch
        self.coefs = None                   # {mu, A, B} planes of the GroupNorm emitters: allocated by the engine, which knows the widest layer
        self.free_list = []                 # alloc / free: base tensors (1-D) whose last reader has been emitted
        self.base = {}                      # data_ptr of a view handed out by alloc -> its base tensor
        self.w16_cache = w16_cache if w16_cache is not None else {}
        self.P = Plan()
        self.dev = device
        self.conv_mode = conv_mode          # 0 fp32 / 1 fp16 operands / 2 split-fp16 (fp32-emulated) in the eligible 3x3 convolutions
        self.lib = _lib.load()
        self.mean = self.rstd = None
        self.gn_partial = self.gn_counters = None
        self.stats_of: Dict[int, tuple] = {}   # data_ptr of an activation tensor -> (epilogue column-sum buffer, channels)
        self.ws = None                      # split-K scratch shared by every convolution of the plan (launches are serial)

    def new16(self, *shape):
        """fp16 workspace (activated tensors of the fp16-activation convolutions), owned by the plan like every other buffer."""
        t = torch.empty(*shape, dtype=torch.float16, device=self.dev)
        self.P.keep.append(t)
        return t

    def new(self, *shape, zero=False):
        # The argument structs hold raw pointers: the plan must own every tensor they point into, otherwise the
        # caching allocator would hand the memory to the next torch.empty() while the plan still uses it.
        t = (torch.zeros if zero else torch.empty)(*shape, dtype=torch.float32, device=self.dev)
        self.P.keep.append(t)
        return t

    def add(self, fn, args, name, keep=()):
        self.P.ops.append(Op(fn, args, name, keep))

    # ---- workspace recycling (launches of a plan are serial) ---------------------------------------------------------------------
    def alloc(self, rows, cols, f16=False):
        """[rows, cols] workspace: a freed buffer of the same dtype that is large enough (the smallest such), else a new plan-owned tensor."""
        dt = torch.float16 if f16 else torch.float32
        n = rows * cols
        fit = [t for t in self.free_list if t.dtype == dt and t.numel() >= n]
        if fit:
            b = min(fit, key=lambda t: t.numel())
            self.free_list = [t for t in self.free_list if t is not b]
        else:
            b = (self.new16 if f16 else self.new)(n)
        v = b[:n].view(rows, cols)
        self.base[v.data_ptr()] = b
        return v

    def free(self, *views):
        """Makes buffers of alloc() available to LATER launches: call it once the last reader is emitted."""
        for v in views:
            if v is None:
                continue
            b = self.base.pop(v.data_ptr(), None)
            if b is not None:
                self.stats_of.pop(v.data_ptr(), None)       # column sums of a recycled tensor describe nothing
                self.free_list.append(b)

    # ---- blocks ----------------------------------------------------------------------------------------------------------------------
    def widen(self, t, c, n, side, name):
        """`t`, or -- for an fp16 stream tensor -- an fp32 copy from alloc(), for a layer that has no fp16-activation kernel at this
        geometry.  The source is not freed: it may sit on a skip stack."""
        if t is None or t.dtype != torch.float16:
            return t
        wide = self.alloc(n * side * side, c)
        self.norm('apply', t, c, c, n, side, side, name + '.widen', use_stats=False, out=wide, out_ld=c)
        return wide

    def f16_conv_ok(self, n, side, cin, extra, cout, wide=False):
        """Does this stride-1 3x3 layer (`extra` = channels of a fused 1x1 skip projection) run on an fp16-activation kernel?  fp16 mode only;
        the library's answer for the shape on fp16 rows: conv3x3_f16dma (kernel ids 2566 / 2572), which ends at 64 pixels.
        wide: above 64 pixels the layer may take the patch kernel (csrc/conv3x3_f16wide.hip: 2575, and 2576 with the fused skip columns).  That
        kernel has one source and no fused normalisation, so only a caller that normalises such layers in a pass asks (the AutoencoderKL decoder;
        UNetEngine under `wide16`)."""
        return self.conv_mode == 1 and self.routes_to(self.shape_args(n, side, cin, cout, in_f16=True, ec0=extra), 2566, 2572, *((2575, 2576) if wide else ()))

    def gemm16_ok(self, rows, k, cout):
        """Does a 1x1 / Linear layer [rows][k] -> [rows][cout] on fp16 rows run on the fp16-activation GEMM (csrc/gemm_f16dma.hip)?"""
        return self.conv_mode == 1 and self.routes_to(self.shape_args(rows, 1, k, cout, taps=1, in_f16=True), 2567)

    def stride2_ok(self, n, side, cin, cout):
        """Does the stride-2 3x3 layer with `side` x `side` OUTPUT images run on fp16 rows (the gather form of the fp16-activation GEMM)?"""
        return self.conv_mode == 1 and self.routes_to(self.shape_args(n, side, cin, cout, in_f16=True, stride=2), 2571)

    def halo_ok(self, n, side):
        """Do fp32 3x3 layers on `side` x `side` images run on the LDS-halo kernels (the family that takes norm_coefs on fp32 rows)?"""
        return self.routes_to(self.shape_args(n, side, 32, 128), *HALO_IDS)

    def split_needs_pass(self, n, side, cin, ec0=0, ec1=0):
        """Split mode: the split-fp16 kernel (2563) takes this 3x3 layer on raw input but not with the fused input normalisation (8x8 images:
        four per tile, the normalisation planes are per image) -- both forms asked; the caller then normalises in a pass."""
        takes = lambda **kw: self.routes_to(self.shape_args(n, side, cin, 128, w16=True, ec0=ec0, ec1=ec1, **kw), 2563)
        return self.conv_mode == 2 and takes() and not takes(norm_coefs=F32, norm_act=DS_ACT_SILU)

    @staticmethod
    def fuses_norm16(mode, side, cout, x0, c0, x1=None, c1=0):
        """fp16-activation 3x3 layer: does the convolution normalise its own LDS halo (conv3x3_f16dma NORM: no pass, no materialised
        concatenation)?  Where `mode` (an engine's fuse_norm16) asks for it and every source is a raw fp16 tensor of whole 64-channel slabs."""
        raw = lambda t: t is None or t.dtype == torch.float16
        return bool(fuse_norm16_here(mode, side, cout) and raw(x0) and raw(x1) and c0 % 64 == 0 and c1 % 64 == 0)

    def gn_conv3x3(self, x0, c0, x1, c1, n, side, gamma, beta, wgt, bias, cout, out, out_ld, name, eps=1e-5, groups=32, w16=None, f16=False,
                   fuse_norm16=False, raw16=None, e16=None, **kw):
        """GroupNorm + SiLU + 3x3 conv over the concatenation [x0 | x1] (x1 may be None), `kw` to the convolution.  Three routes:
        f16 -- the caller found f16_conv_ok() for this layer and allocated `out` (and a block's intermediate tensor) to match: one pass
        writes the activated tensor as fp16 rows (and `raw16`, the raw fp16 copy a fused skip projection reads) and the convolution is the
        fp16-activation matrix kernel, or (fuses_norm16 under the mode `fuse_norm16`) the convolution normalises its own LDS halo on the raw sources.  `e16` = (tensor,
        channels) or (tensor, channels, tensor, channels): raw fp16 source(s) of a fused 1x1 skip projection; an fp16 `out` is stored as such.
        Otherwise fp32 activations: the normalisation rides in the LDS-halo kernel's loader where that kernel takes the shape, else a
        separate pass (also where the split-fp16 kernel takes the normalised tensor but not the fused normalisation: split_needs_pass)."""
        assert self.coefs is not None and self.coefs.numel() >= 3 * n * (c0 + c1), (name, 'the engine sizes Builder.coefs for its widest layer')
        cin = c0 + c1
        src = dict(x1=x1, c1=c1, ld1=c1)
        gn_stats = lambda **k: self.norm('stats', x0, c0, c0, n, side, side, name + '.gn.stats', groups=groups, eps=eps, **src, **k)
        gn_apply = lambda **k: self.norm('apply', x0, c0, c0, n, side, side, name + '.gn', groups=groups, eps=eps, act=DS_ACT_SILU, **src, **k)
        if f16:
            assert w16 is not None and self.conv_mode == 1, name
            ex = dict(zip(('e0', 'ec0', 'e1', 'ec1'), e16 or ()))
            kw = dict(kw, bias=bias, stats=True, w16=w16, in_f16=True, out_f16=(out.dtype == torch.float16))
            gn_stats(gamma=gamma, beta=beta, coefs=self.coefs)
            if raw16 is None and self.fuses_norm16(fuse_norm16, side, cout, x0, c0, x1, c1):
                self.conv(x0, c0, c0, n, side, side, wgt, cout, out, out_ld, 9, name, **src, norm_coefs=self.coefs, norm_act=DS_ACT_SILU, **ex, **kw)
                return
            # the pass form takes ONE raw source for a fused skip projection (the copy `raw16`, or the single fp16 input): two belong to the
            # fused form only, and a caller that decided otherwise must not lose the second one silently
            assert 'e1' not in ex, (name, 'two raw skip sources need the fused normalisation')
            a16 = self.alloc(n * side * side, cin, f16=True)
            gn_apply(use_stats=False, out=a16, out_ld=cin, out_f16=True, raw_out=raw16, raw_ld=cin, coefs=self.coefs, in_f16=(x0.dtype == torch.float16))
            self.conv(a16, cin, cin, n, side, side, wgt, cout, out, out_ld, 9, name, **ex, **kw)
            self.free(a16)
            return
        kw = dict(kw, bias=bias, stats=True, w16=w16)
        unfused_f16 = w16 is not None and self.split_needs_pass(n, side, cin, kw.get('ec0', 0), kw.get('ec1', 0))
        if self.halo_ok(n, side) and not unfused_f16 and x0.dtype == torch.float32 and (x1 is None or x1.dtype == torch.float32):
            gn_stats(gamma=gamma, beta=beta, coefs=self.coefs)
            self.conv(x0, c0, c0, n, side, side, wgt, cout, out, out_ld, 9, name, **src, norm_coefs=self.coefs, norm_act=DS_ACT_SILU, **kw)
        else:
            tmp = self.alloc(n * side * side, cin)
            gn_stats()
            gn_apply(gamma=gamma, beta=beta, out=tmp, out_ld=cin)
            self.conv(tmp, cin, cin, n, side, side, wgt, cout, out, out_ld, 9, name, **kw)
            self.free(tmp)

    def upsample_conv(self, x, cin, n, side_in, wgt, bias, cout, name, w16=None, wide=False, out_f32=False, free_src=False):
        """Nearest x2 of the raw tensor -> 3x3 conv; returns the output from alloc().  On the fp16-activation kernel (the pass writes fp16
        rows, the output joins the fp16 stream unless `out_f32`) where f16_conv_ok() (asked with `wide`) and there is an fp16 packing `w16`, else fp32.
        free_src: `x` is an alloc() buffer without another reader -- recycled as soon as the pass has read it."""
        side = 2 * side_in
        M = n * side * side
        f16 = w16 is not None and self.f16_conv_ok(n, side, cin, 0, cout, wide)
        up = self.alloc(M, cin, f16=f16)
        self.norm('apply', x, cin, cin, n, side_in, side_in, name + '.nearest', use_stats=False, resample=DS_RESAMPLE_UP, out=up, out_ld=cin,
                  out_f16=f16)
        if free_src:
            self.free(x)
        out = self.alloc(M, cout, f16=(f16 and not out_f32))
        self.conv(up, cin, cin, n, side, side, wgt, cout, out, cout, 9, name + '.conv', bias=bias, stats=True, w16=w16, in_f16=f16)
        self.free(up)
        return out

    def finish(self):
        """Ends a plan build: a missing kernel is an error now, not at the first run (P.kernel_ids: launch name -> ds_conv_kernel_id), and
        the tile measurement's 512 MiB flush buffer does not outlive the build."""
        P = self.P
        P.kernel_ids = {}
        for op in P.ops:
            if op.fn is self.lib.ds_conv2d_nhwc:
                kid = self.lib.ds_conv_kernel_id(C.byref(op.keep[0]))
                if kid < 0:
                    _lib.check(kid, f'plan: no kernel for {op.name}')
                P.kernel_ids[op.name] = kid
        release_tuning_scratch()
        return P

    def conv(self, x0, c0, ld0, n, h, w, wgt, cout, out, out_ld, taps, name, **kw):
        """One ds_conv2d_nhwc launch: the struct of conv_args (`kw`: its keywords)."""
        a = self.conv_args(x0, c0, ld0, n, h, w, wgt, cout, out, out_ld, taps, name, **kw)
        assert a.stride != 2 or not a.in_f16 or self.routes_to(a, 2571), name      # (stride 2 on fp16 rows: the caller asked stride2_ok())
        self._autotune(a, (x0,) + tuple(kw.get(k) if a.in_f16 else None for k in ('e0', 'x1', 'e1', 'norm_coefs')))
        self.add(self.lib.ds_conv2d_nhwc, (C.byref(a),), name, keep=(a,))

    def conv_args(self, x0, c0, ld0, n, h, w, wgt, cout, out, out_ld, taps, name, x1=None, c1=0, ld1=0, bias=None, cbias=None,
                  cbias_ld=0, cbias_rows=1, res=None, res_ld=0, scale=1.0, act=DS_ACT_NONE, norm_coefs=None, norm_act=DS_ACT_NONE,
                  e0=None, ec0=0, e1=None, ec1=0, stride=1, stats=False, w16=None, out_nchw=0, in_f16=False, out_f16=False, emb=False,
                  in_up2=False, wino=False, probe=False):
        """The ds_conv_args of a convolution: HOW a plan describes a layer to the library is known here alone; whether and how the library
        takes it is asked of route() with this struct.  probe: the struct is only shown to route() (up2_ok, wino_ok, shape_args) -- nothing
        plan-owned is allocated, no weight packed, no builder state touched; the split-K workspace is offered at a launch's capacity.
        stats=True: the epilogue also leaves the output's per-(64-row block, channel) sums for the consumer's GroupNorm
        (honoured when cout % 64 == 0; otherwise the consumer falls back to a ds_gn_stats pass).
        w16: (fp16 weights of the same layer, shift) -- ops.pack_conv_weight_f16 for the fp16-activation kernels (in_f16); in split mode
        ops.pack_conv_weight_split, used where the library takes this very launch with them, else the fp32 weights `wgt` are.  A 1x1 /
        Linear layer finds its own (linear_w16).
        in_f16: x0 (and e0) are fp16 NHWC tensors (leading dimensions in halfs) written by ``norm(..., out_f16=True)``: the
        fp16-activation kernel (csrc/conv3x3_f16dma.hip); needs w16.
        emb: a projection of the embedding path (one row per image or one shared row): in the invariant mode the row kernel at every row
        count (ds_conv_tune.invariant bit 1), so that both sigma forms and every batch give the same embedding rows.
        in_up2: the layer is conv3x3(nearest_x2(x0)) on the low-res rows x0 ([n][h/2][w/2]; h, w = the output size) with `wgt` =
        ops.pack_conv_weight_up2 (ds_conv_args.in_up2; fp32 only -- the caller asked up2_ok()).
        wino: the Winograd form of the layer, `wgt` = ops.pack_conv_weight_wino (ds_conv_args.wino; exact fp32 only -- the caller asked
        wino_ok())."""
        assert not wino or (w16 is None and not in_f16 and not in_up2 and stride == 1 and taps == 9 and not self.invariant), name
        assert not in_up2 or (w16 is None and not in_f16 and norm_coefs is None and not ec0 and res is None and stride == 1 and taps == 9), name
        lin16 = taps == 1 and x0.dtype == torch.float16
        if lin16:
            # 1x1 / Linear on an fp16 tensor (LayerNorm / GroupNorm pass / attention / GEGLU output in fp16 mode): csrc/gemm_f16dma.hip
            assert x1 is None and not ec0 and norm_coefs is None and not out_nchw and stride == 1
            in_f16 = True
        elif in_f16:
            # stride 2 (the LDM Downsample on the fp16 stream): the gather form of the fp16-activation GEMM; no extras, no residual
            # (round 5) stride 1 with norm_coefs: RAW fp16 sources, the kernel normalises its LDS halo; second sources x1 / e1 allowed then
            assert w16 is not None and taps == 9 and stride in (1, 2) and not out_nchw
            assert norm_coefs is not None or (x1 is None and e1 is None), name
            assert norm_coefs is None or (stride == 1 and all(t is None or t.dtype == torch.float16 for t in (x0, x1, e0, e1))), name
        if taps == 1 and w16 is None and (lin16 or (self.conv_mode == 1 and stride == 1 and norm_coefs is None and not ec0 and not ec1
                                                    and not out_nchw and (not self.invariant or self._rows_per_image_ok(n * h * w)))):
            w16 = self.linear_w16(wgt, n * h * w, c0, c1, dma=lin16, cout=cout)
            assert w16 is not None or not lin16, (name, 'no fp16-activation GEMM for this shape')
        f16 = w16 is not None and (in_f16 or taps == 1)
        # split mode: the split-fp16 weights where the library takes the finished struct with them (asked at the end); invariant: never at 8x8,
        # whose 256-pixel tiles hold four images, i.e. take only batches that are multiples of four
        split = w16 is not None and not f16 and self.conv_mode == 2 and taps == 9 and stride == 1 and not (self.invariant and (h * w) % 256)
        a = ConvArgs(ptr(x0), ptr(x1), c0, c1, ld0, ld1, n, h, w, taps, ptr(w16[0] if f16 or split else wgt), cout, ptr(bias), ptr(cbias), cbias_ld,
                     cbias_rows, ptr(res), res_ld, scale, act, ptr(out), out_ld, ptr(norm_coefs), norm_act, ptr(e0), ptr(e1),
                     ec0, ec1, ec0, ec1, stride)
        if self.ws is None and not probe:
            self.ws = self.new(SPLITK_WORKSPACE_FLOATS)
        a.workspace, a.workspace_floats = ptr(F32 if self.ws is None else self.ws), SPLITK_WORKSPACE_FLOATS
        a.out_nchw = out_nchw               # network output written channel-planar (NCHW) by the epilogue
        a.wgt_f16, a.wgt_shift = (self.conv_mode, w16[1]) if f16 or split else (0, 0)
        a.in_f16, a.in_up2, a.wino = int(bool(in_f16)), int(bool(in_up2)), int(bool(wino))
        if self.invariant:
            a.tune.invariant = 3 if emb else 1
        if in_f16 and ec0 and taps == 9 and stride == 1 and w > 64:
            a.tune.variant = WIDE_EXTRA          # the patch kernel's appended 1x1 slabs (kernel id 2576) are asked for (ds_conv_tune.variant bit 17)
        if out_f16 or out.dtype == torch.float16:          # fp16 output rows: conv0 outputs, projection operands, the fp16 residual stream
            assert in_f16 and out.dtype == torch.float16 and cout % 64 == 0, name
            a.out_f16 = 1
        if res is not None and res.dtype == torch.float16:  # the residual operand is a tensor of the fp16 stream
            assert in_f16, name
            a.res_f16 = 1
        if not probe:
            self.stats_of.pop(out.data_ptr(), None)
        if stats and cout % 64 == 0 and out_ld == cout:
            sums = out if probe else self.new(-(-(n * h * w) // 64) * 2 * cout)       # (a probe: any 16-byte-aligned address)
            a.stats_out = ptr(sums)
            if not probe:
                self.stats_of[out.data_ptr()] = (sums, cout)
        if split and not self.routes_to(a, 2563):
            a.wgt, a.wgt_f16, a.wgt_shift = ptr(wgt), 0, 0
        return a

    def route(self, a):
        """The library's answer to a ds_conv_args: (return code, ConvRouteInfo) of ds_conv_route -- host logic only, nothing is launched.
        Every question this builder or an engine has about a convolution is put here."""
        info = ConvRouteInfo()
        return self.lib.ds_conv_route(C.byref(a), C.byref(info)), info

    def routes_to(self, a, *kernel_ids):
        rc, info = self.route(a)
        return rc == 0 and info.kernel_id in kernel_ids

    def shape_args(self, n, side, c0, cout, taps=9, in_f16=False, w16=False, c1=0, ec0=0, ec1=0, **kw):
        """conv_args, in probe form, of a layer known by its shape alone -- the block-level decisions, taken before buffers exist: `n` images
        of side x side pixels (a Linear layer: n rows, side 1), dense rows, an fp16 packing if in_f16 or w16, and no bias, residual,
        statistics or norm_coefs unless `kw` names one."""
        t = F16 if in_f16 else F32
        return self.conv_args(t, c0, c0, n, side, side, F32, cout, F32, cout, taps, 'shape', x1=t if c1 else None, c1=c1, ld1=c1,
                              e0=t if ec0 else None, ec0=ec0, e1=t if ec1 else None, ec1=ec1, w16=(F32, 0) if in_f16 or w16 else None,
                              in_f16=in_f16, probe=True, **kw)

    def up2_ok(self, x0, c0, ld0, n, h, w, wgt, cout, out, out_ld, **kw):
        """Does the library take this layer as an upsampled-input convolution (ds_conv_args.in_up2)?  The route of the struct
        conv(..., in_up2=True, **kw) would launch.  On the batch-invariant route the answer depends on the layer alone (the 256 x 192
        tiles, the one shape whose use follows the tile count, are off there)."""
        return self.route(self.conv_args(x0, c0, ld0, n, h, w, wgt, cout, out, out_ld, 9, 'up2_ok', in_up2=True, probe=True, **kw))[0] == 0

    def wino_ok(self, x0, c0, ld0, n, h, w, wgt, cout, out, out_ld, **kw):
        """Does the library take this layer in the Winograd form (ds_conv_args.wino)?  The route of the struct conv(..., wino=True, **kw)
        would launch, split-K workspace included (the split-K decision is part of the answer): yes exactly where the direct form would
        run on the 256 x 256 tiles without split-K."""
        if self.invariant or self.conv_mode:
            return False
        rc, info = self.route(self.conv_args(x0, c0, ld0, n, h, w, wgt, cout, out, out_ld, 9, 'wino_ok', wino=True, probe=True, **kw))
        return rc == 0 and info.wino == 1

    @staticmethod
    def _tune_key(a, stride):
        """Layer signature of an fp16-activation launch: everything the best tile shape can depend on (shape, epilogue work, row pitches,
        whether a split-K workspace is offered)."""
        t = a.tune
        return (a.taps, stride, a.n, a.h, a.w, a.c0, a.ec0, a.cout, a.act, a.out_f16, a.res_f16, bool(a.res), bool(a.cbias), bool(a.bias),
                bool(a.stats_out), t.splits, a.ld0, a.out_ld, bool(a.workspace), bool(a.norm_coefs), a.c1, a.ec1)

    def _autotune(self, a, inputs):
        """Fill a.tune.f16dma_nb / f16dma_nw of an fp16-activation launch with the measured best (module docstring of AUTOTUNE): from the
        persisted table, else measured now."""
        t = a.tune
        if not (AUTOTUNE and self.autotune and a.in_f16) or not inputs[0].is_cuda or not _tile_neutral(a):
            return
        if t.mode or t.variant or t.f16dma_nb or t.f16dma_nw or t.ablate:
            return
        stride = a.stride if a.stride else 1
        key = self._tune_key(a, stride)
        dkey = (inputs[0].device.index, key)
        hit = _TUNE_CACHE.get(dkey)
        if hit is None:
            row = load_tile_table().get(str(key))
            if row is not None:          # a table hit needs no launches: fine inside a stream capture too
                hit = (int(row[0]), int(row[1]), {tuple(int(v) for v in k.split(',')): ms for k, ms in row[2].items()})
            elif torch.cuda.is_current_stream_capturing():
                return                   # nothing is measured during a capture: the library's own choice
            else:
                hit = self._measure_tiles(a, inputs, stride)
                _MEASURED[str(key)] = [hit[0], hit[1], {'%d,%d' % k: round(ms, 5) for k, ms in hit[2].items()}]
            _TUNE_CACHE[dkey] = hit
        t.f16dma_nb, t.f16dma_nw = hit[0], hit[1]

    def _measure_tiles(self, a, inputs, stride):
        """Time the launch under every tile-shape candidate.  Side effects, all confined: the launch's fp16 INPUT buffers are refilled with
        random values from a PRIVATE generator (the default CUDA generator is untouched; every plan rewrites its activation buffers on
        each run before reading them, so nothing downstream sees the fill), and its output / statistics / workspace are written as any
        run of the plan writes them."""
        if a.taps == 1:                       # csrc/gemm_f16dma.hip: 128-row tiles hold at most 192 columns; the GEGLU gate pairs even widths
            cands = [(nb, nw) for nw in (4, 8) for nb in ((2, 4) if a.act == _lib.DS_ACT_GEGLU else (1, 2, 3, 4)) if nw == 8 or nb <= 3]
        else:                                 # 3x3 (stride 1: conv3x3_f16dma.hip, 256 columns only on 16- / 32-column images; stride 2: the gather GEMM)
            cands = [(nb, 8) for nb in (1, 2, 3, 4) if nb < 4 or stride == 2 or (a.w in (16, 32) and not a.norm_coefs)]
        cands = [c for c in cands if 64 * c[0] <= -(-a.cout // 64) * 64]
        dev = inputs[0].device
        gen = torch.Generator(device=dev)
        gen.manual_seed(0x5eed)
        for x in inputs[:4]:
            if x is not None and x.dtype == torch.float16:
                x.normal_(generator=gen)
        if len(inputs) > 4 and inputs[4] is not None:          # fused input normalisation: finite {mu, A, B} planes (the next ds_gn_finalize rewrites them)
            inputs[4].normal_(generator=gen)
        if dev.index not in _FLUSH:
            _FLUSH[dev.index] = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
        flush = _FLUSH[dev.index]
        st = _lib.stream_ptr()
        t = a.tune
        times = {}
        for nb, nw in [(0, 0)] + cands + [(0, 0)]:
            t.f16dma_nb, t.f16dma_nw = nb, nw
            if self.lib.ds_conv2d_nhwc(C.byref(a), st):
                continue
            ms = []
            for _ in range(3):
                flush.fill_(1)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                self.lib.ds_conv2d_nhwc(C.byref(a), st)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            times[(nb, nw)] = min(sorted(ms)[1], times.get((nb, nw), float('inf')))
        t.f16dma_nb, t.f16dma_nw = 0, 0
        if (0, 0) not in times:
            return 0, 0, times
        best = min(times, key=times.get)
        if times[best] > 0.97 * times[(0, 0)]:
            best = (0, 0)
        return best[0], best[1], times

    def linear_w16(self, wgt, rows, c0, c1, dma=False, cout=0):
        """w16 of a 1x1 / Linear layer in fp16 mode: (the fp16 packing of `wgt`, cached per weight tensor; shift 0) where the library takes the
        shape with it -- dma: on fp16 rows (gemm16_ok), else on fp32 rows, rounded while staged (gemm_f16_kernel, kernel id 2564) -- else None."""
        ok = self.gemm16_ok(rows, c0, cout) if dma else self.routes_to(self.shape_args(rows, 1, c0, 128, taps=1, w16=True, c1=c1), 2564)
        if wgt.dtype != torch.float32 or wgt.dim() != 2 or wgt.shape[0] % 128 or wgt.shape[1] != c0 + c1 or not ok:
            return None
        key = wgt.data_ptr()
        if key not in self.w16_cache:
            from .ops import pack_linear_weight_f16
            self.w16_cache[key] = (pack_linear_weight_f16(wgt), wgt)       # keep the source alive: its address is the key
        return self.w16_cache[key][0], 0

    def _rows_per_image_ok(self, rows):
        """Invariant mode: may a 1x1 / Linear layer over `rows` rows take the fp16-operand GEMM (whole 256-row tiles)?  Only where every
        batch gives it whole tiles -- a multiple of 256 rows per image -- so the choice never depends on the batch."""
        return bool(self.batch) and rows % self.batch == 0 and (rows // self.batch) % 256 == 0

    def linear(self, x, k, rows, wgt, cout, out, name, ldx=None, out_ld=None, **kw):
        """out[rows, cout] = x[rows, k] W^T (+bias +res ...): a 1x1 'convolution' over rows."""
        self.conv(x, k, ldx or k, rows, 1, 1, wgt, cout, out, out_ld or cout, 1, name, **kw)

    def norm(self, kind, x0, c0, ld0, n, h, w, name, x1=None, c1=0, ld1=0, groups=1, eps=1e-5, use_stats=True, gamma=None,
             beta=None, scale=None, shift=None, ss_ld=0, ss_rows=1, act=DS_ACT_NONE, resample=DS_RESAMPLE_NONE, out=None,
             out_ld=0, coefs=None, out_f16=False, raw_out=None, raw_ld=0, in_f16=False):
        if use_stats and (self.mean is None or self.mean.numel() < n * 64):
            self.mean, self.rstd = self.new(n * 64), self.new(n * 64)
        if kind == 'stats':
            # statistics already left behind by the producing convolutions' epilogues?  Then only finalise them.
            s0 = self.stats_of.get(x0.data_ptr())
            s1 = self.stats_of.get(x1.data_ptr()) if x1 is not None else None
            if s0 is not None and s0[1] == c0 == ld0 and (x1 is None or (s1 is not None and s1[1] == c1 == ld1)) and (h * w) % 64 == 0:
                f = GnFinalizeArgs(ptr(s0[0]), ptr(s1[0]) if s1 else None, c0, c1, n, h * w, groups, eps, ptr(gamma), ptr(beta),
                                   ptr(scale), ptr(shift), ss_ld, ss_rows, ptr(self.mean), ptr(self.rstd), ptr(coefs))
                self.add(self.lib.ds_gn_finalize, (C.byref(f),), name + '.finalize', keep=(f,))
                return
        a = NormArgs(ptr(x0), ptr(x1), c0, c1, ld0, ld1, n, h, w, groups, eps, ptr(self.mean) if use_stats else None,
                     ptr(self.rstd) if use_stats else None, ptr(gamma), ptr(beta), ptr(scale), ptr(shift), ss_ld, ss_rows, act,
                     resample, ptr(out), out_ld, ptr(coefs))
        # fp16 sources (conv0 outputs, tensors of the fp16 residual stream) are recognised by their dtype: bit 0 = x0, bit 1 = x1
        a.in_f16 = (1 if x0.dtype == torch.float16 else 0) | (2 if x1 is not None and x1.dtype == torch.float16 else 0)
        assert not in_f16 or (a.in_f16 & 1), name
        if out_f16:
            assert kind == 'apply' and out.dtype == torch.float16 and (raw_out is None or raw_out.dtype == torch.float16)
            a.out_f16, a.raw_out, a.raw_ld = 1, ptr(raw_out), raw_ld
            self._fold_finalize(a, coefs)
        if kind == 'stats' and n < 256 and not self.invariant:       # (invariant: one workgroup per image at every batch)
            if self.gn_partial is None or self.gn_counters.numel() < n:
                self.gn_partial = torch.empty(n * _lib.DS_GN_MAX_CHUNKS * 128, dtype=torch.float64, device=self.dev)
                self.gn_counters = torch.zeros(n, dtype=torch.int32, device=self.dev)
                self.P.keep += [self.gn_partial, self.gn_counters]
            a.partial, a.counters = ptr(self.gn_partial), ptr(self.gn_counters)
        self.add(self.lib.ds_gn_stats if kind == 'stats' else self.lib.ds_norm_act, (C.byref(a),), name, keep=(a,))

    def _fold_finalize(self, a, coefs):
        """Round 6: an fp16 pass whose {mu, A, B} planes come from the ds_gn_finalize launch right in front of it computes the statistics itself
        (ds_norm_args.stats0 / stats1, csrc/norm_act.hip norm_act16_kernel<FIN>) -- the finalize launch (~6 us each; 950 per ImageNet-64 sampler
        call in round 5) is dropped from the plan.  Only where every workgroup can afford to re-read the image's column sums: images of at most
        32 x 32 pixels, on the 16-byte form of the pass (the host-side mirror of norm16_ok + the FIN checks of ds_norm_act).  The planes are not
        written then: nothing else may read them (the engines' passes are their only readers).  Same arithmetic, same coefficient expressions
        (gn_coefs): the plans agree bit for bit (tests/test_hip_fp16.py, tools/ab_norm.py).
        OFF by default (DS_FOLD_GN_FINALIZE=1 / plan.FOLD_FINALIZE switch it on): built as VERDICT r5 item 3 asked and MEASURED a wash -- the
        launch saved is paid back by every workgroup's own reduction of the column sums: ImageNet-64 fp16 322.3 (two launches) vs 320.1 images/s
        (folded), SD-1.5 fp16 78.1 vs 77.3 (session r9d, alternating; profiles/r6_norm_pass_ab.txt)."""
        if not FOLD_FINALIZE or coefs is None or not self.P.ops:
            return
        prev = self.P.ops[-1]
        if prev.fn is not self.lib.ds_gn_finalize:
            return
        f = prev.keep[0]
        C_ = a.c0 + a.c1
        hw = a.h * a.w
        if f.coefs != coefs.data_ptr() or (f.c0, f.c1, f.n, f.hw) != (a.c0, a.c1, a.n, hw):
            return
        all16 = (a.in_f16 & 1) and (not a.c1 or (a.in_f16 & 2))
        if not (all16 and a.resample == DS_RESAMPLE_NONE and hw % 64 == 0 and hw <= 1024 and C_ % 8 == 0 and a.c0 % 8 == 0 and C_ <= 4096
                and a.ld0 % 8 == 0 and (not a.c1 or a.ld1 % 8 == 0) and a.out_ld % 8 == 0 and (not a.raw_out or a.raw_ld % 8 == 0)):
            return
        self.P.ops.pop()
        a.stats0, a.stats1, a.coefs = f.stats0, f.stats1, None
        a.groups, a.eps = f.groups, f.eps
        a.gamma, a.beta, a.scale, a.shift, a.ss_ld, a.ss_rows = f.gamma, f.beta, f.scale, f.shift, f.ss_ld, f.ss_rows

    def gemm(self, a_, lda, b_, ldb, c_, ldc, m, n, k, name, batch=1, heads=1, a_bs=0, a_hs=0, b_bs=0, b_hs=0, c_bs=0, c_hs=0,
             alpha=1.0, rowbias=None, colbias=None):
        g = GemmArgs(ptr(a_), lda, a_bs, a_hs, ptr(b_), ldb, b_bs, b_hs, ptr(c_), ldc, c_bs, c_hs, m, n, k, batch, heads, alpha,
                     ptr(rowbias), ptr(colbias), DS_ACT_NONE)
        self.add(self.lib.ds_gemm_nt_batched, (C.byref(g),), name, keep=(g,))

    def attention(self, q, k, v, out, name, *, batch, heads, sq, skv, d, ldq, ldk, ldv, ldo, q_bs, k_bs, v_bs, o_bs, scale):
        a = AttnArgs(ptr(q), ptr(k), ptr(v), ptr(out), ldq, ldk, ldv, ldo, q_bs, k_bs, v_bs, o_bs, batch, heads, sq, skv, d, scale)
        f16 = self.conv_mode == 1 and self.lib.ds_attention_f16_supported(d)      # fp16 mode: fp16-operand kernel where it covers the head size
        if out.dtype == torch.float16:
            assert f16, 'fp16 attention output needs the fp16-operand kernel'
            a.out_f16 = 1
        # fp16 q / k / v (the projections' outputs in the fp16 stream) are recognised by their dtype: bit 0 = q, bit 1 = k and v
        a.in_f16 = (1 if q.dtype == torch.float16 else 0) | (2 if k.dtype == torch.float16 else 0)
        assert k.dtype == v.dtype and (not a.in_f16 or f16), name
        if self.invariant and not f16 and d % 128 == 0:
            a.variant = 2           # invariant: the channel-split block at every batch (ds_attention_variant)
        self.add(self.lib.ds_attention_f16 if f16 else self.lib.ds_attention, (C.byref(a),), name, keep=(a,))

    def attention_causal(self, q, k, v, out, name, *, batch, heads, s, d, ldq, ldk, ldv, ldo, q_bs, k_bs, v_bs, o_bs, scale):
        """Causal self-attention over `s` tokens (csrc/text_encoder.hip: the CLIP text encoder); fp32 in every mode."""
        assert all(t.dtype == torch.float32 for t in (q, k, v, out)), name
        if not self.lib.ds_attention_causal_supported(d, s):
            raise NotImplementedError(f'{name}: no causal attention kernel for head size {d} over {s} tokens')
        a = AttnArgs(ptr(q), ptr(k), ptr(v), ptr(out), ldq, ldk, ldv, ldo, q_bs, k_bs, v_bs, o_bs, batch, heads, s, s, d, scale)
        self.add(self.lib.ds_attention_causal, (C.byref(a),), name, keep=(a,))

    def affine_compose(self, aff, ld, rows, width, step, pairs, name):
        """Step-conditioned adaptive blocks: the step row's (scale, shift) folded in place into every row's pairs of `aff` [rows][ld]
        (ds_affine_compose_args; `pairs` = int32 [groups][2] device table of four-column groups).  A plan operation of the library."""
        assert aff.dtype == step.dtype == torch.float32 and pairs.dtype == torch.int32 and pairs.dim() == 2 and pairs.shape[1] == 2, name
        a = _lib.AffineComposeArgs(ptr(aff), ld, rows, width, ptr(step), ptr(pairs), pairs.shape[0])
        self.add(_lib.affine_compose, (C.byref(a),), name, keep=(a,))

    # ---- launches of libdsmetrics (csrc/metrics/fir_resample.hip): the plan then runs through Plan.run_python -----------------------------
    def fir_resample(self, x, ld_x, n, h, w, c, out, out_ld, name, up=False, pad=1, taps=(1, 3, 3, 1), bias=None, res=None, res_ld=0, scale=1.0):
        """out = (fir(x) + bias + res) * scale over fp32 NHWC rows: the depthwise 4-tap filter `taps` as a stride-2 down (padding `pad`) or a
        x2 up (dsm_fir_args; h, w = the INPUT size)."""
        from . import _metrics_lib as ML
        assert len(taps) == 4 and all(t.dtype == torch.float32 for t in (x, out)), name
        a = ML.DsmFirArgs(ptr(x), ld_x, n, h, w, c, 1 if up else 0, pad, (C.c_float * 4)(*[float(t) for t in taps]), ptr(bias), ptr(res), res_ld,
                          scale, ptr(out), out_ld)
        mlib = ML.load()
        if not mlib.dsm_fir_resample_supported(a.up, a.pad, h, w, c):
            raise NotImplementedError(f'{name}: no FIR resampling kernel for up={a.up} pad={pad} on {h} x {w} x {c}')
        self.stats_of.pop(out.data_ptr(), None)
        self.P.foreign = True
        self.add(mlib.dsm_fir_resample, (C.byref(a),), name, keep=(a,))

    def zero_border(self, x, out, outer, h, w, inner, p, name):
        """out [outer][h + 2p][w + 2p][inner] = x [outer][h][w][inner] inside a ring of zeros (dsm_zero_border)."""
        from . import _metrics_lib as ML
        assert x.dtype == out.dtype == torch.float32 and out.numel() >= outer * (h + 2 * p) * (w + 2 * p) * inner, name
        self.stats_of.pop(out.data_ptr(), None)
        self.P.foreign = True
        self.add(ML.load().dsm_zero_border, (ptr(x), ptr(out), outer, h, w, inner, p), name)

    def token_embed(self, tokens, tok_table, pos_table, out, out_ld, batch, seq, width, vocab, name):
        assert tokens.dtype == torch.int32 and tokens.numel() == batch * seq, name
        self.add(self.lib.ds_token_embed, (ptr(tokens), ptr(tok_table), ptr(pos_table), ptr(out), out_ld, batch, seq, width, vocab), name)

    def quick_gelu(self, x, ldx, y, ldy, rows, cols, name):
        self.add(self.lib.ds_quick_gelu, (ptr(x), ldx, ptr(y), ldy, rows, cols), name)

    def layernorm(self, x, ldx, gamma, beta, eps, y, ldy, rows, cols, name):
        if x.dtype == torch.float16:          # a tensor of the fp16 residual stream
            assert y.dtype == torch.float16, name
            fn = self.lib.ds_layernorm_rows_f16io
        else:
            fn = self.lib.ds_layernorm_rows_f16 if y.dtype == torch.float16 else self.lib.ds_layernorm_rows
        self.add(fn, (ptr(x), ldx, ptr(gamma), ptr(beta), eps, ptr(y), ldy, rows, cols), name)

    def geglu(self, x, ldx, y, ldy, rows, inner, name):
        self.add(self.lib.ds_geglu, (ptr(x), ldx, ptr(y), ldy, rows, inner), name)
