"""Exact references, test data, the case table and the argument builder for the convolution / GEMM family: ds_conv2d_nhwc (every kernel id
of csrc/gemm_conv.hip's route, the Winograd form, split-K and its reduce kernels) and ds_gemm_nt_batched.

numpy / torch on the CPU only; the one library call is the host-only ds_conv_route (tests/test_conv_refs_cpu.py proves the table's coverage
with it).  tests/test_hip_conv_kernels.py runs every case on the GPU.  U, SECOND, rne16, inside, worst and the SiLU constants are those of
tests/_norm_refs.py; no constant is fixed here.

FAMILY A: INTEGER OPERANDS, DENSE WEIGHTS.  Activations, weights, bias, per-image bias, residual and the {mu, A, B} planes (norm_act NONE)
are integers (wide activations: integers times 2^-2), out_scale is a power of two.  Every product and every partial sum in ANY order is then a
multiple of the unit 2^-2 below 2^24 units: exact in fp32, whatever the tile shape, the split-K factor or the Winograd transform.  The
criterion is EQUALITY with the fp64 evaluation (as numbers: -0 equals +0); with out_f16 the expected value is rne16 of the exact one and
the column statistics are those of the rounded values.  `conditions` states what makes this true and the CPU test asserts it on the actual
data of every case:
  * sum |in| |w| + |bias| + |cbias| + |res| < 2^24 units per output (in = the normalised input); the Winograd form in addition
    9 max_position sum_c |U| |V| + the appended 1x1 sum < 2^24 units (V = B^T d B has integer entries up to 4 |d|, U = G g G^T is integer for
    weights that are multiples of 4, Y = A^T M A adds at most nine M);
  * every operand is exactly representable in the format the kernel family stages it in: fp32 (exact-fp32 kernels), fp16 hi + lo with ONE
    side's lo = 0 (split-fp16: the dropped lo * lo term would make the product inexact; each case runs twice, wide activations with
    fp16-exact weights and the roles swapped), fp16 (the fp16 families; the fused normalisation of kernel id 2572 rounds its result to
    fp16, which the reference restates with rne16);
  * in every K slab some operand is NOT representable in the next narrower format (fp32 kernels: fp16; split-fp16: fp16 on the wide
    side; fp16 families: bfloat16) -- an operand path narrower than claimed changes the result; and the sums go far beyond 2048, so an
    fp16 accumulator shows.  Cases that request stats_out are the exception: a sum of squares of 64 outputs below 2^24 needs |out| < 2^9,
    which a 13-bit operand excludes; they use magnitudes <= 3 (`mag = small`) and every kernel id has wide cases besides;
  * where stats_out is checked every 64-row column sum and sum of squares is < 2^24 units: the statistics are exact too.

FAMILY B: SELECTOR WEIGHTS, REAL-VALUED INPUTS: the fused input normalisation with SiLU, the output SiLU, randn activations, out_scale
0.7071.  Every output column has exactly ONE non-zero weight, +-2^j (|j| <= 2), at its own (tap, channel) -- or at a channel of the appended
1x1 columns; all other products are exact zeros, so acc[m, co] = +-2^j in(m + tap, c) exactly, in any order and under split-K (the other
splits' planes are exact zeros).  What is left, per output element (derivation: `epilogue` / `epi_process` / epilogue32 of
csrc/igemm_common.h, its scalar fallback, splitk_reduce_kernel and splitk_reduce_f16_kernel of gemm_conv.hip, gemv_rows_kernel -- all the
same chain v = acc * acc_scale (a power of two: exact); v += bias; v += cbias; v += res; v *= out_scale; ds_silu; fp16 rounding):
  * in: raw input: exact.  Fused normalisation t = (x - mu) A + B (conv3x3_halo.hip halo_store, as written or contracted to an fma;
    conv3x3_halo2.hip: fmaf(x - mu, A, B)): U |x - mu| |A| for the subtraction, U |x - mu| |A| for an uncontracted product, U |t| for
    the sum; SiLU as below.  Split-fp16 staging: hi + lo with lo = fp16(v - hi), 2^-11 |lo| <= 2^-22 |v| and (fp16 subnormals) 2^-25
    absolute.  fp16 staging (the fp16 families): the staged value is one of rne16(in - b), rne16(in + b) (DESIGN.md's rule: fp16 gets
    no tolerance of its own; the two coincide except at a rounding boundary) -- the reference is evaluated on both and the output must
    be inside the bound of one of them;
  * three additions, each U |partial sum|, and one product, U |v| (counted also where out_scale is 1);
  * SiLU: SILU_LIP e_v + (K_SILU + silu_exp_term(v)) U |silu(v)| + SILU_ABS (tests/_norm_refs.py);
  * fp16 output: inside(out16=True).
First order in U, times SECOND.  The selectors of a case visit every tap and every channel position inside a slab of the kernel's slab
width (32 channels; 64 for the fp16 families), both sources where there are two, and the appended columns (`selector_visits`); the
thin-output kernel (at most four columns) needs several launches for that (`rounds`).
The Winograd form has no family B: its input transform B^T d B rounds on real-valued data, so a selector does not isolate one term
(tests/test_hip_wino.py keeps the randn comparison of tests/_conv_randn.py); DS_ACT_GEGLU stays with its own tests.

ds_gemm_nt_batched: GEMM_CASES with family-A data (exact) and, under SiLU, the family-B bound on integer operands
(alpha * acc exact; + rowbias, + colbias: two roundings; SiLU).
"""
import ctypes as C
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from _norm_refs import U, SECOND, K_SILU, SILU_ABS, SILU_LIP, silu_exp_term, rne16, inside, worst  # noqa: F401

f32, f16, f64 = np.float32, np.float16, np.float64
NAN = float('nan')
B_SCALE = 0.7071          # family B's out_scale where a case asks for one (the networks' skip_scale, not a power of two)
UNIT = 0.25               # family A: activations are integers times 2^-2

KERNEL_IDS = (0, 128, 256, 1284, 2561, 2563, 2564, 2565, 2566, 2567, 2568, 2570, 2571, 2572, 2573, 2575)

_FIELDS = dict(
    c1=0, taps=9, ec0=0, ec1=0, stride=1, up2=0, wino=0,
    kind='f32',           # f32: exact fp32 | split: wgt_f16 = 2 | f16w: wgt_f16 = 1 on fp32 rows (2564) | f16: in_f16
    out16=0, res16=0, nchw=0,
    norm=0,               # 0 none, 1 {mu, A, B} planes with norm_act NONE, 2 with SiLU (family B)
    bias=1,               # 0 NULL, 1 given, 2 given through a pointer off 16 bytes (scalar epilogue)
    cbias=0,              # 0 NULL, 1 one row (cbias_rows = 1), 2 n rows
    res=0, scale=1.0,     # scale: a power of two (family A) / B_SCALE where != 1 (family B)
    act=0,
    stats=0,              # 1: stats_out, sums and sums of squares exact; 2 (mag = mid): the fp16 rounding is not trivial, sums exact, squares bounded
    ws=0,                 # > 0: a workspace of exactly ws * M * cout floats
    out_pad=4, res_pad=4,  # out_ld = ceil4(cout) + out_pad (fp16 rows: ceil8 + 2 * out_pad); an odd pad makes the leading dimension % 4 != 0
    tune=(),              # ((field, value), ...) of ds_conv_tune
    kid=0, splits=1, widths=(),   # the route the case must take
    fam='A',              # 'A', 'B' or 'AB'
    mag='wide',           # family A magnitudes: wide / small (see above)
    rounds=1,             # family B: launches with different selectors (outputs of a few columns cannot visit a slab in one)
)
Case = namedtuple('Case', ('name', 'n', 'h', 'w', 'c0', 'cout') + tuple(_FIELDS))


def _c(name, n, h, w, c0, cout, **kw):
    bad = set(kw) - set(_FIELDS)
    assert not bad, bad
    f = dict(_FIELDS, **kw)
    f['tune'] = tuple(sorted(dict(f['tune']).items()))
    return Case(name, n, h, w, c0, cout, **f)


T256 = dict(mode=256)
T2565 = dict(mode=256, variant=6)
T2568 = dict(mode=256, variant=16384)
V2048 = dict(variant=2048)

# h, w: the OUTPUT size (stride 2 reads 2h x 2w, up2 reads h/2 x w/2).  Neighbours differ in one option.
CASES = (
    # ---- generic gather kernel (0)
    _c('g_1x1_ragged', 3, 5, 7, 32, 70, taps=1, kid=0, fam='AB'),
    _c('g_1x1_ragged_nobias_res', 3, 5, 7, 32, 70, taps=1, bias=0, res=1, kid=0),
    _c('g_1x1_ragged_outld', 3, 5, 7, 32, 70, taps=1, out_pad=1, cbias=2, kid=0),                   # out_ld % 4 != 0: scalar epilogue
    _c('g_3x3', 2, 8, 8, 32, 64, tune=dict(mode=1), cbias=2, res=1, scale=0.5, kid=0, fam='AB'),
    _c('g_3x3_cb1_act', 2, 8, 8, 32, 64, tune=dict(mode=1), cbias=1, res=1, scale=B_SCALE, act=1, kid=0, fam='B'),
    _c('g_3x3_stats', 2, 8, 8, 32, 64, tune=dict(mode=1), cbias=1, stats=1, mag='small', kid=0),
    _c('g_3x3_resld', 2, 8, 8, 32, 64, tune=dict(mode=1), res=1, res_pad=1, kid=0),                 # res_ld % 4 != 0: scalar epilogue
    _c('g_stride2', 2, 4, 4, 32, 64, stride=2, kid=0, fam='AB'),
    _c('g_splitk', 2, 3, 3, 128, 7, ws=12, kid=0, splits=12, res=1, cbias=2, scale=2.0),
    _c('g_splitk_stats', 2, 8, 8, 128, 64, tune=dict(mode=1, splits=4), ws=4, stats=1, mag='small', kid=0, splits=4),
    _c('g_nchw', 2, 8, 8, 32, 5, tune=dict(mode=1), nchw=1, kid=0),
    # ---- LDS-halo kernel, 128-pixel tiles on four waves (128)
    _c('h128', 3, 8, 8, 32, 96, kid=128, fam='AB'),
    _c('h128_full', 3, 8, 8, 32, 96, cbias=2, res=1, scale=0.5, norm=1, kid=128, fam='AB'),
    _c('h128_b', 3, 8, 8, 32, 96, cbias=1, res=1, scale=B_SCALE, norm=2, act=1, bias=0, kid=128, fam='B'),
    _c('h128_multi_image', 5, 4, 4, 32, 64, cbias=2, norm=1, kid=128, fam='AB'),                    # eight images per tile, ragged last tile
    _c('h128_multi_image_b', 5, 4, 4, 32, 64, cbias=2, norm=2, act=1, kid=128, fam='B'),
    _c('h128_w64', 1, 4, 64, 32, 64, bias=2, kid=128),                                             # bias off 16 bytes: scalar epilogue
    _c('h128_w64_stats', 1, 4, 64, 32, 64, stats=1, mag='small', kid=128),
    _c('h128_tail', 3, 8, 8, 32, 160, tune=V2048, res=1, kid=128, fam='AB'),                       # 128 + 32 columns
    _c('h128_dual_extra', 3, 8, 8, 32, 96, c1=32, ec0=32, ec1=32, norm=1, kid=128, fam='AB'),
    _c('h128_dual_extra_b', 3, 8, 8, 32, 96, c1=32, ec0=32, ec1=32, norm=2, act=1, scale=B_SCALE, kid=128, fam='B'),
    _c('h128_extra1', 3, 8, 8, 32, 96, ec0=32, kid=128),
    _c('h128_splitk', 1, 8, 8, 128, 128, tune=V2048, ws=4, kid=128, splits=4, cbias=2, res=1, fam='AB'),
    _c('h128_splitk_stats', 1, 8, 8, 128, 128, tune=V2048, ws=4, kid=128, splits=4, stats=1, mag='small'),
    _c('h128_splitk_ragged', 1, 8, 8, 128, 7, ws=4, kid=128, splits=4, res=1),                      # scalar partial store
    # ---- 128-pixel tiles on eight half-size waves (1284)
    _c('h1284', 2, 16, 16, 32, 128, kid=1284, fam='AB'),
    _c('h1284_full', 2, 16, 16, 32, 128, cbias=2, res=1, scale=0.25, norm=1, bias=0, kid=1284, fam='AB'),
    _c('h1284_b', 2, 16, 16, 32, 128, cbias=1, res=1, scale=B_SCALE, norm=2, act=1, kid=1284, fam='B'),
    _c('h1284_nonsquare', 2, 4, 32, 32, 128, cbias=1, kid=1284),
    _c('h1284_stats', 2, 16, 16, 32, 128, stats=1, mag='small', kid=1284),
    _c('h1284_splitk', 1, 8, 8, 128, 128, ws=4, kid=1284, splits=4, res=1, fam='AB'),
    _c('h1284_splitk_stats', 1, 8, 8, 128, 128, ws=4, kid=1284, splits=4, stats=1, mag='small'),
    # ---- 256-pixel tiles (256)
    _c('h256', 2, 16, 16, 32, 128, tune=T256, kid=256, fam='AB'),
    _c('h256_full', 2, 16, 16, 32, 128, tune=T256, cbias=2, res=1, scale=0.5, norm=1, kid=256, fam='AB'),
    _c('h256_b', 2, 16, 16, 32, 128, tune=T256, cbias=1, res=1, scale=B_SCALE, norm=2, act=1, bias=0, kid=256, fam='B'),
    _c('h256_tail', 2, 16, 16, 32, 192, tune=T256, c1=32, kid=256, fam='AB'),                      # 128 + 64 columns
    _c('h256_tail_stats', 2, 16, 16, 32, 192, tune=T256, stats=1, mag='small', kid=256),
    _c('h256_splitk', 4, 8, 8, 128, 128, tune=T256, ws=4, kid=256, splits=4, cbias=2, fam='AB'),
    _c('h256_splitk_stats', 4, 8, 8, 128, 128, tune=T256, ws=4, kid=256, splits=4, stats=1, mag='small', res=1),
    # ---- 256 x 256 tiles (2565), 256 x 192 tiles (2568), the Winograd form
    _c('h2565', 2, 16, 16, 32, 256, tune=T2565, kid=2565, fam='AB'),
    _c('h2565_full', 2, 16, 16, 32, 256, tune=T2565, cbias=2, res=1, scale=0.5, norm=1, bias=0, kid=2565, fam='AB'),
    _c('h2565_b', 2, 16, 16, 32, 256, tune=T2565, cbias=1, res=1, scale=B_SCALE, norm=2, act=1, kid=2565, fam='B'),
    _c('h2565_320', 2, 16, 16, 32, 320, tune=T2565, ec0=32, kid=2565, fam='AB'),                   # 256 + 64 columns
    _c('h2565_stats', 2, 16, 16, 32, 256, tune=T2565, stats=1, mag='small', kid=2565),
    _c('h2568', 2, 16, 16, 32, 192, tune=T2568, kid=2568, fam='AB'),
    _c('h2568_full', 2, 16, 16, 32, 192, tune=T2568, cbias=2, res=1, scale=2.0, norm=1, bias=0, kid=2568, fam='AB'),
    _c('h2568_b', 2, 16, 16, 32, 192, tune=T2568, cbias=1, res=1, scale=B_SCALE, norm=2, act=1, kid=2568, fam='B'),
    _c('h2568_stats', 2, 16, 16, 32, 192, tune=T2568, stats=1, mag='small', kid=2568),
    _c('wino', 2, 16, 16, 32, 256, tune=T2565, wino=1, kid=2565),
    _c('wino_full', 2, 16, 16, 32, 256, tune=T2565, wino=1, cbias=2, res=1, scale=0.5, norm=1, bias=0, kid=2565),
    _c('wino_cb1_dual', 2, 16, 16, 32, 256, tune=T2565, wino=1, c1=8, cbias=1, kid=2565),
    _c('wino_stats', 2, 16, 16, 32, 256, tune=T2565, wino=1, stats=1, mag='small', kid=2565),
    _c('wino_act', 2, 16, 16, 32, 256, tune=T2565, wino=1, scale=2.0 ** -12, act=1, kid=2565),        # exact argument, SiLU bound
    _c('wino_w64_extra', 1, 4, 64, 8, 256, tune=T2565, wino=1, ec0=32, kid=2565),
    _c('wino_w64_extra2', 1, 4, 64, 8, 256, tune=T2565, wino=1, ec0=32, ec1=32, res=1, kid=2565),
    # ---- the upsampled-input form on each tile shape
    _c('up2_1284', 2, 16, 16, 32, 128, up2=1, kid=1284, fam='AB'),
    _c('up2_1284_full', 2, 16, 16, 32, 128, up2=1, cbias=2, scale=0.5, bias=0, kid=1284, fam='AB'),
    _c('up2_128', 2, 16, 16, 32, 128, up2=1, tune=V2048, cbias=1, kid=128, fam='AB'),
    _c('up2_128_b', 2, 16, 16, 32, 128, up2=1, tune=V2048, cbias=1, act=1, scale=B_SCALE, kid=128, fam='B'),
    _c('up2_2565', 2, 32, 32, 32, 256, up2=1, tune=T2565, cbias=2, kid=2565, fam='AB'),
    _c('up2_2565_stats', 2, 32, 32, 32, 256, up2=1, tune=T2565, stats=1, mag='small', kid=2565),
    _c('up2_2568', 2, 32, 32, 32, 192, up2=1, tune=T2568, scale=0.5, kid=2568, fam='AB'),
    _c('up2_2568_b', 2, 32, 32, 32, 192, up2=1, tune=T2568, act=1, kid=2568, fam='B'),
    # ---- thin-output kernel (2570) and the <= 4-row projection kernel (2573)
    _c('thin_nchw', 1, 8, 8, 32, 3, nchw=1, kid=2570),
    _c('thin_nchw_norm', 1, 8, 8, 32, 3, nchw=1, norm=1, scale=0.5, bias=0, kid=2570),
    _c('thin_nhwc', 1, 8, 8, 32, 4, out_pad=0, kid=2570),
    _c('thin_nhwc_norm', 1, 8, 8, 32, 4, out_pad=0, norm=1, kid=2570),
    _c('thin_nhwc_b', 2, 8, 8, 32, 4, out_pad=0, norm=2, scale=B_SCALE, kid=2570, fam='B', rounds=8),
    _c('thin_nchw_b', 2, 8, 8, 64, 3, nchw=1, norm=2, bias=0, kid=2570, fam='B', rounds=11),
    _c('rows3', 3, 1, 1, 32, 64, taps=1, kid=2573, fam='AB'),
    _c('rows3_b', 3, 1, 1, 32, 64, taps=1, act=1, scale=B_SCALE, kid=2573, fam='B'),
    _c('rows3_scale_nobias', 3, 1, 1, 32, 64, taps=1, scale=0.5, bias=0, kid=2573),
    _c('rows7_invariant', 7, 1, 1, 32, 64, taps=1, tune=dict(invariant=3), kid=2573),
    # ---- 8-wave LDS-DMA 1x1 kernel (2561): 512 tiles is its floor
    _c('dma8', 32, 16, 16, 32, 2048, taps=1, kid=2561),
    _c('dma8_dual', 32, 16, 16, 32, 2048, taps=1, c1=32, bias=0, cbias=2, kid=2561),
    _c('dma8_ragged', 1, 91, 91, 32, 2000, taps=1, cbias=1, res=1, scale=0.5, kid=2561, fam='AB'),
    _c('dma8_ragged_b', 1, 91, 91, 32, 2000, taps=1, cbias=1, res=1, scale=B_SCALE, act=1, kid=2561, fam='B'),
    # ---- split-fp16 halo kernel (2563)
    _c('split', 1, 16, 16, 32, 96, kind='split', kid=2563, fam='AB'),
    _c('split_multi', 4, 8, 8, 32, 128, kind='split', cbias=2, res=1, scale=0.5, bias=0, kid=2563, fam='AB'),
    _c('split_dual_norm', 1, 16, 16, 32, 200, kind='split', c1=32, ec0=32, norm=1, cbias=1, kid=2563, fam='AB'),
    _c('split_dual_norm_b', 1, 16, 16, 32, 200, kind='split', c1=32, ec0=32, norm=2, cbias=1, res=1, scale=B_SCALE, act=1, kid=2563, fam='B'),
    # ---- fp16 operands on fp32 rows, 1x1 (2564)
    _c('f16w', 1, 16, 16, 64, 70, kind='f16w', taps=1, kid=2564, fam='AB'),
    _c('f16w_dual', 2, 16, 16, 64, 128, kind='f16w', taps=1, c1=64, cbias=2, res=1, scale=0.5, bias=0, kid=2564, fam='AB'),
    _c('f16w_b', 1, 16, 16, 64, 70, kind='f16w', taps=1, cbias=1, scale=B_SCALE, act=1, kid=2564, fam='B'),
    # ---- fp16-activation 3x3 (2566 / 2572), 1x1 (2567), stride 2 (2571), wide images (2575)
    _c('f16c', 1, 16, 16, 64, 64, kind='f16', kid=2566, widths=(1,), fam='AB'),
    _c('f16c_full', 1, 16, 16, 64, 64, kind='f16', cbias=2, res=1, scale=2.0 ** -8, out16=1, bias=0, kid=2566, widths=(1,), fam='AB'),
    _c('f16c_b', 1, 16, 16, 64, 64, kind='f16', cbias=1, res=1, res16=1, scale=B_SCALE, act=1, out16=1, kid=2566, widths=(1,), fam='B'),
    _c('f16c_320', 5, 8, 8, 64, 320, kind='f16', cbias=2, res=1, res16=1, ec0=64, kid=2566, widths=(1,), fam='AB'),   # last tile holds one image
    _c('f16c_320_widths', 5, 8, 8, 64, 320, kind='f16', tune=dict(f16dma_nb=3), cbias=2, res=1, ec0=64, kid=2566, widths=(3, 2), fam='AB'),
    _c('f16c_stats16', 1, 16, 16, 64, 64, kind='f16', stats=1, out16=1, mag='small', kid=2566, widths=(1,)),
    _c('f16c_stats16_rounding', 1, 16, 16, 64, 64, kind='f16', stats=2, out16=1, mag='mid', kid=2566, widths=(1,)),
    _c('f16c_splitk', 1, 16, 16, 256, 64, kind='f16', ws=2, kid=2566, splits=2, widths=(1,), cbias=1, res=1, fam='AB'),
    _c('f16c_splitk_stats16', 1, 16, 16, 256, 64, kind='f16', ws=2, kid=2566, splits=2, widths=(1,), stats=1, out16=1, res=1, res16=1,
       mag='small'),
    _c('f16n', 1, 16, 16, 64, 64, kind='f16', c1=64, norm=1, kid=2572, widths=(1,), fam='AB'),
    _c('f16n_full', 2, 16, 16, 64, 64, kind='f16', c1=64, norm=1, cbias=2, res=1, res16=1, scale=2.0 ** -8, out16=1, bias=0, kid=2572, widths=(1,),
       fam='AB'),
    _c('f16n_b', 1, 16, 16, 64, 64, kind='f16', c1=64, norm=2, cbias=1, res=1, scale=B_SCALE, act=1, kid=2572, widths=(1,), fam='B'),
    _c('f16n_stats', 1, 16, 16, 64, 64, kind='f16', c1=64, norm=1, stats=1, mag='small', kid=2572, widths=(1,)),
    _c('f16g', 1, 3, 5, 64, 64, kind='f16', taps=1, kid=2567, fam='AB'),
    _c('f16g_nw8', 2, 16, 17, 64, 128, kind='f16', taps=1, tune=dict(f16dma_nw=8), cbias=2, res=1, res16=1, scale=2.0 ** -8, out16=1, bias=0, kid=2567,
       fam='AB'),
    _c('f16g_b', 1, 16, 17, 64, 128, kind='f16', taps=1, tune=dict(f16dma_nw=8), cbias=1, res=1, scale=B_SCALE, act=1, kid=2567, fam='B'),
    _c('f16g_stats', 1, 8, 8, 64, 64, kind='f16', taps=1, stats=1, mag='small', kid=2567),
    _c('f16s2', 1, 4, 4, 64, 64, kind='f16', stride=2, kid=2571, fam='AB'),
    _c('f16s2_16', 2, 4, 4, 64, 64, kind='f16', stride=2, cbias=2, scale=2.0 ** -8, out16=1, bias=0, kid=2571, fam='AB'),
    _c('f16s2_b', 1, 4, 4, 64, 64, kind='f16', stride=2, cbias=1, scale=B_SCALE, act=1, kid=2571, fam='B'),
    _c('f16s2_stats', 1, 8, 8, 64, 64, kind='f16', stride=2, stats=1, mag='small', kid=2571),
    _c('f16wide', 1, 4, 128, 64, 64, kind='f16', kid=2575, widths=(1,), fam='AB'),
    _c('f16wide_512', 2, 4, 128, 64, 512, kind='f16', cbias=2, res=1, scale=2.0 ** -8, out16=1, bias=0, kid=2575, widths=(3, 2), fam='AB'),
    _c('f16wide_b', 1, 4, 128, 64, 64, kind='f16', cbias=1, act=1, scale=B_SCALE, res=1, res16=1, kid=2575, widths=(1,), fam='B'),
)
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
BIG = ('dma8', 'dma8_dual')          # 16.7 M outputs: family A only

RUNS = tuple((c.name, fam, v) for c in CASES for fam in c.fam          # (case, family, split-fp16 role in family A / selector round in B)
             for v in ((0, 1) if (c.kind == 'split' and fam == 'A') else (range(c.rounds) if fam == 'B' else (0,))))

# The family-A layer several kernels can run: all of them must return the same bits.
AGREE = (
    # (name, n, h, w, c0, cout, [(label, case overrides)])
    ('l16', 2, 16, 16, 32, 256, (('generic', dict(tune=dict(mode=1), kid=0)), ('h128', dict(tune=dict(mode=128, variant=2048), kid=128)),
                                 ('h1284', dict(tune=dict(mode=128), kid=1284)), ('h256', dict(tune=dict(mode=256, variant=7), kid=256)),
                                 ('h2565', dict(tune=T2565, kid=2565)), ('wino', dict(tune=T2565, wino=1, kid=2565)),
                                 ('split', dict(kind='split', kid=2563)))),
)


def agree_cases():
    """The AGREE layers as Case tuples: same geometry, same data (weights multiples of 4 so that the Winograd U is integer), one per kernel."""
    out = []
    for name, n, h, w, c0, cout, kernels in AGREE:
        for label, kw in kernels:
            out.append(_c(f'{name}_{label}', n, h, w, c0, cout, cbias=2, res=1, scale=0.5, **kw))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# geometry

def ceil_to(v, q):
    return -(-v // q) * q


def geo(case):
    """(input h, input w, input rows, output rows M, cin, ecin, slab width)."""
    ih, iw = (case.h // 2, case.w // 2) if case.up2 else (case.h * case.stride, case.w * case.stride)
    return dict(ih=ih, iw=iw, min=case.n * ih * iw, m=case.n * case.h * case.w, cin=case.c0 + case.c1, ecin=case.ec0 + case.ec1,
                slab=64 if case.kind in ('f16', 'f16w') else 32)


def out_ld(case):
    if case.nchw:
        return 4
    return ceil_to(case.cout, 8) + 2 * case.out_pad if case.out16 else ceil_to(case.cout, 4) + case.out_pad


def res_ld(case):
    return ceil_to(case.cout, 8) + 2 * case.res_pad if case.res16 else ceil_to(case.cout, 4) + case.res_pad


# ------------------------------------------------------------------------------------------------------------------------------
# data

def _odd(g, shape, lim):
    """odd integers in [-lim, lim] (lim odd)."""
    return 2.0 * g.integers(-(lim + 1) // 2, (lim + 1) // 2, size=shape) + 1.0


def _ints(g, shape, lim):
    return g.integers(-lim, lim + 1, size=shape).astype(f64)


def selectors(case, rnd=0):
    """Family B: per output column (tap, channel of [x0 | x1] or -1, channel of [e0 | e1] or -1, weight); round `rnd` of case.rounds continues
    where the columns of the round before stopped."""
    gq = geo(case)
    slab, cin, ecin = gq['slab'], gq['cin'], gq['ecin']
    nslabs = cin // slab if cin % slab == 0 else -(-cin // slab)
    sel = []
    for co in range(rnd * case.cout, (rnd + 1) * case.cout):
        wv = (-1.0 if (co // 2) % 2 else 1.0) * 2.0 ** (co % 5 - 2)
        if ecin and co % 5 == 4:
            sel.append((0, -1, (co * 13) % ecin, wv))
            continue
        ch = ((co // 3) % nslabs) * slab + co % slab
        sel.append((co % case.taps, ch % cin, -1, wv))
    return sel


def selector_visits(case):
    """What the selectors of a case reach: taps, channel positions inside a slab, sources of the main and of the appended operand."""
    gq = geo(case)
    sel = [s_ for rnd in range(case.rounds) for s_ in selectors(case, rnd)]
    main = [s for s in sel if s[1] >= 0]
    return dict(taps={s[0] for s in main}, cpos={s[1] % gq['slab'] for s in main}, src={int(s[1] >= case.c0) for s in main},
                esrc={int(s[2] >= case.ec0) for s in sel if s[2] >= 0})


def make_data(case, fam, role=0, seed=0):
    """The operands of one run as fp64 arrays (every value exactly representable in the format the run stores it in).
    x [n, ih, iw, cin], e [n, h, w, ecin] or None, w [cout, cin, k, k], we [cout, ecin] or None, bias [cout], cbias [rows, cout],
    res [M, cout], planes [n, 3, cin], scale."""
    gq = geo(case)
    g = np.random.default_rng([seed, sum(map(ord, case.name)), ord(fam), role])
    n, cin, ecin, m = case.n, gq['cin'], gq['ecin'], gq['m']
    k = 3 if case.taps == 9 else 1
    xs, ws_, es = (n, gq['ih'], gq['iw'], cin), (case.cout, cin, k, k), (n, case.h, case.w, ecin)
    d = dict(e=None, we=None, bias=None, cbias=None, res=None, planes=None, scale=float(case.scale))
    half_in = case.kind in ('f16', 'f16w')
    if fam == 'A':
        assert case.norm in (0, 1) and np.log2(case.scale) % 1 == 0 and not (case.act and (case.stats or case.out16)), case.name
        if case.mag in ('small', 'mid'):
            d['x'], d['w'] = _ints(g, xs, 1 if case.wino else 3), _ints(g, ws_, 1) * (4.0 if case.wino else 1.0)
            if ecin:
                d['e'], d['we'] = _ints(g, es, 3), _ints(g, (case.cout, ecin), 1)
            ob = 3
            if case.mag == 'mid':                           # |out| reaches 32 with six fraction bits: fp16 rounds it
                ob = 63
        else:
            wide_x = not (case.kind == 'split' and role == 1)
            if half_in:
                d['x'] = _odd(g, xs, 1023) * (UNIT if not case.norm else 1.0)          # 10-bit odd: fp16 holds it, bfloat16 does not
            elif case.wino:
                d['x'] = _ints(g, xs, 7) * UNIT
                d['x'][..., ::4] = _odd(g, xs, 4095)[..., ::4] * UNIT                   # every slab of 8 has two 13-bit channels
            elif wide_x:
                d['x'] = _odd(g, xs, 4095) * UNIT                                       # 13-bit odd: fp32 (and fp16 hi + lo) holds it, fp16 does not
            else:
                d['x'] = _ints(g, xs, 3) * UNIT
            if case.kind == 'split' and role == 1:
                d['w'] = _ints(g, ws_, 3)
                d['w'][:, ::4] = _odd(g, ws_, 8191)[:, ::4]                             # every fourth channel needs hi + lo after the 2^shift scaling
            elif case.wino:
                d['w'] = 4.0 * _ints(g, ws_, 1)                                         # U = G g G^T integer
            else:
                d['w'] = _ints(g, ws_, 3)
            if ecin:
                d['e'] = (_odd(g, es, 1023) if half_in else (_odd(g, es, 4095) if wide_x else _ints(g, es, 3))) * UNIT
                d['we'] = _ints(g, (case.cout, ecin), 3)
                if case.kind == 'split' and role == 1:
                    d['we'][:, ::4] = _odd(g, (case.cout, ecin), 8191)[:, ::4]
            ob = 65535                                                                  # 17-bit odd epilogue operands: fp32 only
        if case.bias:
            d['bias'] = _odd(g, (case.cout,), ob) * (2.0 ** -6 if case.mag == 'mid' else 1.0)
        if case.cbias:
            d['cbias'] = _odd(g, (n if case.cbias == 2 else 1, case.cout), ob)
        if case.res:
            d['res'] = _odd(g, (m, case.cout), 2047 if (case.res16 and ob > 3) else ob)
        if case.norm:
            mu, a, b = _ints(g, (n, cin), 2), g.choice([-1.0, 1.0, 2.0], size=(n, cin)), _odd(g, (n, cin), 3)    # B != 0
            d['planes'] = np.stack([mu, a, b], axis=1)
        return d
    # family B
    x = g.standard_normal(xs)
    d['x'] = x.astype(f16).astype(f64) if case.kind == 'f16' else x.astype(f32).astype(f64)
    w = np.zeros(ws_)
    we = np.zeros((case.cout, ecin)) if ecin else None
    for co, (tap, ch, ech, wv) in enumerate(selectors(case, role)):
        if ech >= 0:
            we[co, ech] = wv
        else:
            w[co, ch, tap // k, tap % k] = wv
    d['w'], d['we'] = w, we
    if ecin:
        e = g.standard_normal(es)
        d['e'] = e.astype(f16).astype(f64) if case.kind == 'f16' else e.astype(f32).astype(f64)
    r32 = lambda v: v.astype(f32).astype(f64)
    if case.bias:
        d['bias'] = r32(g.standard_normal(case.cout))
    if case.cbias:
        d['cbias'] = r32(g.standard_normal((n if case.cbias == 2 else 1, case.cout)))
    if case.res:
        r = g.standard_normal((m, case.cout))
        d['res'] = r.astype(f16).astype(f64) if case.res16 else r32(r)
    if case.norm:
        d['planes'] = r32(np.stack([0.3 * g.standard_normal((n, cin)), 0.5 + g.random((n, cin)), 0.5 + g.standard_normal((n, cin))], axis=1))
    return d


# ------------------------------------------------------------------------------------------------------------------------------
# evaluation: the layer as plain torch in a chosen dtype (fp64: the reference; fp32: the evaluation the CPU test holds to the criterion and
# mutates)

def _t(v, dt):
    return torch.from_numpy(np.ascontiguousarray(v)).to(dt)


def _silu(v):
    return v * torch.sigmoid(v) if v.dtype != torch.float64 else v / (1.0 + torch.exp(-v))


def _r16(v):
    """round to fp16 (nearest even) and back, directly from the tensor's dtype."""
    return v.to(torch.float16).to(v.dtype)


def normalised_input(case, d, dt=torch.float64, mut=()):
    """in = act((x - mu) A + B) as [n, ih, iw, cin] in `dt`, before any fp16 staging; the padded border is applied by `evaluate`."""
    x = _t(d['x'], dt)
    if not case.norm:
        return x
    mu, a, b = (_t(d['planes'][:, i], dt)[:, None, None, :] for i in range(3))
    t = (x - mu) * a + b
    return _silu(t) if case.norm == 2 else t


def evaluate(case, d, dt=torch.float64, mut=(), xin=None):
    """-> dict(out [M, cout] in `dt` (fp16 outputs: the rounded values), stats [blocks, 2, cout] or None).  `mut`: names of deliberate
    defects (tests/test_conv_refs_cpu.py); xin: the staged input to use instead of the normalised one (family B's fp16 candidates)."""
    gq = geo(case)
    k = 3 if case.taps == 9 else 1
    half_in = case.kind in ('f16', 'f16w')
    if xin is None:
        xin = normalised_input(case, d, dt)
        if half_in and (case.norm or case.kind == 'f16w'):
            xin = _r16(xin)
    else:
        xin = _t(xin, dt)
    w = _t(d['w'], dt)
    if 'slab_f16' in mut:                                   # one 32-channel operand slab rounded to fp16
        xin = xin.clone()
        xin[..., :32] = _r16(xin[..., :32])
    xc = xin.permute(0, 3, 1, 2)
    if case.up2:
        xc = F.interpolate(xc, scale_factor=2, mode='nearest')
    if k == 3:
        xc = F.pad(xc, (1, 1, 1, 1))
        if 'pad_raw' in mut and case.norm:                  # the zero padding applied to the raw tensor: the border is act(-mu A + B)
            zero = dict(d, x=np.zeros_like(d['x']))
            border = normalised_input(case, zero, dt).permute(0, 3, 1, 2)
            full = F.pad(border, (1, 1, 1, 1), mode='replicate')
            full[:, :, 1:-1, 1:-1] = xc[:, :, 1:-1, 1:-1]
            xc = full
        if 'halo_cell' in mut:                              # one out-of-image halo cell non-zero
            xc = xc.clone()
            xc[-1, 0, 0, 2] = xc[-1, 0, 1, 2]
    if 'tap_shift' in mut:                                  # one selected tap shifted by one pixel (column 0's weight moves to the next tap)
        w = w.clone()
        co = 0
        nz = torch.nonzero(w[co])
        c_, ky, kx = (int(v) for v in nz[0])
        val = w[co, c_, ky, kx].item()
        w[co, c_, ky, kx] = 0
        w[co, c_, ky, (kx + 1) % k] = val
    y = F.conv2d(xc, w, stride=case.stride)
    if 'acc_f16' in mut:                                    # the accumulator rounded to fp16 once
        y = _r16(y)
    y = y.permute(0, 2, 3, 1).reshape(gq['m'], case.cout)
    if gq['ecin']:
        e = _t(d['e'], dt).reshape(gq['m'], gq['ecin'])
        y = y + e @ _t(d['we'], dt).t()
    hw = case.h * case.w
    if d['bias'] is not None:
        y = y + _t(d['bias'], dt)[None]
    if d['cbias'] is not None:
        cb = _t(d['cbias'], dt)
        img = torch.arange(gq['m']) // hw
        if 'cbias_neighbour' in mut:                        # per-image bias taken from the neighbouring image
            img = (img + 1) % case.n
        if 'cbias_rows' in mut and cb.shape[0] == 1:        # cbias_rows = 1 treated as n: image i reads what lies i rows behind the one row
            cb = cb + torch.arange(case.n, dtype=dt)[:, None]
        y = y + cb[img % cb.shape[0]]
    sc = float(d['scale'])
    if d['res'] is not None and 'res_after_scale' not in mut:
        y = y + _t(d['res'], dt)
    y = y * sc
    if d['res'] is not None and 'res_after_scale' in mut:
        y = y + _t(d['res'], dt)
    if case.act:
        y = _silu(y)
    unrounded = y
    if case.out16:
        if 'rtz16' in mut:                                  # rounded toward zero instead of to nearest even
            h = y.to(torch.float16)
            hf = h.to(y.dtype)
            over = hf.abs() > y.abs()
            y = torch.where(over, _toward_zero16(h, over).to(y.dtype), hf)
        else:
            y = _r16(y)
    if 'one_element' in mut:                                # one output element off by 1e-5 of the absmax
        y = y.clone()
        y[gq['m'] // 2, case.cout // 2] += 1e-5 * float(y.abs().max())
    stats = None
    if case.stats:
        sv = unrounded if 'stats_unrounded' in mut else y
        stats = block_sums(sv, gq['m'], case.cout)
    return dict(out=y, stats=stats)


def _toward_zero16(h, over):
    """fp16 tensor h with the elements flagged in `over` moved one fp16 step toward zero."""
    bits = h.view(torch.int16).clone()
    bits[over] -= 1                                        # sign-magnitude: one step toward zero for either sign
    return bits.view(torch.float16)


def block_sums(y, m, cout):
    """[ceil(m / 64), 2, cout]: column sums and sums of squares of every 64-row block (the last one may be partial), in y's dtype."""
    nb = -(-m // 64)
    pad = torch.zeros(nb * 64, cout, dtype=y.dtype)
    pad[:m] = y
    blk = pad.reshape(nb, 64, cout)
    return torch.stack([blk.sum(1), (blk * blk).sum(1)], 1)


def squares_bound(ref_sq):
    """stats = 2: 64 squares (one rounding each) and at most 64 additions of non-negative terms in any order."""
    return 65.0 * U * np.abs(ref_sq) * SECOND


def stats_per_image(case):
    """True where a 64-row block of stats_out is not 64 consecutive output rows (the upsampled form: phase-major; the Winograd form: two
    patch rows): the comparison is then of each image's sums, which are exact all the same."""
    return bool(case.up2 or case.wino)


def image_sums(stats, case):
    nb = case.h * case.w // 64
    s = np.asarray(stats, dtype=f64).reshape(case.n, nb, 2, case.cout)
    return s.sum(1)


# ------------------------------------------------------------------------------------------------------------------------------
# family A: the conditions that make equality the criterion

def conditions(case, d, role=0):
    """Family A: dict of the quantities the CPU test asserts on (see the module docstring)."""
    gq = geo(case)
    k = 3 if case.taps == 9 else 1
    xin = normalised_input(case, d).numpy()
    half_in = case.kind in ('f16', 'f16w')
    staged = rne16(xin) if half_in else xin
    xa = torch.from_numpy(np.abs(staged)).permute(0, 3, 1, 2)
    if case.up2:
        xa = F.interpolate(xa, scale_factor=2, mode='nearest')
    wa = torch.from_numpy(np.abs(d['w']))
    tot = F.conv2d(xa, wa, stride=case.stride, padding=k // 2).permute(0, 2, 3, 1).reshape(gq['m'], case.cout)
    # (the upsampled form multiplies with FOLDED weights, sums of up to four: |sum| <= sum of magnitudes, so `tot` covers them)
    extra = 0.0
    if gq['ecin']:
        extra = torch.from_numpy(np.abs(d['e']).reshape(gq['m'], gq['ecin'])) @ torch.from_numpy(np.abs(d['we'])).t()
        tot = tot + extra
    for key in ('bias', 'res'):
        if d[key] is not None:
            tot = tot + torch.from_numpy(np.abs(d[key]))
    if d['cbias'] is not None:
        tot = tot + torch.from_numpy(np.abs(d['cbias'])).max(0).values[None]
    c = dict(units=float(tot.max()) / UNIT)
    if case.wino:
        from diff_sampler_amd import ops
        bt = torch.tensor(ops.WINO_BT, dtype=torch.float64).abs()
        gm = torch.tensor(ops.WINO_G, dtype=torch.float64)
        xp = F.pad(torch.from_numpy(np.abs(staged)).permute(0, 3, 1, 2), (1, 1, 1, 1))
        pat = xp.unfold(2, 4, 2).unfold(3, 4, 2)                               # [n, c, ty, tx, 4, 4]
        v = torch.einsum('ik,nctukl,jl->nctuij', bt, pat, bt)                    # |V| <= |B^T| |d| |B|
        u = torch.einsum('ik,ockl,jl->ocij', gm, torch.from_numpy(d['w']), gm)
        c['wino_u_integer'] = bool((u == u.round()).all())
        mm = torch.einsum('nctuij,ocij->ntuoij', v, u.abs())
        c['units'] = max(c['units'], (9.0 * float(mm.max()) + float(torch.as_tensor(extra).max())
                                      + sum(float(np.abs(d[k_]).max()) for k_ in ('bias', 'cbias', 'res') if d[k_] is not None)) / UNIT)
    # representability
    ok16 = lambda v: bool(np.array_equal(rne16(v), v))
    ok32 = lambda v: bool(np.array_equal(np.asarray(v, dtype=f64).astype(f32).astype(f64), v))
    bf16 = lambda v: torch.from_numpy(np.asarray(v, dtype=f64)).to(torch.bfloat16).to(torch.float64).numpy()
    ops_main = [d['x'], d['w']] + ([d['e'], d['we']] if gq['ecin'] else [])
    if half_in:
        c['operands_fit'] = all(ok16(v) for v in ops_main if v is not d['x'] or not case.norm) and ok16(staged)
    elif case.kind == 'split':
        wide, narrow = ([xin, d['e']], [d['w'], d['we']]) if role == 0 else ([d['w'], d['we']], [xin, d['e']])
        hi_lo = lambda v: bool(np.array_equal(rne16(v) + rne16(v - rne16(v)), v))
        c['operands_fit'] = all(hi_lo(v) for v in wide if v is not None) and all(ok16(v) for v in narrow if v is not None)
    else:
        c['operands_fit'] = all(ok32(v) for v in ops_main) and ok32(xin)
    for key in ('bias', 'cbias', 'planes'):
        if d[key] is not None:
            c['operands_fit'] = c['operands_fit'] and ok32(d[key])
    if d['res'] is not None:
        c['operands_fit'] = c['operands_fit'] and (ok16(d['res']) if case.res16 else ok32(d['res']))
    # every K slab holds an operand the next narrower format cannot hold
    slab = 8 if case.wino else gq['slab']
    narrower = bf16 if half_in else rne16
    wide_src = d['w'] if (case.kind == 'split' and role == 1) else staged
    lost = wide_src != narrower(wide_src)
    if wide_src is staged:
        per_slab = lost.reshape(-1, gq['cin'] // slab, slab).any(axis=(0, 2))
    else:
        per_slab = lost.reshape(case.cout, gq['cin'] // slab, slab, -1).any(axis=(0, 2, 3))
    c['every_slab_wide'] = bool(per_slab.all())
    return c


def a_reference(case, d):
    """Family A -> (ref [M, cout] fp64, bound or None, stats or None).  bound None: the criterion is equality.  With an output SiLU
    (the Winograd form, which has no family B) the argument is exact and only ds_silu's own error is left."""
    if not case.act:
        r = evaluate(case, d)
        return r['out'].numpy(), None, (r['stats'].numpy() if r['stats'] is not None else None)
    v = evaluate(case._replace(act=0), d)['out'].numpy()
    y = v / (1.0 + np.exp(-v))
    return y, ((K_SILU + silu_exp_term(v)) * U * np.abs(y) + SILU_ABS) * SECOND, None


def a_inside(case, got, ref, bound):
    got = np.asarray(got, dtype=f64)
    if bound is None:
        return got == ref
    return inside(got, ref, bound)


# ------------------------------------------------------------------------------------------------------------------------------
# family B: reference and bound

def b_reference(case, d):
    """-> (ref_lo, ref_hi, bound) [M, cout] fp64: the reference as an interval -- a point except where an fp16-staged input may round to any
    fp16 value of [rne16(in - b), rne16(in + b)] (one value almost everywhere; several next to zero, where (x - mu) A + B cancels).  Every
    output is a monotone function of its one input except across SiLU's minimum, which the interval then includes."""
    gq = geo(case)
    x = d['x']
    e_in = np.zeros_like(x)
    xin = x
    if case.norm:
        mu, a, b = (d['planes'][:, i][:, None, None, :] for i in range(3))
        dd = x - mu
        t = dd * a + b
        e_t = 2.0 * U * np.abs(dd) * np.abs(a) + U * np.abs(t)
        if case.norm == 2:
            xin = t / (1.0 + np.exp(-t))
            e_in = SILU_LIP * e_t + (K_SILU + silu_exp_term(t)) * U * np.abs(xin) + SILU_ABS
        else:
            xin, e_in = t, e_t
        e_in = e_in * SECOND
    cands = [xin]
    if case.kind == 'split':
        e_in = e_in + 2.0 ** -22 * np.abs(xin) + 2.0 ** -25
    elif case.kind == 'f16w' or (case.kind == 'f16' and case.norm):
        lo, hi = rne16(xin - e_in), rne16(xin + e_in)
        cands = [lo, hi]
        e_in = np.zeros_like(x)
    # the one input element each output sees, and its error
    k = 3 if case.taps == 9 else 1
    wabs = np.abs(d['w'])
    ein_t = torch.from_numpy(e_in).permute(0, 3, 1, 2)
    if case.up2:
        ein_t = F.interpolate(ein_t, scale_factor=2, mode='nearest')
    e_acc = F.conv2d(ein_t, torch.from_numpy(wabs), stride=case.stride, padding=k // 2).permute(0, 2, 3, 1).reshape(gq['m'], case.cout).numpy()
    if case.kind == 'split' and gq['ecin']:          # the appended 1x1 operand is staged as hi + lo like the main one
        e_abs = np.abs(d['e']).reshape(gq['m'], gq['ecin'])
        e_acc = e_acc + (2.0 ** -22 * e_abs + 2.0 ** -25) @ np.abs(d['we']).T
    out = []
    noepi = dict(d, bias=None, cbias=None, res=None, scale=1.0)
    plain = case._replace(act=0, out16=0, stats=0)
    for cand in cands:
        acc = evaluate(plain, noepi, xin=cand)['out'].numpy()
        part, e_pre = acc, e_acc.copy()
        hw = case.h * case.w
        terms = []
        if d['bias'] is not None:
            terms.append(d['bias'][None])
        if d['cbias'] is not None:
            terms.append(d['cbias'][(np.arange(gq['m']) // hw) % d['cbias'].shape[0]])
        if d['res'] is not None:
            terms.append(d['res'])
        for t_ in terms:
            part = part + t_
            e_pre = e_pre + U * np.abs(part)
        v = part * d['scale']
        e_v = abs(d['scale']) * e_pre + U * np.abs(v)
        if case.act:
            y = v / (1.0 + np.exp(-v))
            e_y = SILU_LIP * e_v + (K_SILU + silu_exp_term(v)) * U * np.abs(y) + SILU_ABS
        else:
            y, e_y = v, e_v
        out.append((v, y, e_y * SECOND))
    vs, ys, bs = (np.stack([o[i] for o in out]) for i in range(3))
    ylo, yhi = ys.min(0), ys.max(0)
    if case.act:
        straddles = (vs.min(0) < SILU_ARGMIN) & (vs.max(0) > SILU_ARGMIN)
        ylo = np.where(straddles, SILU_MIN, ylo)
    return ylo, yhi, bs.max(0)


SILU_ARGMIN = -1.2784645427610738          # silu'(t) = 0
SILU_MIN = -0.2784645427610738             # silu(SILU_ARGMIN) = SILU_ARGMIN + 1 (from 1 + e^-t (1 + t) = 0)


def b_inside(case, got, ref):
    """Per element: ref_lo - bound <= got <= ref_hi + bound (fp16 outputs: between the rounded ends, tests/_norm_refs.py `inside`)."""
    ylo, yhi, bound = ref
    got = np.asarray(got, dtype=f64)
    if case.out16:
        return (got >= rne16(ylo - bound)) & (got <= rne16(yhi + bound))
    return (got >= ylo - bound) & (got <= yhi + bound)


# ------------------------------------------------------------------------------------------------------------------------------
# ds_conv_args of a case on buffers that guard everything the launch must not touch

class FakeAlloc:
    """Addresses without memory: ds_conv_route is host logic and only looks at NULL-ness and alignment."""

    def __init__(self):
        self.next = 0x100000

    def __call__(self, name, shape, dtype, fill):
        class _T:
            pass
        t = _T()
        n = int(np.prod(shape)) * (2 if dtype == torch.float16 else 4)
        t.ptr = self.next
        t.data_ptr = lambda p=self.next: p
        self.next += ceil_to(n, 256) + 256
        return t


class TorchAlloc:
    def __init__(self, device):
        self.device = device

    def __call__(self, name, shape, dtype, fill):
        return torch.full(tuple(int(s) for s in shape), fill, dtype=dtype, device=self.device)


SPARE_ROWS = 3
WS_GUARD = 4096


def pack_weights(case, d):
    """-> (packed weight tensor on the CPU, wgt_shift)."""
    from diff_sampler_amd import ops
    w = torch.from_numpy(d['w']).to(torch.float32)
    we = torch.from_numpy(d['we']).to(torch.float32)[:, :, None, None] if d['we'] is not None else None
    if case.kind == 'split':
        return ops.pack_conv_weight_split(w, we)
    if case.kind in ('f16', 'f16w'):
        if case.taps == 1:
            return ops.pack_linear_weight_f16(ops.pack_linear_weight(w[:, :, 0, 0])), 0
        return ops.pack_conv_weight_f16(w, we), 0
    if case.wino:
        return ops.pack_conv_weight_wino(w, extra=we), 0
    if case.up2:
        return ops.pack_conv_weight_up2(w), 0
    wp = ops.pack_conv_weight(w)
    if we is not None:
        wp = torch.cat([wp, ops.pack_conv_weight(we)], 1).contiguous()
    return wp, 0


def build(case, d=None, alloc=None):
    """ds_conv_args of the case (+ the buffers, by name).  d = None with a FakeAlloc: the routing fields only.
    Sources: one allocation [rows, cin + 8] whose padding columns hold NaN, x0 / x1 two column ranges of it (e0 / e1 alike); output: NaN,
    padding columns and SPARE_ROWS rows behind row M; stats_out: one spare block; workspace: exactly case.ws * M * cout floats declared,
    WS_GUARD more behind them."""
    from diff_sampler_amd import _lib
    alloc = alloc or FakeAlloc()
    gq = geo(case)
    half_in = case.kind == 'f16'
    xdt = torch.float16 if half_in else torch.float32
    isz = 2 if half_in else 4
    m, cin, ecin = gq['m'], gq['cin'], gq['ecin']
    b = {}

    def put(name, shape, dtype, value=None, cols=None):
        t = alloc(name, shape, dtype, NAN)
        if value is not None and isinstance(t, torch.Tensor):
            v = torch.from_numpy(np.ascontiguousarray(value)).to(dtype).to(t.device)
            if cols is None:
                t.reshape(-1)[:v.numel()] = v.reshape(-1)
            else:
                t[:v.shape[0], :cols] = v
        b[name] = t
        return t

    have = d is not None
    ldx = cin + 8
    xb = put('x', (gq['min'], ldx), xdt, d['x'].reshape(gq['min'], cin) if have else None, cin)
    eld = ecin + 8
    eb = put('e', (m, eld), xdt, d['e'].reshape(m, ecin) if have else None, ecin) if ecin else None
    if have:
        wp, shift = pack_weights(case, d)
        wb = alloc('w', wp.shape, torch.float32, 0.0)
        wb.copy_(wp)
        b['w'] = wb
    else:
        wb, shift = alloc('w', (128,), torch.float32, 0.0), 0
    bias = put('bias', (case.cout + 4,), torch.float32, None) if case.bias else None
    boff = 4 if case.bias == 2 else 0
    if bias is not None and have:
        bias[boff // 4: boff // 4 + case.cout] = torch.from_numpy(d['bias']).float().to(bias.device)
    cb_ld = ceil_to(case.cout, 4) + 4
    cb = put('cbias', (case.n if case.cbias == 2 else 1, cb_ld), torch.float32, d['cbias'] if have else None, case.cout) if case.cbias else None
    rld = res_ld(case)
    rb = put('res', (m + SPARE_ROWS, rld), torch.float16 if case.res16 else torch.float32, d['res'] if have else None, case.cout) if case.res else None
    old = out_ld(case)
    odt = torch.float16 if case.out16 else torch.float32
    ob = put('out', (case.n * case.cout * case.h * case.w + 64,) if case.nchw else (m + SPARE_ROWS, old), odt)
    planes = put('planes', (case.n, 3, cin), torch.float32, d['planes'] if have else None) if case.norm else None
    nblk = -(-m // 64)
    st = put('stats', ((nblk + 1) * 2 * case.cout,), torch.float32) if case.stats else None
    ws_floats = case.ws * m * case.cout
    ws = put('ws', (ws_floats + WS_GUARD,), torch.float32) if case.ws else None
    p = lambda t, off=0: (t.data_ptr() + off) if t is not None else None
    a = _lib.ConvArgs(p(xb), p(xb, case.c0 * isz) if case.c1 else None, case.c0, case.c1, ldx, ldx if case.c1 else 0, case.n, case.h, case.w,
                      case.taps, p(wb), case.cout, p(bias, boff), p(cb), cb_ld if cb is not None else 0, case.n if case.cbias == 2 else 1,
                      p(rb), rld if rb is not None else 0, float(d['scale']) if have else float(case.scale),
                      _lib.DS_ACT_SILU if case.act else _lib.DS_ACT_NONE, p(ob), old, p(planes),
                      _lib.DS_ACT_SILU if case.norm == 2 else _lib.DS_ACT_NONE, p(eb), p(eb, case.ec0 * isz) if case.ec1 else None,
                      case.ec0, case.ec1, eld if ecin else 0, eld if case.ec1 else 0)
    for f in ('mode', 'variant', 'splits', 'f16dma_nb', 'f16dma_nw', 'ablate', 'invariant'):          # (not the thread's / environment's defaults)
        setattr(a.tune, f, 0)
    for f, v in case.tune:
        setattr(a.tune, f, v)
    a.stride = case.stride if case.stride != 1 else 0
    a.out_nchw, a.in_up2, a.wino = case.nchw, case.up2, case.wino
    a.wgt_f16 = {'f32': 0, 'split': 2, 'f16w': 1, 'f16': 1}[case.kind]
    a.wgt_shift = shift
    a.in_f16, a.out_f16, a.res_f16 = int(half_in), case.out16, case.res16
    if st is not None:
        a.stats_out = p(st)
    if ws is not None:
        a.workspace, a.workspace_floats = p(ws), ws_floats
    return a, b


def route(a):
    """ds_conv_route -> (rc, kernel id, splits, wino, widths)."""
    from diff_sampler_amd import _lib
    r = _lib.ConvRouteInfo()
    rc = _lib.load().ds_conv_route(C.byref(a), C.byref(r))
    return rc, r.kernel_id, r.splits, r.wino, tuple(r.f16_widths[:r.f16_groups])


def expected_route(case):
    return 0, case.kid, case.splits, case.wino, tuple(case.widths)


def scalar_epilogue(case):
    """Which trigger of the scalar epilogue a case pulls (vec_epilogue_ok of csrc/gemm_conv.hip), or None."""
    if out_ld(case) % 4 and not case.nchw:
        return 'out_ld'
    if case.res and res_ld(case) % 4:
        return 'res_ld'
    if case.bias == 2:
        return 'bias'
    return None


def options(case):
    o = set()
    if case.bias:
        o.add('bias')
    if case.cbias == 1:
        o.add('cbias1')
    if case.cbias == 2:
        o.add('cbiasn')
    if case.res:
        o.add('res')
    if case.scale != 1.0:
        o.add('scale')
    if case.act:
        o.add('act')
    if case.res16:
        o.add('res16')
    if case.out16:
        o.add('out16')
    return o


# ------------------------------------------------------------------------------------------------------------------------------
# ds_gemm_nt_batched

GemmCase = namedtuple('GemmCase', 'name m n k batch heads alpha rowbias colbias act')
GEMM_CASES = (
    GemmCase('g_1x1', 1, 1, 32, 1, 1, 1.0, 0, 0, 0),
    GemmCase('g_64', 64, 64, 32, 2, 2, 0.5, 1, 0, 0),
    GemmCase('g_100x129', 100, 129, 96, 2, 3, 1.0, 0, 1, 0),
    GemmCase('g_129x100', 129, 100, 32, 1, 2, 0.25, 1, 1, 0),
    GemmCase('g_129x1_silu', 129, 1, 96, 2, 1, 0.5, 1, 1, 1),
    GemmCase('g_1x129', 1, 129, 32, 3, 2, 1.0, 0, 0, 0),
    GemmCase('g_64x100_silu', 64, 100, 96, 1, 2, 1.0, 0, 1, 1),
    GemmCase('g_100x64', 100, 64, 32, 2, 2, 2.0, 1, 0, 0),
)


def gemm_data(case, seed=0):
    """Attention strides: A / B rows hold the heads side by side ([batch][rows][heads * k + 8], NaN padding), C is [batch][heads][m][ldc]
    with ldc = ceil4(n) + 4.  Family-A values: odd 13-bit integers times 2^-2 against integers in [-3, 3]; 17-bit odd biases."""
    g = np.random.default_rng([seed, sum(map(ord, case.name))])
    a = _odd(g, (case.batch, case.m, case.heads, case.k), 4095) * UNIT
    b = _ints(g, (case.batch, case.n, case.heads, case.k), 3)
    rb = _odd(g, (case.m,), 65535) if case.rowbias else None
    cb = _odd(g, (case.n,), 65535) if case.colbias else None
    if case.act:          # keep SiLU's argument in its interesting range
        a, rb, cb = a / 1024.0, (rb / 65536.0 if rb is not None else None), (cb / 65536.0 if cb is not None else None)
    return dict(a=a, b=b, rowbias=rb, colbias=cb)


def gemm_reference(case, d):
    """-> (ref, bound or None, largest magnitude sum in units of the data) with ref [batch, heads, m, n] fp64; bound None = exact.
    igemm_common.h `epilogue` MODE 1: v = acc * alpha (exact: a power of two); v += colbias; v += rowbias; ds_silu.  Without SiLU every
    term is a multiple of the unit UNIT min(alpha, 1) and the sum of magnitudes stays below 2^24 units: exact.  Under SiLU the operands are
    scaled into its interesting range, the accumulator (units of UNIT / 1024) is still exact and the two bias additions are counted."""
    acc = np.einsum('bmhk,bnhk->bhmn', d['a'], d['b'])
    units = np.einsum('bmhk,bnhk->bhmn', np.abs(d['a']), np.abs(d['b'])) * abs(case.alpha)
    unit = UNIT * min(case.alpha, 1.0) / (1024.0 if case.act else 1.0)
    v = acc * case.alpha
    e = np.zeros_like(v)
    for t_ in ((d['colbias'][None, None, None, :] if d['colbias'] is not None else None),
               (d['rowbias'][None, None, :, None] if d['rowbias'] is not None else None)):
        if t_ is not None:
            v = v + t_
            if not case.act:
                units = units + np.abs(t_)
            e = e + U * np.abs(v)
    if not case.act:
        return v, None, float(units.max()) / unit
    y = v / (1.0 + np.exp(-v))
    return y, (SILU_LIP * e + (K_SILU + silu_exp_term(v)) * U * np.abs(y) + SILU_ABS) * SECOND, float(units.max()) / unit
