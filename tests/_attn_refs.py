"""References, bounds, emulations and case tables for the five attention kernels: ds_attention (csrc/attention.hip), ds_attention_f16
(csrc/attention_f16.hip), ds_attention_causal (csrc/text_encoder.hip) and dsm_attention (csrc/metrics/clip_score.hip).

numpy / torch on the CPU only; nothing here imports the library.  tests/test_attn_refs_cpu.py checks the references against ATen, the
bounds against fp32 emulations of the kernels' operation order, the coverage of the case table and that the exact family bites on
mutants of the emulation; tests/test_hip_attn_kernels.py uses all of it on the GPU.  U, SECOND, rne16, inside and worst are those of
tests/_norm_refs.py.

THE EXACT FAMILY.  Every kernel computes exp as exp2 of scores that carry the factor fl32(scale * fl32(log2 e)); for scale = fl32(ln 2)
2^-k (k = 0, 2, 3, 4) that factor is exactly 2^-k (test_attn_refs_cpu checks it).  With q rows of three non-zero channels of +-2^k, k
entries integers in [-2, 2], v entries integers in [-7, 7] and skv <= 256, every score is an integer in [-6, 6]; every s - m, every weight
2^n (n >= -12, normal in fp16 too), every partial sum (a multiple of 2^-12 below 2^11: 23 bits), every rescale factor and the f16 kernel's
denominator row are exact in fp32 / fp16 whatever the order of summation.  What is left are the reciprocal of the denominator and the
final product, both correctly rounded (the library is built without fast-math):
    |got - ref| <= (2 U + U^2) |ref| <= 2 U SECOND |ref|,                           (exact_bound)
with ref the fp64 quotient of exact sums.  A dropped, doubled or misplaced key of weight 2^-12 moves an output by ~2^-12 / skv >> 2 U: the
family carries the sensitivity.  Its ONE assumption is that the hardware exp2 (v_exp_f32) is exact on integer arguments in [-126, 0]:
test_hip_attn_kernels.py::test_exp2_is_exact_on_integer_arguments holds it (EXP2_INT_EXCESS, in units of U, is what it measured: 0).

THE GENERIC FAMILY against fp64 softmax(q k^T scale) v covers what integers cannot: the numerical formulation.  Per (query, channel) with
s_j the fp64 scores (natural units), m their maximum, w_j the fp64 softmax weights, o = sum_j w_j v_j, T the number of key tiles:
  * a score is a length-d fp32 dot product of q fl(scale log2 e) (three roundings: the constant, the product, q times it) and k:
        E_j = (d + 3) U |scale| sum_c |q_c k_jc|                      (any order of summation, the channel split's three additions included)
  * the exponent's argument fl(s_j - m_run) costs U (m - s_j) (in natural units; the running maximum is below the final one);
  * a weight passes one exp2 (K_EXP2 U relative, measured) and at most T rescales, each a product with an exp2 of its own; the
    denominator likewise:  (K_EXP2 + 2) (T + 1) U;
  * the maximum itself carries the error of its own score: max_j E_j (it cancels in exact arithmetic, but not in fl(s_j - m));
        delta_j = E_j + max_j E_j + U (m - s_j) + (K_EXP2 + 2) (T + 1) U       relative error of weight j
  * a relative error delta_j of weight j moves o_c by w_j delta_j (v_jc - o_c) (numerator and denominator move together);
  * the skv products and additions of P V, the T rescales of O^T, the denominator's sum, the reciprocal and the final product:
        (skv + T + 4) U (sum_j w_j |v_jc| + |o_c|)
  bound = 2 sum_j w_j delta_j |v_jc - o_c| + (skv + T + 4) U (sum_j w_j |v_jc| + |o_c|) + FLUSH
The factor 2 on the first term is headroom, not derived.  FLUSH: a weight below 2^-126 is flushed to zero: skv 2^-126 (max |v| + |o_c|),
absolute (the denominator is at least 1).  First order in U, times SECOND.  On randn the bound is 1e-4 .. 1e-3 of |o|: rigorous, loose.
ds_attention_f16: the reference is computed on the operands as the kernel rounds them -- rne16(fl32(q fl32(scale log2 e))) for fp32 q
(the scores are then in log2 units and carry no further factor), the raw fp16 q with the factor on the fp32 scores otherwise, rne16(k),
rne16(v) -- and the weights are rounded to fp16 before P V: relative 2^-11 and (fp16 subnormals) absolute 2^-25 each, in units of the
largest weight.  Where the denominator comes out of the matrix pipe (d = 40, 80) it is the sum of the ROUNDED weights and the term is
sum_j (2^-11 w_j + 2^-25 / L) |v_jc - o_c|; elsewhere the denominator is of the unrounded weights and the term multiplies |v_jc|.
"""
import math
from collections import namedtuple

import numpy as np

from _norm_refs import U, SECOND, rne16, inside, worst  # noqa: F401

f32, f16, f64 = np.float32, np.float16, np.float64
LOG2E32 = f32(1.4426950408889634)
LN2_32 = np.array([0x3f317218], dtype=np.uint32).view(f32)[0]          # fl32(ln 2): times LOG2E32 it rounds to exactly 1.0f
EXACT_K = (0, 2, 3, 4)

# The hardware exp2 (__builtin_amdgcn_exp2f = v_exp_f32), MEASURED on the MI355X through ds_attention at skv = 2, d = 8, v = (0, 1), scale =
# fl32(ln 2): out = p / (1 + p) with p = exp2(x), x the score difference (tests/test_hip_attn_kernels.py re-measures and asserts both):
#   integer x in [-126, 0]: the output equals fl(2^x fl(1 / fl(1 + 2^x))) bit for bit -- exp2 is exact there, EXP2_INT_EXCESS = 0;
#   ~1 M points x of [-126, 0]: the relative error of exp2 in units of U, EXP2_MEASURED (for x > -25 the three roundings of the
#   quotient, 3 U, are taken off and the rest is multiplied by 1 + p, the inverse of d log out / d log p; below, out = p exactly).
# The bounds use K_EXP2 = twice the measured maximum.  DESIGN.md's tolerance table carries the same numbers.
EXP2_INT_EXCESS = 0.0
EXP2_MEASURED = 1.388         # at x = -29.94; the same maximum on x <= -25 alone, where the output is exp2(x) itself
K_EXP2 = 2 * EXP2_MEASURED
EXP2_SWEEP = (-126.0, 0.0, 1 << 20)


# ------------------------------------------------------------------------------------------------------------------------------
# What each head size compiles to (a restatement of the kernels' constexpr traits)

def traits_f32(d):
    """csrc/attention.hip: VREM :32, KB / KT :45-46, PREFETCH :41, ES_ALIAS :53; the split: ds_attention_variant :242-250, launch :259-274."""
    vrem = d > 32 and d % 32 == 8
    return dict(kt=64 if (d <= 64 and not vrem) else 32, vrem=vrem,
                split='only' if d >= 512 else ('choice' if d % 128 == 0 else 'query'), alias=d >= 512)


def prefetch_f32(d, split):
    """PREFETCH = D <= 96 || DSPLIT (attention.hip:41); split 1 = query, 2 = channel."""
    return d <= 96 or split == 2


def traits_f16(d):
    """csrc/attention_f16.hip: DP :62 (zero-padded contraction), ONES :65, PREFETCH :76."""
    return dict(kt=64, zero_pad=d % 16 != 0, ones=d % 32 != 0, prefetch=d <= 96)


F32_SIZES = (8, 16, 32, 40, 64, 80, 96, 128, 160, 256, 512)
F16_SIZES = (32, 40, 64, 80, 96, 128, 160)


# ------------------------------------------------------------------------------------------------------------------------------
# The case table: one small launch per case.  kernel: f32 = ds_attention, f16 = ds_attention_f16, causal = ds_attention_causal,
# m88 = dsm_attention.  variant as ds_attn_args.variant; in16 / out16 as ds_attn_args.in_f16 / out_f16; k: the exact family's scale is
# fl32(ln 2) 2^-k.

Case = namedtuple('Case', 'name kernel d batch heads sq skv variant in16 out16 k')


def _c(kernel, d, batch, heads, sq, skv, variant=0, in16=0, out16=0, k=0):
    name = f'{kernel}_d{d}_b{batch}h{heads}_q{sq}_k{skv}' + (f'_v{variant}' if variant else '') + \
        (f'_in{in16}o{out16}' if kernel == 'f16' else '')
    return Case(name, kernel, d, batch, heads, sq, skv, variant, in16, out16, k)


CASES = (
    # ds_attention: every head size; skv in {1, KT-1, KT, KT+1, 2 KT+1} of its own KT; sq in {1, 31, 32, 33, 127, 128, 129} (query split)
    _c('f32', 8, 2, 3, 1, 63), _c('f32', 8, 1, 2, 129, 129, k=2),
    _c('f32', 16, 1, 3, 31, 64, k=3), _c('f32', 16, 3, 1, 127, 65),
    _c('f32', 32, 2, 2, 32, 1), _c('f32', 32, 1, 1, 128, 129, k=4),
    _c('f32', 40, 1, 3, 33, 31), _c('f32', 40, 2, 2, 129, 65, k=2), _c('f32', 40, 1, 1, 1, 32),
    _c('f32', 64, 1, 2, 127, 65, k=3), _c('f32', 64, 2, 1, 33, 63), _c('f32', 64, 1, 3, 128, 64),
    _c('f32', 80, 1, 2, 32, 33), _c('f32', 80, 2, 1, 129, 1),
    _c('f32', 96, 1, 1, 31, 32, k=4), _c('f32', 96, 1, 2, 128, 65),
    # multiples of 128: query split (variant 1, no prefetch), channel split (variant 2; sq in {1, 31, 32, 33, 65}), the library's choice
    _c('f32', 128, 1, 2, 129, 33, 1), _c('f32', 128, 1, 1, 127, 31, 1, k=2),
    _c('f32', 128, 2, 1, 33, 65, 2), _c('f32', 128, 1, 2, 65, 32, 2, k=3), _c('f32', 128, 1, 1, 1, 1, 2), _c('f32', 128, 1, 1, 31, 33, 2),
    _c('f32', 128, 1, 1, 32, 31, 2), _c('f32', 128, 1, 1, 33, 65, 0),
    _c('f32', 160, 1, 2, 33, 65), _c('f32', 160, 1, 1, 127, 32, k=4),
    _c('f32', 256, 1, 1, 129, 65, 1), _c('f32', 256, 1, 1, 32, 33, 1), _c('f32', 256, 1, 2, 65, 65, 2, k=2), _c('f32', 256, 1, 1, 31, 1, 2),
    _c('f32', 256, 2, 1, 33, 31, 0),
    _c('f32', 512, 1, 1, 33, 65),
    # ds_attention_f16: sq in {1, 33, 255, 256, 257}, skv in {1, 63, 64, 65, 129}, batch heads in {1, 7, 8, 9}
    _c('f16', 40, 1, 1, 33, 65, in16=0, out16=0), _c('f16', 40, 7, 1, 1, 63, in16=1, out16=1, k=2),
    _c('f16', 40, 2, 4, 257, 129, in16=2, out16=0), _c('f16', 40, 3, 3, 255, 1, in16=3, out16=1, k=3),
    _c('f16', 64, 1, 1, 256, 64, in16=0, out16=1, k=4), _c('f16', 64, 1, 7, 33, 129, in16=1, out16=0),
    _c('f16', 64, 4, 2, 1, 65, in16=2, out16=1), _c('f16', 64, 3, 3, 257, 63, in16=3, out16=0, k=2),
    _c('f16', 32, 1, 1, 255, 1, in16=0, out16=0), _c('f16', 32, 2, 1, 33, 65, in16=3, out16=1, k=3),
    _c('f16', 80, 1, 2, 257, 63, in16=1, out16=0), _c('f16', 80, 1, 1, 33, 129, in16=2, out16=1, k=4),
    _c('f16', 96, 1, 1, 1, 64, in16=0, out16=1), _c('f16', 96, 2, 2, 256, 65, in16=3, out16=0, k=2),
    _c('f16', 128, 1, 1, 33, 65, in16=2, out16=0), _c('f16', 128, 1, 2, 255, 129, in16=1, out16=1, k=3),
    _c('f16', 160, 1, 1, 257, 129, in16=3, out16=0), _c('f16', 160, 1, 2, 33, 63, in16=0, out16=1, k=4),
    # ds_attention_causal: d = 64, sq = skv
    _c('causal', 64, 2, 3, 1, 1), _c('causal', 64, 1, 2, 31, 31, k=2), _c('causal', 64, 3, 1, 32, 32), _c('causal', 64, 1, 1, 33, 33, k=3),
    _c('causal', 64, 2, 2, 77, 77), _c('causal', 64, 1, 2, 128, 128, k=4),
    # dsm_attention: d = 88
    _c('m88', 88, 2, 2, 1, 1), _c('m88', 88, 1, 3, 31, 31, k=2), _c('m88', 88, 1, 1, 32, 32), _c('m88', 88, 2, 1, 33, 33, k=3),
    _c('m88', 88, 1, 2, 129, 129), _c('m88', 88, 1, 1, 33, 65, k=4),
)
CASE_BY_NAME = {c.name: c for c in CASES}


def case_kt(case):
    return traits_f32(case.d)['kt'] if case.kernel == 'f32' else (64 if case.kernel == 'f16' else 32)


def case_tiles(case):
    return -(-case.skv // case_kt(case))


def named_split(case):
    """The work split an f32 case names: 1 query, 2 channel (what ds_attention_variant must answer for it)."""
    if case.d >= 512:
        return 2
    if case.d % 128:
        return 1
    return case.variant if case.variant else 2          # the library's choice at these sizes: fewer than 1 024 waves


# ------------------------------------------------------------------------------------------------------------------------------
# Inputs.  Everything is [batch, rows, heads, d] fp64 here; pack() lays it out for the kernels.

def exact_scale(case):
    return f32(LN2_32 * f32(2.0 ** -case.k))


def exact_inputs(case, seed=0):
    """q: three channels of +-2^k per row; k: integers in [-2, 2]; v: integers in [-7, 7].  For designated queries the keys 0, KT (the first
    key of the second tile) and skv - 1 are set to 2 sign(q) on the query's channels: the score 6, the largest there is, so the running
    maximum moves late, early and at a tile boundary; one query row is zero: all its scores are equal."""
    rng = np.random.default_rng(seed + 7919 * CASES.index(case))
    b, h, sq, skv, d = case.batch, case.heads, case.sq, case.skv, case.d
    q = np.zeros((b, sq, h, d))
    ch = np.argsort(rng.random((b, sq, h, d)), axis=-1)[..., :3]
    np.put_along_axis(q, ch, rng.choice([-1.0, 1.0], size=ch.shape), axis=-1)
    k = rng.integers(-2, 3, size=(b, skv, h, d)).astype(f64)
    v = rng.integers(-7, 8, size=(b, skv, h, d)).astype(f64)
    kt = case_kt(case)
    stars = sorted({0, skv - 1} | ({kt} if kt < skv else set()))
    for bi in range(b):
        for hi in range(h):
            taken = set()
            for n, j in enumerate(stars):
                i = min(sq - 1, j + bi + hi) if case.kernel == 'causal' else (n * max(1, sq // 4) + bi + hi) % sq
                taken.add(i)
                nz = q[bi, i, hi] != 0
                k[bi, j, hi, nz] = 2.0 * q[bi, i, hi, nz]
            ieq = (sq // 2 + hi) % sq
            if ieq not in taken:
                q[bi, ieq, hi] = 0.0
    return q * 2.0 ** case.k, k, v


def exact_ref(case, q, k, v):
    """fp64, exact up to the final division: integer scores, weights 2^(s - m), sums of multiples of 2^-12 below 2^11."""
    s = np.einsum('bqhd,bkhd->bhqk', q, k) * 2.0 ** -case.k
    assert np.array_equal(s, np.round(s)) and np.abs(s).max() <= 6
    if case.kernel == 'causal':
        s = np.where(np.arange(case.skv)[None, :] > np.arange(case.sq)[:, None], -np.inf, s)
    w = np.exp2(s - s.max(-1, keepdims=True))
    return np.einsum('bhqk,bkhd->bqhd', w, v) / w.sum(-1).transpose(0, 2, 1)[..., None]


def exact_bound(ref):
    return (2.0 + 2.0 * EXP2_INT_EXCESS) * U * SECOND * np.abs(ref)


GENERIC_KINDS = ('randn', 'big', 'ramp', 'spike', 'flush', 'negscale')


def generic_inputs(case, kind, seed=0):
    """(q, k, v, scale): randn; q x 30 (logits of a few hundred); keys scaled by a ramp (the maximum moves in every tile); one key ahead
    of all others by more than 150 log2 units (every other weight underflows: the output is that key's v); half of the keys more than
    126 log2 units below the others (flushed weights); randn with a negative scale."""
    rng = np.random.default_rng(seed + 104729 * CASES.index(case) + GENERIC_KINDS.index(kind))
    b, h, sq, skv, d = case.batch, case.heads, case.sq, case.skv, case.d
    q, k, v = rng.standard_normal((b, sq, h, d)), 1.5 * rng.standard_normal((b, skv, h, d)), rng.standard_normal((b, skv, h, d))
    scale = d ** -0.5
    if kind == 'big':
        q *= 30.0
    elif kind == 'ramp':
        k *= (0.25 + 4.0 * np.arange(skv) / max(1, skv - 1))[None, :, None, None]
    elif kind in ('spike', 'flush'):
        # channel 0 carries the gap: q_0 = 20, k_0 = 60 on the leading keys and 0 on the others: 1200 scale against |rest| < 12 sqrt(d) scale
        scale = 1.0 / 8.0
        q[..., 0], k[..., 0] = 20.0, 0.0
        lead = [skv // 2] if kind == 'spike' else list(range(0, skv, 2))
        k[:, lead, :, 0] = 60.0
        if case.kernel == 'causal':          # key 0 is the only one every query sees
            k[:, 0, :, 0] = 60.0 if kind == 'flush' else 120.0
    elif kind == 'negscale':
        scale = -scale
    return q, k, v, scale


def as_operands(case, q, k, v):
    """The tensors as the kernel's operand types hold them: fp32, or fp16 where in_f16 says so."""
    q16, kv16 = (case.in16 & 1, case.in16 & 2) if case.kernel == 'f16' else (0, 0)
    return q.astype(f16 if q16 else f32), k.astype(f16 if kv16 else f32), v.astype(f16 if kv16 else f32)


# ------------------------------------------------------------------------------------------------------------------------------
# The generic reference and its bound (module docstring)

def generic_ref(case, q, k, v, scale):
    """q, k, v: the operands (as_operands) -> (ref, bound) fp64 [batch, sq, heads, d]."""
    b, h, sq, skv, d = case.batch, case.heads, case.sq, case.skv, case.d
    T = case_tiles(case)
    isf16 = case.kernel == 'f16'
    qe, ke, ve = q.astype(f64), k.astype(f64), v.astype(f64)
    fac = float(scale)
    if isf16:
        sc = f32(scale) * LOG2E32
        ke, ve = rne16(ke), rne16(ve)
        if case.in16 & 1:
            fac = float(sc) * math.log(2.0)
        else:
            qe, fac = rne16((q.astype(f32) * sc).astype(f64)), math.log(2.0)
    ones = isf16 and traits_f16(d)['ones']
    ref, bound = np.empty((b, sq, h, d)), np.empty((b, sq, h, d))
    causal = np.arange(skv)[None, :] > np.arange(sq)[:, None] if case.kernel == 'causal' else None
    for bi in range(b):
        for hi in range(h):
            qq, kk, vv = qe[bi, :, hi], ke[bi, :, hi], ve[bi, :, hi]
            s = fac * (qq @ kk.T)
            E = (d + 3) * U * abs(fac) * (np.abs(qq) @ np.abs(kk).T)
            if causal is not None:
                s, E = np.where(causal, -np.inf, s), np.where(causal, 0.0, E)
            m = s.max(-1, keepdims=True)
            p = np.exp(s - m)
            L = p.sum(-1, keepdims=True)
            w = p / L
            o = w @ vv
            gap = np.where(np.isfinite(s), m - s, 0.0)
            delta = E + E.max(-1, keepdims=True) + U * gap + (K_EXP2 + 2) * (T + 1) * U
            first, half = np.empty_like(o), np.zeros_like(o)
            for i0 in range(0, sq, 16):
                sl = slice(i0, i0 + 16)
                dev = np.abs(vv[None, :, :] - o[sl, None, :])
                first[sl] = np.einsum('qk,qkc->qc', w[sl] * delta[sl], dev)
                if isf16:
                    wr = 2.0 ** -11 * w[sl] + np.where(np.isfinite(s[sl]), 2.0 ** -25, 0.0) / L[sl]
                    half[sl] = np.einsum('qk,qkc->qc', wr, dev if ones else np.broadcast_to(np.abs(vv)[None], dev.shape))
            flush = skv * 2.0 ** -126 * (np.abs(vv).max() + np.abs(o))
            ref[bi, :, hi] = o
            bound[bi, :, hi] = (2.0 * first + half + (skv + T + 4) * U * (w @ np.abs(vv) + np.abs(o)) + flush) * SECOND
    return ref, bound


# ------------------------------------------------------------------------------------------------------------------------------
# fp32 emulations of the kernels' order, one (image, head) at a time, the queries vectorised.  `mutant` names a deliberate bug (MUTANTS).

MUTANTS = ('dup_counted', 'last_masked', 'o_not_rescaled', 'l_not_rescaled', 'v_swap', 'vrem_half', 'head_k')


def _exp2(x):
    """exp2 in fp32, exact on integers, results below 2^-126 flushed to zero."""
    x = np.asarray(x, dtype=f32)
    with np.errstate(under='ignore', over='ignore'):
        r = np.exp2(x.astype(f64)).astype(f32)
    return np.where(r < f32(2.0 ** -126), f32(0), r)


def _key(kb, r, hb):
    """Register r of lane half hb holds this key of 32-key block kb (the 32x32 MFMA C/D layout)."""
    return kb * 32 + (r & 3) + 8 * (r >> 2) + 4 * hb


def _mask(keys, skv, sq, causal, mutant):
    lim = skv + 1 if mutant == 'dup_counted' else (skv - 1 if mutant == 'last_masked' else skv)
    masked = np.broadcast_to(keys[None, :] >= lim, (sq, keys.size))
    if causal:
        masked = masked | (keys[None, :] > np.arange(sq)[:, None])
    return masked


_SWAP = np.arange(64)
for _b0 in (0, 32):
    _SWAP[_b0 + 4:_b0 + 8], _SWAP[_b0 + 8:_b0 + 12] = np.arange(_b0 + 8, _b0 + 12), np.arange(_b0 + 4, _b0 + 8)


def emulate_f32(q, k, v, scale, kt, vrem=False, dsplit=False, causal=False, mutant=None):
    """attention.hip / text_encoder.hip / clip_score.hip: q [sq, d], k, v [skv, d] fp32 -> out [sq, d] fp32."""
    sq, d = q.shape
    skv = k.shape[0]
    qs = q.astype(f32) * (f32(scale) * LOG2E32)
    dm = d - 8 if vrem else d
    m, l = np.full(sq, -1e30, f32), np.zeros((sq, 2), f32)
    ot, oe = np.zeros((sq, dm), f32), np.zeros((sq, 2, 8), f32)
    for t in range(-(-skv // kt)):
        keys = t * kt + np.arange(kt)
        kc = np.minimum(keys, skv - 1)
        ktile, vtile = k[kc].astype(f32), v[kc].astype(f32)
        if mutant == 'v_swap':
            vtile = vtile[_SWAP[:kt]]
        parts = []
        for c0 in range(0, d, d // 4 if dsplit else d):
            st = np.zeros((sq, kt), f32)
            for ks in range(c0, c0 + (d // 4 if dsplit else d), 8):
                for r in range(4):
                    st = st + (np.outer(qs[:, ks + r], ktile[:, ks + r]) + np.outer(qs[:, ks + 4 + r], ktile[:, ks + 4 + r]))
            parts.append(st)
        st = ((parts[0] + parts[1]) + parts[2]) + parts[3] if dsplit else parts[0]
        st = np.where(_mask(keys, skv, sq, causal, mutant), f32(-1e30), st)
        mn = np.maximum(m, st.max(1))
        alpha = _exp2(m - mn)
        m = mn
        p = _exp2(st - mn[:, None])
        rs = np.zeros((sq, 2), f32)
        for kb in range(kt // 32):
            for r in range(16):
                for hb in range(2):
                    rs[:, hb] = rs[:, hb] + p[:, _key(kb, r, hb)]
        l = (l if mutant == 'l_not_rescaled' else l * alpha[:, None]) + rs
        if mutant != 'o_not_rescaled':
            ot, oe = ot * alpha[:, None], oe * alpha[:, None, None]
        for kb in range(kt // 32):
            for r in range(16):
                k0, k1 = _key(kb, r, 0), _key(kb, r, 1)
                ot = ot + (np.outer(p[:, k0], vtile[k0, :dm]) + np.outer(p[:, k1], vtile[k1, :dm]))
                if vrem:
                    oe[:, 0] = oe[:, 0] + np.outer(p[:, k0], vtile[k0, dm:])
                    oe[:, 1] = oe[:, 1] + np.outer(p[:, k1], vtile[k1, dm:])
    inv = f32(1) / (l[:, 0] + l[:, 1])
    out = ot * inv[:, None]
    if vrem:
        rem = (oe[:, 0] if mutant == 'vrem_half' else oe[:, 0] + oe[:, 1]) * inv[:, None]
        out = np.concatenate([out, rem], axis=1)
    return out


def emulate_f16(q, k, v, scale, in16, out16, mutant=None):
    """attention_f16.hip: operands fp32 or fp16 as in16 says -> out [sq, d] fp32 (fp16 values where out16)."""
    sq, d = q.shape
    skv = k.shape[0]
    sc = f32(scale) * LOG2E32
    ones = d % 32 != 0
    if in16 & 1:
        qe, ss = q.astype(f16).astype(f64), sc
    else:
        qe, ss = (q.astype(f32) * sc).astype(f16).astype(f64), f32(1)
    ke, ve = k.astype(f16).astype(f64), v.astype(f16).astype(f64)
    if ones:
        ve = np.concatenate([ve, np.ones((skv, 1))], axis=1)
    m, l = np.full(sq, -1e30, f32), np.zeros((sq, 2), f32)
    ot = np.zeros((sq, ve.shape[1]), f32)
    for t in range(-(-skv // 64)):
        keys = t * 64 + np.arange(64)
        kc = np.minimum(keys, skv - 1)
        ktile, vtile = ke[kc], ve[kc]
        if mutant == 'v_swap':
            vtile = vtile[_SWAP]
        st = np.zeros((sq, 64), f32)
        for c0 in range(0, d, 16):
            st = (st.astype(f64) + qe[:, c0:c0 + 16] @ ktile[:, c0:c0 + 16].T).astype(f32)
        st = np.where(_mask(keys, skv, sq, False, mutant), f32(-1e30), st)
        mn = np.maximum(m, st.max(1) * ss)
        alpha = _exp2(m - mn)
        m = mn
        p = _exp2((st.astype(f64) * f64(ss) - mn[:, None].astype(f64)).astype(f32))
        if not ones:
            rs = np.zeros((sq, 2), f32)
            for kb in range(2):
                for r in range(16):
                    for hb in range(2):
                        rs[:, hb] = rs[:, hb] + p[:, _key(kb, r, hb)]
            l = (l if mutant == 'l_not_rescaled' else l * alpha[:, None]) + rs
        if mutant != 'o_not_rescaled':
            keep = ot[:, d].copy() if ones and mutant == 'l_not_rescaled' else None
            ot = ot * alpha[:, None]
            if keep is not None:
                ot[:, d] = keep
        pf = p.astype(f16).astype(f64)
        for s in range(4):
            ot = (ot.astype(f64) + pf[:, 16 * s:16 * s + 16] @ vtile[16 * s:16 * s + 16]).astype(f32)
    inv = f32(1) / (ot[:, d] if ones else l[:, 0] + l[:, 1])
    out = ot[:, :d] * inv[:, None]
    return out.astype(f16).astype(f32) if out16 else out


def emulate_case(case, q, k, v, scale, mutant=None):
    """The emulation of the case's kernel over every (image, head); q, k, v as as_operands gives them."""
    out = np.empty((case.batch, case.sq, case.heads, case.d), f32)
    for bi in range(case.batch):
        for hi in range(case.heads):
            hk = (hi + 1) % case.heads if mutant == 'head_k' else hi
            qq, kk, vv = q[bi, :, hi], k[bi, :, hk], v[bi, :, hi]
            if case.kernel == 'f16':
                out[bi, :, hi] = emulate_f16(qq, kk, vv, scale, case.in16, case.out16, mutant)
            else:
                tr = traits_f32(case.d) if case.kernel == 'f32' else dict(kt=32, vrem=False)
                out[bi, :, hi] = emulate_f32(qq, kk, vv, scale, tr['kt'], tr['vrem'], case.kernel == 'f32' and named_split(case) == 2,
                                             case.kernel == 'causal', mutant)
    return out


# The case on which each mutant of the emulation must leave the exact family's bound (test_attn_refs_cpu asserts it).
MUTANT_CASES = {
    'dup_counted': 'f32_d64_b1h2_q127_k65',
    'last_masked': 'f16_d40_b1h1_q33_k65_in0o0',
    'o_not_rescaled': 'f32_d96_b1h2_q128_k65',
    'l_not_rescaled': 'm88_d88_b1h1_q33_k65',
    'v_swap': 'f16_d64_b1h7_q33_k129_in1o0',
    'vrem_half': 'f32_d40_b1h3_q33_k31',
    'head_k': 'causal_d64_b2h2_q77_k77',
}


# ------------------------------------------------------------------------------------------------------------------------------
# Buffer layout: packed rows of ld = heads d + PAD_COLS elements, PAD_ROWS spare rows per image; what is no operand element holds NaN
# (or, fill='junk', large finite numbers: the kernels must give the same bits either way).

PAD_COLS, PAD_ROWS = 8, 3


def pack(x, dtype, fill='nan', seed=0):
    """x [batch, rows, heads, d] -> (buffer [batch, rows + PAD_ROWS, heads d + PAD_COLS] of dtype, ld, batch stride in elements)."""
    b, rows, h, d = x.shape
    ld = h * d + PAD_COLS
    if fill == 'nan':
        buf = np.full((b, rows + PAD_ROWS, ld), np.nan, dtype)
    else:
        buf = (1e3 * np.random.default_rng(seed).standard_normal((b, rows + PAD_ROWS, ld))).astype(dtype)
    buf[:, :rows, :h * d] = x.reshape(b, rows, h * d).astype(dtype)
    return buf, ld, (rows + PAD_ROWS) * ld


def out_buffer(case):
    dtype = f16 if case.out16 else f32
    ld = case.heads * case.d + PAD_COLS
    return np.full((case.batch, case.sq + PAD_ROWS, ld), np.nan, dtype), ld, (case.sq + PAD_ROWS) * ld


def unpack_out(case, buf):
    """The live block as fp64 [batch, sq, heads, d]; everything else must still be NaN."""
    hd = case.heads * case.d
    assert np.isnan(buf[:, case.sq:]).all(), 'a guard row was written'
    assert np.isnan(buf[:, :case.sq, hd:]).all(), 'a padding column was written'
    return buf[:, :case.sq, :hd].astype(f64).reshape(case.batch, case.sq, case.heads, case.d)


def fields(case, ptr, ld, bs, scale):
    """ds_attn_args of a case as a dict; ptr / ld / bs: dicts over q, k, v, out."""
    return dict(q=ptr['q'], k=ptr['k'], v=ptr['v'], out=ptr['out'], ldq=ld['q'], ldk=ld['k'], ldv=ld['v'], ldo=ld['out'],
                q_bs=bs['q'], k_bs=bs['k'], v_bs=bs['v'], o_bs=bs['out'], batch=case.batch, heads=case.heads, sq=case.sq, skv=case.skv,
                d=case.d, scale=float(scale), out_f16=case.out16, in_f16=case.in16, variant=case.variant)


# ------------------------------------------------------------------------------------------------------------------------------
# Calls the four entry points must refuse before they launch anything (DS_E_ARG -1, DS_E_ALIGN -2, DS_E_SHAPE -3).  Every entry starts
# from a case that runs and changes one thing.

FAKE = 0x10000


def fake_ptrs():
    return {k: FAKE * (i + 1) for i, k in enumerate(('q', 'k', 'v', 'out'))}


BASE = {'f32': 'f32_d64_b2h1_q33_k63', 'f16': 'f16_d64_b3h3_q257_k63_in3o0', 'causal': 'causal_d64_b2h2_q77_k77', 'm88': 'm88_d88_b1h1_q33_k65'}


def _common(kernel, counts_big):
    r = [(f'{kernel}_null_{p}', kernel, {p: None}, {}, -1) for p in ('q', 'k', 'v', 'out')]
    r += [(f'{kernel}_{f}_{val}', kernel, {f: val}, {}, -1) for f, val in (('batch', 0), ('heads', 0), ('sq', 0), ('skv', -1), ('sq', -5))]
    r += [(f'{kernel}_{f}_65536', kernel, {f: 65536}, {}, -1) for f in counts_big]
    r += [(f'{kernel}_{f}_plus2', kernel, {f: ('+', 2)}, {}, -2) for f in ('ldq', 'ldk', 'ldv', 'ldo', 'q_bs', 'k_bs', 'v_bs', 'o_bs')]
    r += [(f'{kernel}_{p}_misaligned', kernel, {}, {p: 8}, -2) for p in ('q', 'k', 'v', 'out')]
    return r


REFUSALS = (
    _common('f32', ('batch', 'heads')) + [
        ('f32_in_f16', 'f32', dict(in_f16=1), {}, -1), ('f32_out_f16', 'f32', dict(out_f16=1), {}, -1),
        ('f32_variant_3', 'f32', dict(variant=3), {}, -1), ('f32_variant_neg', 'f32', dict(variant=-1), {}, -1),
        ('f32_d24', 'f32', dict(d=24), {}, -3), ('f32_d88', 'f32', dict(d=88), {}, -3), ('f32_d0', 'f32', dict(d=0), {}, -3),
        ('f32_ptr_plus4', 'f32', {}, dict(k=4), -2)]
    + _common('f16', ()) + [
        ('f16_in_f16_4', 'f16', dict(in_f16=4), {}, -1), ('f16_in_f16_7', 'f16', dict(in_f16=7), {}, -1),
        ('f16_variant_3', 'f16', dict(variant=3), {}, -1), ('f16_variant_neg', 'f16', dict(variant=-1), {}, -1),
        ('f16_variant_2_d80', 'f16', dict(variant=2, d=80), {}, -3),
        ('f16_q16_ldq_4', 'f16', dict(ldq=('+', 4)), {}, -2), ('f16_q16_q_bs_4', 'f16', dict(q_bs=('+', 4)), {}, -2),
        ('f16_kv16_ldk_4', 'f16', dict(ldk=('+', 4)), {}, -2), ('f16_kv16_k_bs_4', 'f16', dict(k_bs=('+', 4)), {}, -2),
        ('f16_d8', 'f16', dict(d=8), {}, -3), ('f16_d256', 'f16', dict(d=256), {}, -3), ('f16_d48', 'f16', dict(d=48), {}, -3),
        ('f16_q16_scale_zero', 'f16', dict(scale=0.0), {}, -1), ('f16_q16_scale_negative', 'f16', dict(scale=-0.125), {}, -1),
        ('f16_q16_scale_nan', 'f16', dict(scale=float('nan')), {}, -1), ('f16_q16_scale_inf', 'f16', dict(scale=float('inf')), {}, -1),
        ('f16_q16_only_scale_negative', 'f16', dict(scale=-0.125, in_f16=1), {}, -1)]
    + _common('causal', ('batch',)) + [
        ('causal_in_f16', 'causal', dict(in_f16=1), {}, -1), ('causal_out_f16', 'causal', dict(out_f16=1), {}, -1),
        ('causal_sq_ne_skv', 'causal', dict(skv=64), {}, -1), ('causal_sq_129', 'causal', dict(sq=129, skv=129), {}, -3),
        ('causal_d40', 'causal', dict(d=40), {}, -3), ('causal_d128', 'causal', dict(d=128), {}, -3)]
    + _common('m88', ('batch', 'heads')) + [
        ('m88_reserved0', 'm88', dict(out_f16=1), {}, -1), ('m88_reserved1', 'm88', dict(in_f16=1), {}, -1),
        ('m88_reserved2', 'm88', dict(variant=1), {}, -1), ('m88_d64', 'm88', dict(d=64), {}, -3), ('m88_d96', 'm88', dict(d=96), {}, -3),
        ('m88_ldq_below_span', 'm88', dict(ldq=84), {}, -1), ('m88_ldo_below_span', 'm88', dict(ldo=84), {}, -1)]
)
# Calls that look like refusals and are none: a negative scale is served wherever the factor is folded into q.
ACCEPTED_NEGATIVE_SCALE = (('f32', 0), ('f16', 0), ('f16', 2), ('causal', 0), ('m88', 0))


def refusal_fields(entry, ptr=None):
    """(kernel, ds_attn_args fields) of a refusal-table entry; ptr: real device addresses on the GPU, fake ones otherwise."""
    name, kernel, changes, offs, _ = entry
    case = CASE_BY_NAME[BASE[kernel]]
    ptr = dict(ptr or fake_ptrs())
    for p, o in offs.items():
        ptr[p] += o
    hd = case.heads * case.d + PAD_COLS
    ld = dict(q=hd, k=hd, v=hd, out=hd)
    bs = dict(q=(case.sq + PAD_ROWS) * hd, k=(case.skv + PAD_ROWS) * hd, v=(case.skv + PAD_ROWS) * hd, out=(case.sq + PAD_ROWS) * hd)
    f = fields(case, ptr, ld, bs, case.d ** -0.5)
    for key, val in changes.items():
        f[key] = f[key] + val[1] if isinstance(val, tuple) else val
    return kernel, f
