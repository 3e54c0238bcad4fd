"""Plain fp64 restatements of the normalisation family of csrc/norm_act.hip (GroupNorm statistics, the statistics from the convolutions'
partial sums, the {mu, A, B} planes, the fused normalise / affine / SiLU / resample pass in both kernels), of LayerNorm rows, GEGLU and the
noise embedding; the per-element error bounds the GPU tests hold the kernels to; and the tables of shapes those tests run.

numpy / torch on the CPU only; nothing here imports the library.  tests/test_norm_refs_cpu.py checks the references against ATen in fp64,
the bounds against fp32 emulations of the kernels' operation order, and (through ds_norm_route) that the tables reach every kernel and
loop they name; tests/test_hip_norm_kernels.py uses them on the GPU.

Notation: U = 2^-24 is the unit roundoff of fp32, one fp32 rounding of v costs at most U |v|; gam(k) = k U / (1 - k U) bounds k of them
compounded.  A bound is first order in U with every first-order term written out; the terms of order U^2 are covered by the factor
SECOND = 1 + 2^-10 on the whole bound (they are U times a first-order term each, and there are far fewer than 2^14 of them).
"""
import math
from collections import namedtuple

import numpy as np
import torch

U = 2.0 ** -24
SECOND = 1.0 + 2.0 ** -10
EPS = 1e-5


def gam(k):
    return k * U / (1.0 - k * U)


# ------------------------------------------------------------------------------------------------------------------------------
# Device functions whose accuracy cannot be derived from their source: MEASURED on the MI355X against fp64 (tools: the sweep is
# tests/test_hip_norm_kernels.py::test_device_function_constants_hold_on_a_dense_sweep, which re-measures and asserts them), in units of
# U |result|; the constant used by the bounds is TWICE the measured maximum (the sweep is finite).  DESIGN.md's tolerance table carries the
# same numbers.
#   ds_silu(t) = t * v_rcp_f32(1 + __expf(-t)), __expf(v) = v_exp_f32(fl(v * fl(log2 e))): ~1 M points of [-100, 100] through ds_norm_act in
#   identity + SiLU form.  Two parts of its error are DERIVED and only the rest is measured:
#     - the rounded constant and the rounded product each move the exponent by at most U |t| log2 e, i.e. e^-t by |t| U relative each;
#       through y = t / (1 + e^-t) that is 2 |t| s(-t) U |y| with s(-t) = e^-t / (1 + e^-t) (SILU_EXP: at most 2 U |y| for t > -1.3, growing
#       like 2 |t| U on the negative tail, where the result itself is e^t small -- measured without this term the maximum is 61 U at t = -87);
#     - for t < -87.3 the denominator reaches 2^126 and its reciprocal is subnormal or zero; |silu(t)| = |t| e^t < 88.8 * 2^-126 < 2^-119
#       there: the absolute term SILU_ABS.
#   The measurement is of (|err| - SILU_ABS - SILU_EXP)+ / (U |silu|).
SILU_MEASURED = 2.657
K_SILU = 2 * SILU_MEASURED
SILU_ABS = 2.0 ** -119
SILU_LIP = 1.1            # max |d silu / dt| = 1.0998 (at t = 2.3994)
#   GEGLU: erff through ds_geglu with a = 1 over the same sweep of gates: the ABSOLUTE error of erff(g / sqrt 2) in units of U (|erf| <= 1),
#   i.e. (|err| - 3 U |gelu|)+ / (U |g / 2|) -- see geglu_ref.
ERF_MEASURED = 1.039
K_ERF = 2 * ERF_MEASURED
#   sinf / cosf through ds_noise_embed with the argument given directly (flag 2, frequency 1): ~1 M arguments of [-1e3, 1e3];
#   logf through the same kernel with frequency 2^-20 (the product is exact and sin(a) = a (1 - 4e-13) for |a| < 1.6e-6): the relative
#   error of sinf(logf(sigma) / 4 * 2^-20) against log(sigma) / 4 * 2^-20, sigma log-uniform in [0.002, 80].
TRIG_MEASURED = 2.041
K_TRIG = 2 * TRIG_MEASURED
LOG_MEASURED = 3.132
K_LOG = 2 * LOG_MEASURED


def silu_exp_term(t):
    """The derived part of ds_silu's relative error, in units of U: 2 |t| e^-t / (1 + e^-t)."""
    t = np.asarray(t, dtype=np.float64)
    return 2.0 * np.abs(t) * np.exp(-np.logaddexp(0.0, t))


# ------------------------------------------------------------------------------------------------------------------------------
# helpers

def rne16(v):
    """fp64 -> the nearest fp16 value (round to nearest even, overflow to inf), as fp64.  Through fp32 would round twice: numpy converts
    float64 to float16 directly."""
    return np.asarray(v, dtype=np.float64).astype(np.float16).astype(np.float64)


def inside(got, ref, bound, out16=False):
    """Per element: |got - ref| <= bound -- for an fp16 output `got` must lie in [rne16(ref - bound), rne16(ref + bound)] (rounding is
    monotone, so a kernel whose fp32 value is inside the bound rounds into that interval; fp16 gets no tolerance of its own).  NaN in
    `got` is outside.  Returns the boolean array."""
    got, ref, bound = (np.asarray(v, dtype=np.float64) for v in (got, ref, bound))
    if out16:
        return (got >= rne16(ref - bound)) & (got <= rne16(ref + bound))
    return np.abs(got - ref) <= bound


def worst(got, ref, bound, out16=False):
    """Diagnostic for a failing comparison: (number outside, flat index of the worst element, its got / ref / bound)."""
    ok = inside(got, ref, bound, out16)
    got, ref, bound = (np.asarray(v, dtype=np.float64) for v in (got, ref, bound))
    bad = np.flatnonzero(~ok.reshape(-1))
    if bad.size == 0:
        return 'all inside'
    excess = np.abs(got - ref).reshape(-1)[bad] - np.broadcast_to(bound, got.shape).reshape(-1)[bad]
    excess = np.where(np.isnan(excess), np.inf, excess)
    i = bad[int(np.argmax(excess))]
    return f'{bad.size} of {ok.size} outside; worst at {i}: got {got.reshape(-1)[i]!r} ref {ref.reshape(-1)[i]!r} bound {np.broadcast_to(bound, got.shape).reshape(-1)[i]!r}'


def within_ulps32(got, ref64, ulps=1):
    """got (fp32) within `ulps` fp32 ulps of the fp64 reference rounded once."""
    r = np.asarray(ref64, dtype=np.float64).astype(np.float32)
    lo, hi = r, r
    for _ in range(ulps):
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
    got = np.asarray(got, dtype=np.float32)
    return (got >= lo) & (got <= hi)


def silu64(t):
    return t / (1.0 + np.exp(-t))


# ------------------------------------------------------------------------------------------------------------------------------
# 1. GroupNorm statistics (ds_gn_stats, ds_gn_finalize, the self-finalising pass)
#    The kernels sum x and x^2 in fp64 and round mean and 1 / sqrt(var + eps) ONCE to fp32: they are held to 1 fp32 ulp of the fp64
#    reference (within_ulps32).  The slack of one ulp covers only the unordered fp64 LDS atomics landing the fp64 value on the other side of
#    a rounding boundary: the one-pass variance E[x^2] - mean^2 loses E[x^2] / var * 2^-53 relative in fp64, and the tables keep
#    E[x^2] / var <= 1e4 (data `30 + randn`: 901), eight orders of magnitude below U.  A CONSTANT group is the exception by construction: its
#    value has few significant bits, every sum is exact, var is exactly 0 and rstd = 1 / sqrt(eps).

def gn_stats_ref(x, groups, eps=EPS):
    """x: [n, P, C] (pixels x concatenated channels; fp32 values or fp16 values, any float dtype) -> fp64 (mean, rstd) [n, groups],
    two-pass in fp64."""
    x = np.asarray(x, dtype=np.float64)
    n, p, c = x.shape
    xg = x.reshape(n, p, groups, c // groups)
    mean = xg.mean(axis=(1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean(axis=(1, 3))
    return mean, 1.0 / np.sqrt(var + float(np.float32(eps)))


def block_sums(x):
    """What the producing convolutions leave behind: per (64-row block, channel) {sum, sum of squares} as fp32, [n * P / 64, 2, C] from
    x [n, P, C] (P % 64 == 0) -- summed in fp64 and rounded once (the test's INPUT; its provenance does not matter to the kernels)."""
    x = np.asarray(x, dtype=np.float64)
    n, p, c = x.shape
    xb = x.reshape(n * p // 64, 64, c)
    return np.stack([xb.sum(1), (xb * xb).sum(1)], axis=1).astype(np.float32)


def gn_from_sums_ref(stats, n, hw, groups, eps=EPS):
    """Statistics from GIVEN fp32 block sums [n * hw / 64, 2, C] (the two sources concatenated along C): the reference is the fp64 sum of
    those fp32 numbers, not of the tensor they came from.  mean = S / cnt, var = max(Q / cnt - mean^2, 0) -- the formula is part of the
    operation here (there is no tensor to take a second pass over)."""
    s = np.asarray(stats, dtype=np.float64)
    nrb, c = hw // 64, s.shape[2]
    s = s.reshape(n, nrb, 2, groups, c // groups).sum(axis=(1, 4))          # [n, 2, groups]
    cnt = float(c // groups) * hw
    mean = s[:, 0] / cnt
    var = np.maximum(s[:, 1] / cnt - mean * mean, 0.0)
    return mean, 1.0 / np.sqrt(var + float(np.float32(eps)))


def finalize_gpb(n, groups):
    """Groups per workgroup of ds_gn_finalize (its one routing formula, restated): ceil(n groups / 512) clamped to [1, groups]."""
    return max(1, min(groups, -(-(n * groups) // 512)))


# ------------------------------------------------------------------------------------------------------------------------------
# 2. The {mu, A, B} planes:  A = rstd gamma (1 + scale),  B = beta (1 + scale) + shift   (gn_coefs: A = fl(fl(r gm) sc1), sc1 = fl(scale + 1),
#    B = fma(bt, sc1, sh)).  With r within k_r U relative of rstd (k_r = 3: one ulp = 2 U at worst, plus the rounding of the reference
#    itself; k_r = 1 when the test hands the kernel the rounded reference):
#      A: r (k_r) + sc1 (1) + r gm (1) + (.) sc1 (1)           -> gam(k_r + 3) |A|
#      B: sc1 (1) on the product, the fma's one rounding        -> U (1 + U) |bt (1 + scale)| + U |B|
#      mu: the fp32 mean, k_mu U |mean| (k_mu as k_r)

def planes_ref(mean, rstd, gamma, beta, scale, shift, c, k_stat=3):
    """mean, rstd: fp64 [n, G]; gamma, beta: [c] or None; scale, shift: [rows, c] (rows 1 or n) or None.  Returns the fp64 planes
    [n, 3, c] and their bound; k_stat: how many U the kernel's mean / rstd are from the reference's (3: computed on the device to one
    ulp; 1: the rounded reference, handed over; 0: no statistics, mu = 0 and r = 1 exactly)."""
    mean, rstd = np.asarray(mean, dtype=np.float64), np.asarray(rstd, dtype=np.float64)
    n, g = mean.shape
    cpg = c // g
    mu = np.repeat(mean, cpg, axis=1)
    r = np.repeat(rstd, cpg, axis=1)
    gm = np.ones(c) if gamma is None else np.asarray(gamma, dtype=np.float64)
    bt = np.zeros(c) if beta is None else np.asarray(beta, dtype=np.float64)
    sc1 = np.ones((1, c)) if scale is None else 1.0 + np.asarray(scale, dtype=np.float64).reshape(-1, c)
    sh = np.zeros((1, c)) if shift is None else np.asarray(shift, dtype=np.float64).reshape(-1, c)
    a = r * gm[None] * sc1
    b = np.broadcast_to(bt[None] * sc1 + sh, (n, c))
    planes = np.stack([mu, a, b], axis=1)
    bound = np.stack([k_stat * U * np.abs(mu), gam(k_stat + 3) * np.abs(a),
                      U * (1 + U) * np.abs(np.broadcast_to(bt[None] * sc1, (n, c))) + U * np.abs(b)], axis=1)
    return planes, bound * SECOND


# ------------------------------------------------------------------------------------------------------------------------------
# 3. The pass  y = resample(act((x - mu) A + B))   (gn_affine: t = fma(fl(x - mu), A, B); ds_silu; box filter ((v00 + v01) + (v10 + v11)) / 4)
#    With the kernel's mu within e_mu of the mean, A within e_A, B within e_B (section 2, or U |.| each when the test hands the kernel
#    rounded planes):
#      t:  e_mu |A|                    the fp32 mean (the term U |mu| |A|: the mean is stored in fp32 whatever the data's spread)
#        + U |x - mean| |A|            fl(x - mu)
#        + |x - mean| e_A + e_B        the coefficients
#        + U |t|                       the fma's rounding
#      SiLU: SILU_LIP e_t + (K_SILU + 2 |t| s(-t)) U |silu(t)| + SILU_ABS
#      identity form (no statistics, no gamma, no scale, no beta): t = x exactly, e_t = 0
#      2x2 box filter: (sum of the four bounds + U (|v00 + v01| + |v10 + v11| + |sum|)) / 4 -- three additions, the scaling by 1/4 is exact
#      nearest-neighbour x2: a copy
#      fp16 output: one more rounding, handled by inside(out16=True)

def _resample(v, mode):
    """v: [n, h, w, C] fp64; mode 0 none, 1 down (2x2 box), 2 up (nearest)."""
    if mode == 0:
        return v
    if mode == 2:
        return v.repeat(2, axis=1).repeat(2, axis=2)
    return ((v[:, 0::2, 0::2] + v[:, 0::2, 1::2]) + (v[:, 1::2, 0::2] + v[:, 1::2, 1::2])) * 0.25


def _resample_bound(v, b, mode):
    if mode != 1:
        return _resample(b, mode)
    s01, s23 = v[:, 0::2, 0::2] + v[:, 0::2, 1::2], v[:, 1::2, 0::2] + v[:, 1::2, 1::2]
    bs = (b[:, 0::2, 0::2] + b[:, 0::2, 1::2]) + (b[:, 1::2, 0::2] + b[:, 1::2, 1::2])
    return 0.25 * (bs + U * (np.abs(s01) + np.abs(s23) + np.abs(s01 + s23)))


def pass_ref(x, planes, plane_bound, act, resample, identity=False):
    """x: [n, h, w, C] (the concatenated input, any float dtype); planes / plane_bound: fp64 [n, 3, C] (section 2) -- None with `identity`.
    Returns fp64 (y, bound) [n, OH, OW, C]."""
    x = np.asarray(x, dtype=np.float64)
    if identity:
        t, et = x, np.zeros_like(x)
    else:
        mu, a, b = (planes[:, k][:, None, None, :] for k in range(3))
        emu, ea, eb = (plane_bound[:, k][:, None, None, :] for k in range(3))
        d = x - mu
        t = d * a + b
        et = (emu + U * np.abs(d)) * np.abs(a) + np.abs(d) * ea + eb + U * np.abs(t)
    if act:
        y = silu64(t)
        ey = SILU_LIP * et + (K_SILU + silu_exp_term(t)) * U * np.abs(y) + SILU_ABS
    else:
        y, ey = t, et
    return _resample(y, resample), _resample_bound(y, ey, resample) * SECOND


def raw_ref(x, resample):
    """The raw copy (raw_out): the resampled, concatenated, UN-normalised input.  fp16 in, fp16 out: a copy is exact; the box filter adds
    the widened values in fp32."""
    x = np.asarray(x, dtype=np.float64)
    return _resample(x, resample), _resample_bound(x, np.zeros_like(x), resample) * SECOND


# ------------------------------------------------------------------------------------------------------------------------------
# 4. LayerNorm rows (layernorm_rows_kernel: the row in registers, LPR lanes per row, two passes)
#      s:     every element passes through at most 2 (inside its quad) + 8 (the lane's quads) + 6 (shuffles) = 16 additions
#             -> |s - S| <= gam(16) sum |x|
#      mean:  inv_n = fl(1 / cols) (1), s inv_n (1)                        -> e_m = gam(16) mean|x| + 2 U |mean|
#      q:     d = fl(x - m) (1), d d (1), at most 32 + 6 additions of non-negative terms; sum (x - m)^2 = n var + n e_m^2 exactly (the cross
#             term vanishes), then q inv_n (2), + eps (1), sqrtf (1), 1 / (.) (1):
#             rstd relative: rho = (gam(2 * 2 + 38 + 3) + e_m^2 / (var + eps)) / 2 + 2 U
#      out:   fl(fl(fl(fl(x - m) r) g) + b), contracted or not:  (e_m + |x - mean| (rho + 3 U)) rstd |g| + U |out|

def layernorm_ref(x, gamma, beta, eps=EPS):
    """x: [rows, cols] (fp32 or fp16 values) -> fp64 (y, bound)."""
    x = np.asarray(x, dtype=np.float64)
    g, b = np.asarray(gamma, dtype=np.float64)[None], np.asarray(beta, dtype=np.float64)[None]
    mean = x.mean(1, keepdims=True)
    d = x - mean
    var = (d * d).mean(1, keepdims=True)
    ve = var + float(np.float32(eps))
    rstd = 1.0 / np.sqrt(ve)
    y = d * rstd * g + b
    e_m = gam(16) * np.abs(x).mean(1, keepdims=True) + 2 * U * np.abs(mean)
    rho = 0.5 * (gam(45) + e_m * e_m / ve) + 2 * U
    bound = (e_m + np.abs(d) * (rho + 3 * U)) * rstd * np.abs(g) + U * np.abs(y)
    return y, bound * SECOND


def layernorm_lanes(cols):
    """Lanes per row of the launcher (restated): 16 up to 512 columns, 32 up to 1024, 64 above."""
    n4 = cols // 4
    return 16 if n4 <= 128 else (32 if n4 <= 256 else 64)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. GEGLU  y = a gelu(g),  gelu(g) = 0.5 g (1 + erf(g / sqrt 2))   (geglu_kernel: a * (0.5f * g * (1.0f + erff(g * 0.70710678f))))
#      z = fl(g c), c = fl(1 / sqrt 2): 2 U |z| on the argument; |z erf'(z)| <= 0.484, so at most U on erf -- inside the measured constant,
#      which is the ABSOLUTE error of erff(fl(g c)) against erf(g / sqrt 2) in units of U (|erf| <= 1).
#      w = fl(1 + erf): at negative gates 1 + erf cancels, the absolute error K_ERF U stays: the term K_ERF U |a g / 2| -- absolute in w,
#      not relative to the result (at g = -6 the kernel returns -0 for -6e-9: erff is -1 exactly there).
#      fl(1 + erf) (1), (0.5 g) w (1; 0.5 g is exact), a (.) (1)            -> 3 U |y|

def geglu_ref(x, inner):
    """x: [rows, >= 2 inner] fp32 -> fp64 (y, bound) [rows, inner]."""
    x = np.asarray(x, dtype=np.float64)
    a, g = x[:, :inner], x[:, inner:2 * inner]
    erf = torch.erf(torch.from_numpy(np.ascontiguousarray(g)) * (0.5 ** 0.5)).numpy()
    y = a * (0.5 * g * (1.0 + erf))
    return y, (K_ERF * U * np.abs(a * 0.5 * g) + 3 * U * np.abs(y)) * SECOND


# ------------------------------------------------------------------------------------------------------------------------------
# 6. Noise embedding  out[b] = [cos | sin](c_noise(sigma_b) freqs)  (flag bit 0: [sin | cos]; bit 1: the argument is given, else log(sigma) / 4)
#      cn = logf(sigma) / 4: K_LOG U |cn| (the division by 4 is exact);  ang = fl(cn f): U |ang|;  |d cos|, |d sin| <= 1;
#      cosf / sinf: K_TRIG U |result|

def noise_embed_ref(sigma, freqs, swap):
    sigma, freqs = np.asarray(sigma, dtype=np.float64), np.asarray(freqs, dtype=np.float64)
    given = bool(swap & 2)
    cn = sigma if given else np.log(sigma) / 4.0
    ang = cn[:, None] * freqs[None]
    e_ang = np.abs(ang) * (U + (0.0 if given else K_LOG * U))
    cs, sn = np.cos(ang), np.sin(ang)
    first, second = (sn, cs) if swap & 1 else (cs, sn)
    y = np.concatenate([first, second], axis=1)
    bound = np.concatenate([e_ang, e_ang], axis=1) + K_TRIG * U * np.abs(y)
    return y, bound * SECOND


# ------------------------------------------------------------------------------------------------------------------------------
# fp32 emulations of the kernels' operation order on the CPU (tests/test_norm_refs_cpu.py: each must stay inside its bound).  numpy
# float32 arithmetic rounds every operation once, like the kernels; an fma is the fp64 product-sum rounded to fp32 (the product of two
# fp32 numbers is exact in fp64).  Transcendentals are the fp64 functions rounded once -- the emulation checks the DERIVED part of a
# bound, the measured constants are checked on the GPU.

f32 = np.float32


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def emulate_planes(mean, rstd, gamma, beta, scale, shift, c):
    m32, r32 = np.asarray(mean).astype(f32), np.asarray(rstd).astype(f32)
    n, g = m32.shape
    cpg = c // g
    gm = np.ones(c, f32) if gamma is None else np.asarray(gamma, f32)
    bt = np.zeros(c, f32) if beta is None else np.asarray(beta, f32)
    sc1 = np.ones((1, c), f32) if scale is None else (np.asarray(scale, f32).reshape(-1, c) + f32(1))
    sh = np.zeros((1, c), f32) if shift is None else np.asarray(shift, f32).reshape(-1, c)
    a = (np.repeat(r32, cpg, 1) * gm[None]) * sc1
    b = np.broadcast_to(_fma32(np.broadcast_to(bt[None], sc1.shape), sc1, sh), (n, c))
    return np.stack([np.repeat(m32, cpg, 1), a.astype(f32), b.astype(f32)], axis=1)


def emulate_pass(x, planes32, act, resample, identity=False, out16=False):
    x = np.asarray(x, f32)
    if identity:
        t = x
    else:
        mu, a, b = (planes32[:, k][:, None, None, :].astype(f32) for k in range(3))
        t = _fma32(x - mu, np.broadcast_to(a, x.shape), np.broadcast_to(b, x.shape))
    y = silu64(t.astype(np.float64)).astype(f32) if act else t
    if resample == 2:
        y = y.repeat(2, axis=1).repeat(2, axis=2)
    elif resample == 1:
        y = ((y[:, 0::2, 0::2] + y[:, 0::2, 1::2]) + (y[:, 1::2, 0::2] + y[:, 1::2, 1::2])) * f32(0.25)
    return y.astype(np.float16) if out16 else y


def emulate_layernorm(x, gamma, beta, eps=EPS):
    """The kernel's order: per lane the quads idx = lane + LPR i, (v0 + v1) + (v2 + v3) added to the lane's sum; xor-butterfly over the lanes."""
    x = np.asarray(x, f32)
    rows, cols = x.shape
    lpr, n4 = layernorm_lanes(cols), cols // 4
    xq = np.zeros((rows, 8 * lpr, 4), f32)
    xq[:, :n4] = x.reshape(rows, n4, 4)
    live = (np.arange(8 * lpr) < n4).reshape(8, lpr)            # [i, lane]
    xq = xq.reshape(rows, 8, lpr, 4)

    def reduce_lanes(v):                                        # v: [rows, lpr]
        o = lpr // 2
        while o > 0:
            v = v + v[:, np.arange(lpr) ^ o]
            o //= 2
        return v[:, :1]

    s = np.zeros((rows, lpr), f32)
    for i in range(8):
        s = np.where(live[i][None], s + ((xq[:, i, :, 0] + xq[:, i, :, 1]) + (xq[:, i, :, 2] + xq[:, i, :, 3])), s)
    inv_n = f32(1) / f32(cols)
    mean = reduce_lanes(s) * inv_n
    q = np.zeros((rows, lpr), f32)
    for i in range(8):
        for j in range(4):
            d = xq[:, i, :, j] - mean
            q = np.where(live[i][None], q + d * d, q)
    rstd = f32(1) / np.sqrt(reduce_lanes(q) * inv_n + f32(eps))
    return (x - mean) * rstd * np.asarray(gamma, f32)[None] + np.asarray(beta, f32)[None]


def emulate_geglu(x, inner):
    x = np.asarray(x, f32)
    a, g = x[:, :inner], x[:, inner:2 * inner]
    z = g * f32(0.70710678118654752440)
    erf = torch.erf(torch.from_numpy(np.ascontiguousarray(z.astype(np.float64)))).numpy().astype(f32)
    return a * (f32(0.5) * g * (f32(1) + erf))


def emulate_noise_embed(sigma, freqs, swap):
    sigma, freqs = np.asarray(sigma, f32), np.asarray(freqs, f32)
    cn = sigma if swap & 2 else (np.log(sigma.astype(np.float64)).astype(f32) / f32(4))
    ang = (cn[:, None] * freqs[None]).astype(f32)
    cs, sn = np.cos(ang.astype(np.float64)).astype(f32), np.sin(ang.astype(np.float64)).astype(f32)
    return np.concatenate([sn, cs] if swap & 1 else [cs, sn], axis=1)


# ------------------------------------------------------------------------------------------------------------------------------
# Case tables.  Every image has h != w unless it is a single pixel.

# ds_gn_stats.  in16: ds_norm_args.in_f16; partial: the small-batch scratch is given; P: the pixel chunks per image the launcher must
# choose (checked through ds_norm_route); const: group 0 of image 0 holds one constant.
StatsCase = namedtuple('StatsCase', 'name n c0 c1 ld0 ld1 h w groups in16 partial P const')


def _s(name, n, c0, c1, h, w, groups, *, ld0=None, ld1=None, in16=0, partial=False, P=1, const=False):
    return StatsCase(name, n, c0, c1, c0 if ld0 is None else ld0, c1 if ld1 is None else ld1, h, w, groups, in16, partial, P, const)


STATS_CASES = [
    _s('cpg1', 2, 64, 0, 3, 5, 64),                                   # a quad straddles 4 groups
    _s('cpg2_one_pixel', 2, 8, 0, 1, 1, 4),                           # 2 groups per quad; a single pixel
    _s('cpg3', 2, 12, 0, 3, 5, 4),                                    # quads straddle 2 groups at an odd offset
    _s('cpg5', 2, 40, 0, 5, 3, 8),
    _s('cpg125_idle_threads', 2, 1000, 0, 1, 9, 8),                   # 250 quads x 4 lanes: 24 idle threads
    _s('two_sources', 2, 4, 20, 3, 5, 2, ld0=8),                      # group 0 = channels 0..11 spans x0 | x1; ld0 > c0
    _s('two_sources_h0', 2, 4, 20, 3, 5, 2, ld0=8, in16=1),
    _s('two_sources_h1', 2, 4, 20, 3, 5, 2, ld0=8, ld1=24, in16=2),
    _s('two_sources_h01', 2, 4, 20, 3, 5, 2, ld0=8, ld1=24, in16=3),
    _s('c4096_one_lane', 1, 4096, 0, 1, 7, 32),
    _s('split_ragged', 3, 1024, 0, 6, 7, 32, partial=True, P=2),      # stride 8 over 42 pixels: the last stride is ragged
    _s('split_max', 1, 1024, 0, 16, 33, 32, partial=True, P=32),      # DS_GN_MAX_CHUNKS
    _s('split_tiny_image', 2, 64, 0, 2, 3, 16, partial=True, P=1),
    _s('split_n256', 256, 8, 0, 2, 3, 2, partial=True, P=1),
    _s('const_group', 2, 24, 0, 3, 5, 4, const=True),
    _s('const_group_split', 2, 512, 0, 8, 9, 32, partial=True, P=2, const=True),
]

CONST_VALUE = 30.5            # few significant bits: sums of it and of its square are exact in fp64


def stats_inputs(case, seed=0):
    """x [n, P, C] as fp32 values (fp16-representable in the channels of an fp16 source), `30 + randn`; gamma, beta [C]; scale, shift [n, 2C]
    (the tests use row 0 alone for ss_rows = 1)."""
    g = torch.Generator().manual_seed(2000 + seed)
    c = case.c0 + case.c1
    while True:
        x = 30.0 + torch.randn(case.n, case.h * case.w, c, generator=g)
        if case.in16 & 1:
            x[..., :case.c0] = x[..., :case.c0].half().float()
        if case.in16 & 2:
            x[..., case.c0:] = x[..., case.c0:].half().float()
        if case.const:
            x[0, :, :c // case.groups] = CONST_VALUE
        # a group of two or fifteen samples can come out nearly constant: draw again until E[x^2] / var <= 1e4 in every group (section 1)
        xg = x.double().reshape(case.n, case.h * case.w, case.groups, -1).permute(0, 2, 1, 3).reshape(case.n, case.groups, -1)
        var, ex2 = xg.var(-1, unbiased=False), (xg * xg).mean(-1)
        if bool(((ex2 <= 1e4 * var) | (var == 0)).all()):
            break
    return dict(x=x.numpy(), gamma=(1 + 0.3 * torch.randn(c, generator=g)).numpy(), beta=torch.randn(c, generator=g).numpy(),
                scale=(0.3 * torch.randn(case.n, 2 * c, generator=g)).numpy(), shift=torch.randn(case.n, 2 * c, generator=g).numpy())


# ds_gn_finalize.  null: the operand that is NULL ('gamma', 'beta', 'scale' (with shift), 'coefs') or None; neg: image 0's sums are
# replaced by ones whose Q / cnt - mean^2 is negative (-1e-6 mean^2: negative in any summation order).
FinCase = namedtuple('FinCase', 'name n c0 c1 hw groups null neg')

FINALIZE_CASES = (
    [FinCase(f'nrb{k}', 2, 64, 0, 64 * k, 32, None, False) for k in (1, 2, 3, 5, 16, 17)] +
    [FinCase(f'gpb{finalize_gpb(n, 32)}_n{n}', n, 64, 0, 64, 32, None, False) for n in (2, 17, 33)] +
    [FinCase('c512_per_block', 2, 1024, 0, 64, 2, None, False),
     FinCase('group_across_sources', 2, 20, 44, 192, 8, None, False),
     FinCase('gpb3_across_sources', 33, 20, 76, 128, 32, None, False)] +
    [FinCase(f'no_{k}', 3, 20, 44, 128, 8, k, False) for k in ('gamma', 'beta', 'scale', 'coefs')] +
    [FinCase('negative_variance', 2, 64, 0, 128, 32, None, True)])


def finalize_inputs(case, seed=0):
    g = torch.Generator().manual_seed(3000 + seed)
    c = case.c0 + case.c1
    x = 1.0 + torch.randn(case.n, case.hw, c, generator=g)              # E[x^2] / var = 2
    stats = block_sums(x.numpy())
    if case.neg:
        nrb, m = case.hw // 64, 1.5
        stats[:nrb, 0] = np.float32(64 * m)
        stats[:nrb, 1] = np.float32(64 * m * m * (1 - 1e-6))
    return dict(stats=stats, gamma=(1 + 0.3 * torch.randn(c, generator=g)).numpy(), beta=torch.randn(c, generator=g).numpy(),
                scale=(0.3 * torch.randn(case.n, 2 * c, generator=g)).numpy(), shift=torch.randn(case.n, 2 * c, generator=g).numpy())


# ds_norm_act.
#   form: 'identity' | 'beta' | 'gb' (gamma + beta, no statistics) | 'stats' (mean / rstd alone) | 'full' (mean / rstd + gamma + beta)
#         | 'ada' (full + scale / shift, one row per image) | 'planes' ({mu, A, B} given; fp16 out only) | 'fin' (the pass finalises
#         the given block sums itself; gamma + beta + scale / shift)
#   in16: ds_norm_args.in_f16;  out16, raw: fp16 output / with raw copy;  tune: ds_norm_args.tune_variant
#   kernel, rs: what ds_norm_route must answer (0: the 8-byte kernel; 1 / 2 / 3: the 16-byte kernel on planes / self-finalising / on
#               mean + rstd; rs: the launch resamples)
#   loops: the loops some workgroup must enter (pass_loops), besides whatever else it enters
#   mis: 'gamma' = gamma is a view one float into its allocation
PassCase = namedtuple('PassCase', 'name n c0 c1 ld0 ld1 h w groups form in16 out16 raw act resample out_pad tune kernel loops mis')


def _p(name, n, c0, c1, h, w, form, kernel, *, groups=1, ld0=None, ld1=None, in16=0, out16=0, raw=0, act=1, resample=0, out_pad=0, tune=0,
       loops=(), mis=None):
    return PassCase(name, n, c0, c1, c0 if ld0 is None else ld0, c1 if ld1 is None else ld1, h, w, groups, form, in16, out16, raw, act, resample,
                    out_pad, tune, kernel, tuple(loops), mis)


NONE, DOWN, UP = 0, 1, 2

PASS_CASES = (
    # the 8-byte kernel, fp32 -> fp32
    [_p(f'k0_f32_rs{rs}_{h}x{w}', 2, 8, 4, h, w, 'full', 0, groups=3, resample=rs, ld0=12, out_pad=4, loops=('tail',))
     for rs in (NONE, DOWN, UP) for (h, w) in ((2, 4), (4, 6), (3, 5)) if not (rs == DOWN and h == 3)] +
    [_p(f'k0_f32_{form}_rs{rs}', 2, 8, 4, 4, 6, form, 0, groups=3, resample=rs, act=act, loops=('tail',))
     for form, rs, act in (('identity', NONE, 1), ('identity', DOWN, 0), ('beta', NONE, 0), ('gb', UP, 1), ('stats', DOWN, 1), ('ada', NONE, 1))] +
    [_p('k0_mixed_h0', 2, 8, 4, 4, 6, 'full', 0, groups=3, in16=1, resample=DOWN, ld0=12, loops=('tail',)),
     _p('k0_mixed_h1', 2, 8, 4, 4, 6, 'ada', 0, groups=3, in16=2, resample=UP, ld1=8, loops=('tail',)),
     # fp16 out: planes as input with a raw copy; C = 12 is no whole octet, tune_variant 1 keeps a 16-byte shape on this kernel
     _p('k0_f16_planes_c12', 2, 8, 4, 4, 6, 'planes', 0, groups=3, in16=3, out16=1, raw=1, ld0=12, out_pad=4, loops=('tail',)),
     _p('k0_f16_planes_c12_down', 2, 8, 4, 4, 6, 'planes', 0, groups=3, in16=3, out16=1, raw=1, resample=DOWN, loops=('tail',)),
     _p('k0_f16_planes_tune1', 2, 16, 8, 4, 6, 'planes', 0, groups=3, in16=3, out16=1, raw=1, tune=1, ld0=24, loops=('tail',)),
     _p('k0_f16_full_tune1_up', 2, 16, 8, 4, 6, 'full', 0, groups=3, in16=3, out16=1, raw=1, tune=1, resample=UP, loops=('tail',)),
     _p('k0_f16_four_deep', 3, 64, 0, 8, 16, 'planes', 0, groups=4, in16=1, out16=1, raw=1, tune=1, loops=('four',)),
     # four pixels in flight followed by the one-pixel tail in one workgroup, ragged last trip: the least the launcher's 2048-workgroup rule
     # allows in fp32 (176 MB each way)
     _p('k0_f32_four_then_tail', 1024, 1024, 0, 6, 7, 'gb', 0, loops=('four+tail', 'ragged'))] +
    # the 16-byte kernel on planes (1) and on mean / rstd (3), sources 16 | 8 with ld0 = 24
    [_p(f'k{k}_rs{rs}', 2, 16, 8, 4, 6, form, k, groups=3, in16=3, out16=1, raw=1, resample=rs, ld0=24, out_pad=8,
        loops=('tail',) if rs != DOWN else ('down1',))
     for k, form in ((1, 'planes'), (3, 'ada')) for rs in (NONE, DOWN, UP)] +
    [_p('k1_one_octet', 2, 8, 0, 4, 6, 'planes', 1, in16=1, out16=1, loops=('tail',)),
     _p('k3_one_octet', 2, 8, 0, 4, 6, 'full', 3, groups=2, in16=1, out16=1, raw=1, loops=('tail',)),
     _p('k1_c2056_idle_threads', 1, 2056, 0, 2, 3, 'planes', 1, in16=1, out16=1, loops=('tail',)),
     _p('k3_c2056_idle_threads', 1, 2048, 8, 2, 3, 'full', 3, groups=8, in16=3, out16=1, raw=1, loops=('tail',)),
     _p('k1_c4096', 1, 4096, 0, 3, 5, 'planes', 1, in16=1, out16=1, raw=1, loops=('tail',)),
     _p('k3_c4096_up', 1, 4096, 0, 1, 3, 'full', 3, groups=32, in16=1, out16=1, resample=UP, loops=('four',)),
     _p('k1_down_two_deep_then_tail', 2, 1024, 0, 6, 10, 'planes', 1, in16=1, out16=1, raw=1, resample=DOWN, loops=('down2+down1',)),
     _p('k3_down_two_deep_then_tail', 2, 1024, 0, 6, 10, 'full', 3, groups=32, in16=1, out16=1, raw=1, resample=DOWN, loops=('down2+down1',)),
     _p('k1_four_deep', 2, 64, 0, 8, 32, 'planes', 1, in16=1, out16=1, raw=1, loops=('four',)),
     _p('k3_four_deep_prefetched', 2, 64, 0, 8, 32, 'ada', 3, groups=4, in16=1, out16=1, raw=1, loops=('four',)),
     _p('k3_up_four_deep', 2, 64, 0, 4, 8, 'full', 3, groups=4, in16=1, out16=1, raw=1, resample=UP, loops=('four',)),
     # four-deep and tail in ONE workgroup: the launcher's 16-pixels-per-thread branch (>= 16 M elements), 33 MB
     _p('k1_four_then_tail', 470, 1024, 0, 5, 7, 'planes', 1, in16=1, out16=1, raw=1, loops=('four+tail', 'ragged')),
     _p('k3_four_then_tail', 470, 1024, 0, 5, 7, 'full', 3, groups=32, in16=1, out16=1, loops=('four+tail', 'ragged'))] +
    # the self-finalising form at 1, 3 and 16 row blocks; a group spans x0 | x1 (16 | 8 in groups of 12; 72 | 56 in groups of 32)
    [_p('k2_nrb1', 2, 16, 8, 4, 16, 'fin', 2, groups=2, in16=3, out16=1, raw=1, ld0=24, out_pad=8, loops=('tail',))] +
    [_p(f'k2_nrb{hw // 64}_c128', 2, 72, 56, h, hw // h, 'fin', 2, groups=4, in16=3, out16=1, raw=1, ld0=80, out_pad=8, loops=('four',))
     for h, hw in ((4, 64), (8, 192), (16, 1024))] +
    # fix 2: a gamma that is not 16-byte aligned takes the 8-byte kernel in the mean / rstd form
    [_p('k3_gamma_misaligned_falls_back', 2, 16, 8, 4, 6, 'ada', 0, groups=3, in16=3, out16=1, raw=1, ld0=24, mis='gamma', loops=('tail',))])

# the 16-byte cases that tune_variant = 1 may legally send to the 8-byte kernel: the two kernels' outputs must be EQUAL bits
TUNE1_TWINS = [c.name for c in PASS_CASES if c.kernel in (1, 3)]


def pass_case(name):
    return next(c for c in PASS_CASES if c.name == name)


def out_hw(case):
    if case.resample == DOWN:
        return case.h // 2, case.w // 2
    if case.resample == UP:
        return case.h * 2, case.w * 2
    return case.h, case.w


def pass_inputs(case, seed=0):
    """The operands of one ds_norm_act case as numpy arrays: x [n, h, w, C] fp32 values (fp16-representable where the source is fp16);
    gamma / beta [C], scale / shift [n, C] or None by the case's form; `planes32` / `mean32`, `rstd32` (what the kernel is handed: the
    fp64 reference statistics rounded once -- k_stat = 1) or `stats` (block sums, form 'fin').  The large cases use cheap data: the values
    only have to differ per element."""
    g = torch.Generator().manual_seed(4000 + seed)
    c = case.c0 + case.c1
    x = torch.randn(case.n, case.h, case.w, c, generator=g)
    x.mul_(2.0).add_(0.7)
    if case.in16 & 1:
        x[..., :case.c0] = x[..., :case.c0].half().float()
    if case.in16 & 2:
        x[..., case.c0:] = x[..., case.c0:].half().float()
    x = x.numpy()
    d = dict(x=x, gamma=None, beta=None, scale=None, shift=None)
    form = case.form
    if form in ('gb', 'full', 'ada', 'planes', 'fin'):
        d['gamma'] = (1 + 0.3 * torch.randn(c, generator=g)).numpy()
    if form in ('beta', 'gb', 'full', 'ada', 'planes', 'fin'):
        d['beta'] = torch.randn(c, generator=g).numpy()
    if form in ('ada', 'planes', 'fin'):
        d['scale'] = (0.3 * torch.randn(case.n, c, generator=g)).numpy()
        d['shift'] = torch.randn(case.n, c, generator=g).numpy()
    return d


def pass_reference(case, d):
    """fp64 (y, bound, raw, raw_bound, extra) of a case; `extra` holds what the kernel is handed besides the operands of pass_inputs:
    mean32 / rstd32, planes32 or stats."""
    x = d['x']
    n, h, w, c = x.shape
    extra = {}
    if case.form == 'identity':
        y, b = pass_ref(x, None, None, case.act, case.resample, identity=True)
    else:
        flat = x.reshape(n, h * w, c)
        if case.form == 'fin':
            extra['stats'] = block_sums(flat)
            mean, rstd = gn_from_sums_ref(extra['stats'], n, h * w, case.groups)
            k = 3                                               # the pass's own statistics: one ulp of slack
        elif case.form in ('stats', 'full', 'ada', 'planes'):
            mean, rstd = gn_stats_ref(flat, case.groups)
            if case.form != 'planes':
                extra['mean32'], extra['rstd32'] = mean.astype(f32), rstd.astype(f32)
            k = 1                                               # the reference's statistics, rounded once
        else:                                                   # 'beta', 'gb': no statistics -- mu = 0, r = 1 exactly
            mean, rstd, k = np.zeros((n, 1)), np.ones((n, 1)), 0
        planes, pb = planes_ref(mean, rstd, d['gamma'], d['beta'], d['scale'], d['shift'], c, k)
        if case.form == 'planes':                               # the kernel is handed the rounded planes: U |.| each
            extra['planes32'] = planes.astype(f32)
            pb = U * np.abs(planes)
        y, b = pass_ref(x, planes, pb, case.act, case.resample)
    raw, rawb = raw_ref(x, case.resample) if case.raw else (None, None)
    return y, b, raw, rawb, extra


def pass_loops(case, lanes, chunk, chunks):
    """Which loops of the pass kernels the workgroups of a launch enter, from the geometry ds_norm_route reports (the kernels' loop
    headers restated): 'four' (four pixels in flight), 'tail' (one pixel), 'four+tail' (one thread runs both), 'down2' / 'down1' (the
    16-byte kernel's two-deep box-filter loop and its tail), 'down2+down1', 'ragged' (a last trip in which only some pixel lanes have
    a pixel)."""
    oh, ow = out_hw(case)
    ohw = oh * ow
    found = set()
    down16 = case.kernel != 0 and case.resample == DOWN
    four_ok = (case.resample == NONE) if case.kernel == 0 else (case.resample != DOWN)
    for b in range(chunks):
        p0, p1 = b * chunk, min(b * chunk + chunk, ohw)
        if (p1 - p0) % lanes:
            found.add('ragged')
        for pl in range(lanes):
            p, deep, tail = p0 + pl, 0, 0
            if down16:
                while p + lanes < p1:
                    p, deep = p + 2 * lanes, deep + 1
            elif four_ok:
                while p + 3 * lanes < p1:
                    p, deep = p + 4 * lanes, deep + 1
            while p < p1:
                p, tail = p + lanes, tail + 1
            names = ('down2', 'down1') if down16 else ('four', 'tail')
            if deep:
                found.add(names[0])
            if tail:
                found.add(names[1])
            if deep and tail:
                found.add(names[0] + '+' + names[1])
    return found


# LayerNorm: both sides of each lanes-per-row switch (512 | 1024 columns), the extremes, rows around a block's row count
LN_COLS = (4, 8, 508, 512, 516, 1020, 1024, 1028, 2044, 2048)
LN_ENTRIES = ('f32', 'f16out', 'f16io')


def ln_rows(cols):
    rpb = 256 // layernorm_lanes(cols)
    return (1, rpb - 1, rpb + 1)


LN_SECOND_TRIP = (65539, 4)            # 4096 workgroups x 16 rows = 65536 rows per trip of the grid stride


def ln_inputs(rows, cols, f16in, seed=0, const_row=True):
    g = torch.Generator().manual_seed(5000 + seed + 7 * rows + cols)
    x = 100.0 + torch.randn(rows, cols, generator=g)
    if const_row:
        x[rows // 2] = 1.5
    if f16in:
        x = x.half().float()
    return x.numpy(), (1 + 0.3 * torch.randn(cols, generator=g)).numpy(), torch.randn(cols, generator=g).numpy()


GEGLU_INNER = (4, 12, 1284)
GEGLU_GATES = (0.0, -0.0, 1e-30, -1e-30, 3.0, -3.0, 6.0, -6.0, 40.0, -40.0)
GEGLU_SECOND_TRIP = (2049, 8196)       # 16384 workgroups x 256 threads = 4 194 304 quads per trip; 2049 x 2049 quads: the second trip


def geglu_inputs(rows, inner, ldx, seed=0):
    g = torch.Generator().manual_seed(6000 + seed + rows + inner)
    x = torch.full((rows, ldx), float('nan'))
    x[:, :2 * inner] = torch.randn(rows, 2 * inner, generator=g) * 2
    gates = torch.tensor(GEGLU_GATES)
    k = min(len(gates), inner)
    x[0, inner:inner + k] = gates[:k]
    if rows > 1 and inner < len(gates):
        for r in range(1, rows):
            lo = (r * inner) % len(gates)
            seg = gates[lo:lo + inner]
            x[r, inner:inner + len(seg)] = seg
    return x.numpy()


# noise embedding: (bs, nch, out_ld); bs * nch / 2 = 7 * 10, 300 * 3 (several workgroups, the last one partly idle), 3 * 160
NOISE_SHAPES = ((7, 20, 24), (300, 6, 8), (3, 320, 320))


def noise_inputs(bs, nch, swap, seed=0):
    g = torch.Generator().manual_seed(7000 + seed + bs)
    lo, hi = math.log(0.002), math.log(80.0)
    sigma = torch.exp(torch.rand(bs, generator=g) * (hi - lo) + lo)
    half = nch // 2
    if swap & 2:                    # the argument is given: timesteps up to 1e3, the latent-diffusion frequencies
        sigma = torch.rand(bs, generator=g) * 1000.0
        freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half)
    else:                           # EDM's PositionalEmbedding: (1 / 10000)^(i / half), arguments log(sigma) / 4
        freqs = (1.0 / 10000.0) ** (torch.arange(half, dtype=torch.float32) / half)
    return sigma.numpy(), freqs.numpy()


# ------------------------------------------------------------------------------------------------------------------------------
# ds_norm_args of a case as a dict of field values (no library import here: the tests pass it to _lib.NormArgs(**fields)).  `ptr` maps an
# operand name to its address -- device addresses on the GPU, any aligned non-zero integers for ds_norm_route on the CPU.

FAKE = 0x10000


def fake_ptrs():
    return {k: FAKE * (i + 1) for i, k in enumerate(('x0', 'x1', 'mean', 'rstd', 'gamma', 'beta', 'scale', 'shift', 'out', 'coefs', 'partial',
                                                    'raw_out', 'stats0', 'stats1'))}


def stats_fields(case, ptr, ss_rows=1):
    c = case.c0 + case.c1
    f = dict(x0=ptr['x0'], x1=ptr['x1'] if case.c1 else None, c0=case.c0, c1=case.c1, ld0=case.ld0, ld1=case.ld1, n=case.n, h=case.h, w=case.w,
             groups=case.groups, eps=EPS, mean=ptr['mean'], rstd=ptr['rstd'], gamma=ptr['gamma'], beta=ptr['beta'], scale=ptr['scale'],
             shift=ptr['shift'], ss_ld=2 * c, ss_rows=ss_rows, coefs=ptr['coefs'], in_f16=case.in16)
    if case.partial:
        f['partial'] = ptr['partial']
    return f


def pass_fields(case, ptr):
    c = case.c0 + case.c1
    form = case.form
    f = dict(x0=ptr['x0'], x1=ptr['x1'] if case.c1 else None, c0=case.c0, c1=case.c1, ld0=case.ld0, ld1=case.ld1, n=case.n, h=case.h, w=case.w,
             groups=case.groups, eps=EPS, act=case.act, resample=case.resample, out=ptr['out'], out_ld=c + case.out_pad, out_f16=case.out16,
             in_f16=case.in16, tune_variant=case.tune, ss_ld=c, ss_rows=case.n)
    if form in ('stats', 'full', 'ada'):
        f.update(mean=ptr['mean'], rstd=ptr['rstd'])
    if form in ('gb', 'full', 'ada', 'fin'):
        f['gamma'] = ptr['gamma']
    if form in ('beta', 'gb', 'full', 'ada', 'fin'):
        f['beta'] = ptr['beta']
    if form in ('ada', 'fin'):
        f.update(scale=ptr['scale'], shift=ptr['shift'])
    if form == 'planes':
        f['coefs'] = ptr['coefs']
    if form == 'fin':
        f.update(stats0=ptr['stats0'], stats1=ptr['stats1'] if case.c1 else None)
    if case.raw:
        f.update(raw_out=ptr['raw_out'], raw_ld=c + case.out_pad)
    return f


# Calls the launchers must refuse before they launch anything: the return codes are DS_E_ARG -1, DS_E_ALIGN -2, DS_E_SHAPE -3.  Every entry
# starts from a case that runs and changes one thing; statistics pointers are always given (ds_gn_stats needs them, and the groups checks
# of ds_norm_act apply where mean is given).
REFUSALS = [
    # (name, base case, field changes, pointer offsets, expected ds_norm_act code or None, expected ds_gn_stats code or None)
    ('fin_tune1', 'k2_nrb1', dict(tune_variant=1), {}, -1, None),
    ('fin_gamma_misaligned', 'k2_nrb1', {}, dict(gamma=4), -2, None),
    ('fin_shift_misaligned', 'k2_nrb1', {}, dict(shift=4), -2, None),
    ('fin_ss_ld_odd', 'k2_nrb1', dict(ss_ld=26), {}, -2, None),
    ('groups_zero', 'k0_f32_rs0_4x6', dict(groups=0), {}, -3, -3),
    ('groups_do_not_divide', 'k0_f32_rs0_4x6', dict(groups=5), {}, -3, -3),
    ('groups_zero_f16', 'k3_rs0', dict(groups=0), {}, -3, -3),
    ('x0_f32_misaligned', 'k0_f32_rs0_4x6', {}, dict(x0=4), -2, -2),
    ('x1_f32_misaligned', 'k0_f32_rs0_4x6', {}, dict(x1=8), -2, -2),
    ('out_f32_misaligned', 'k0_f32_rs0_4x6', {}, dict(out=4), -2, None),
    ('x0_f16_misaligned_stats', 'k0_mixed_h0', {}, dict(x0=4), -1, -2),
    ('n_zero', 'k0_f32_rs0_4x6', dict(n=0), {}, -3, -3),
    ('h_zero', 'k0_f32_rs0_4x6', dict(h=0), {}, -3, -3),
    ('w_negative', 'k0_f32_rs0_4x6', dict(w=-2), {}, -3, -3),
    ('down_odd', 'k0_f32_rs2_3x5', dict(resample=1), {}, -3, None),
    ('x1_missing', 'k0_f32_rs0_4x6', dict(x1=None), {}, -1, -1),
    ('ld0_below_c0', 'k0_f32_rs0_4x6', dict(ld0=4), {}, -3, -3),
]


def refusal_fields(entry, ptr):
    name, base, changes, offs, _, _ = entry
    ptr = dict(ptr)
    for k, v in offs.items():
        ptr[k] += v
    f = pass_fields(pass_case(base), ptr)
    f.setdefault('mean', ptr['mean'])
    f.setdefault('rstd', ptr['rstd'])
    f.update(changes)
    return f
