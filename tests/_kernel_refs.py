"""Plain fp64 restatements of the solver-side kernels (csrc/solver.hip, csrc/gits.hip) and of the glue kernels of csrc/norm_act.hip,
the per-element error bounds the GPU tests hold the kernels to, and the tables of shapes / modes those tests run.

numpy / torch on the CPU only; nothing here imports the library.  tests/test_kernel_refs_cpu.py checks the references and the bounds
against independent evaluations on the CPU, tests/test_hip_solver_kernels.py and tests/test_hip_gits.py use them on the GPU.
"""
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24            # unit roundoff of fp32

# ------------------------------------------------------------------------------------------------------------------------------
# 1. ds_solver_update
#      D = raw ? c_skip x + c_out F : F     d = (x - D) / t     m = store_d ? d : D     x' = cx xb + cm m + sum_k ch_k hist_k
#      AFS: d = x / sqrt(1 + t^2), D = x - t d
#    coefficient rows (include/ds_engine.h): 0 cx, 1 cm, 2..4 ch[0..2], 5 t, 6 sigma, 7 unused

UpdCase = namedtuple('UpdCase', 'name n c h w mode nhist xb_distinct outs store_d coef misalign')
#   mode: 'raw4' / 'raw8' (raw NHWC rows of f_ld = 4 / 8 floats), 'planar' (raw, f_ld = 0), 'nonraw' (F is the denoised tensor), 'afs'
#   outs: 'x', 'm', 'both';  coef: 'host' (hcoefs by value), 'dev1' (device row shared), 'devn' (one device row per sample)
#   misalign: None or the operand that is a view starting one float into its allocation ('xe', 'f', 'hist1', 'm_out', 'x_out')


def _u(name, shape, mode, nhist, xbd, outs, sd, coef, mis=None, n=3):
    c, h, w = shape
    return UpdCase(name, n, c, h, w, mode, nhist, bool(xbd), outs, int(sd), coef, mis)


UPDATE_CASES = [
    # solver_update_fast_kernel<3> / <4>: c in {3, 4}, H*W % 4 == 0, everything 16-byte aligned, raw rows of exactly 4 floats or planar
    _u('fast3_quad_raw4', (3, 2, 2), 'raw4', 0, 0, 'both', 1, 'host'),
    _u('fast4_quad_raw4', (4, 2, 2), 'raw4', 1, 1, 'both', 0, 'devn'),
    _u('fast3_planar', (3, 4, 6), 'planar', 2, 1, 'x', 1, 'dev1'),
    _u('fast4_nonraw_3h', (4, 2, 2), 'nonraw', 3, 0, 'both', 0, 'host'),
    _u('fast3_afs', (3, 4, 6), 'afs', 1, 0, 'both', 1, 'devn'),
    _u('fast4_afs_3h_m', (4, 2, 2), 'afs', 3, 1, 'm', 0, 'dev1'),
    _u('fast3_nonraw_m', (3, 2, 2), 'nonraw', 0, 1, 'm', 1, 'devn'),
    _u('fast4_planar_3h', (4, 2, 2), 'planar', 3, 0, 'x', 0, 'devn'),
    _u('fast3_raw4_2h', (3, 4, 6), 'raw4', 2, 1, 'both', 1, 'dev1'),
    # solver_update_kernel<4>: vec4-eligible, but another channel count, raw rows of 8 floats, or raw rows of 4 at a misaligned address
    _u('gen_c1_raw4', (1, 2, 2), 'raw4', 0, 0, 'both', 1, 'host'),
    _u('gen_c2_raw4_2h', (2, 4, 6), 'raw4', 2, 1, 'both', 0, 'devn'),
    _u('gen_c5_raw8_3h', (5, 2, 2), 'raw8', 3, 0, 'both', 1, 'devn'),
    _u('gen_c8_planar', (8, 4, 6), 'planar', 1, 1, 'x', 0, 'dev1'),
    _u('gen_c5_nonraw', (5, 4, 6), 'nonraw', 2, 0, 'both', 1, 'dev1'),
    _u('gen_c8_afs_3h', (8, 2, 2), 'afs', 3, 1, 'both', 0, 'host'),
    _u('gen_c1_afs_m', (1, 4, 6), 'afs', 0, 0, 'm', 1, 'devn'),
    _u('gen_c2_nonraw_x', (2, 2, 2), 'nonraw', 1, 1, 'x', 0, 'host'),
    _u('gen_c5_raw8_0h', (5, 4, 6), 'raw8', 0, 1, 'm', 0, 'host'),
    _u('gen_c3_raw4_f_off', (3, 4, 4), 'raw4', 1, 0, 'both', 1, 'devn', 'f'),
    _u('gen_c4_raw8', (4, 2, 2), 'raw8', 2, 0, 'both', 0, 'dev1'),
    # solver_update_kernel<1> by shape: H*W % 4 != 0
    _u('sc_3x5x5_raw4', (3, 5, 5), 'raw4', 2, 0, 'both', 1, 'devn'),
    _u('sc_4x3x3_raw4_3h', (4, 3, 3), 'raw4', 3, 1, 'both', 0, 'host'),
    _u('sc_5x1x1_raw8', (5, 1, 1), 'raw8', 1, 0, 'both', 1, 'dev1'),
    _u('sc_3x5x5_planar', (3, 5, 5), 'planar', 0, 1, 'x', 0, 'dev1'),
    _u('sc_4x3x3_nonraw', (4, 3, 3), 'nonraw', 3, 0, 'x', 1, 'devn'),
    _u('sc_5x1x1_afs_m', (5, 1, 1), 'afs', 2, 1, 'm', 0, 'host'),
    _u('sc_3x5x5_afs', (3, 5, 5), 'afs', 1, 0, 'both', 1, 'devn'),
    _u('sc_4x3x3_planar_m', (4, 3, 3), 'planar', 1, 1, 'm', 1, 'host'),
    # the second trip of each kernel's grid-stride loop (4096 blocks x 256 threads), cheapest operands
    _u('trip2_scalar', (1, 3, 116509), 'nonraw', 0, 0, 'm', 1, 'host', n=3),
    _u('trip2_generic', (1, 4, 524289), 'nonraw', 0, 0, 'm', 1, 'host', n=2),
    _u('trip2_fast', (3, 4, 524289), 'nonraw', 0, 0, 'm', 1, 'host', n=2),
]
# solver_update_kernel<1> by alignment at (3, 4, 4): one operand at a time one float into its allocation
MISALIGNED_OPERANDS = ('xe', 'f', 'hist1', 'm_out', 'x_out')
MISALIGN_BASE = _u('sc_align', (3, 4, 4), 'nonraw', 2, 1, 'both', 1, 'devn')
MISALIGN_AFS = _u('sc_align_afs', (3, 4, 4), 'afs', 2, 1, 'both', 1, 'devn')


def update_f_ld(case):
    return {'raw4': 4, 'raw8': 8}.get(case.mode, 0)


def expected_update_kernel(case):
    """The kernel ds_solver_update launches for a case: the launcher's rule (csrc/solver.hip) restated from the case's own description.
    A misaligned operand takes the 16-byte kernels away -- except raw NHWC rows, which the generic kernel reads with scalar loads at any
    address (only the streaming kernel wants them aligned)."""
    rows = case.mode in ('raw4', 'raw8')
    if case.misalign is not None:
        assert case.misalign in MISALIGNED_OPERANDS
        assert not (case.misalign == 'f' and case.mode == 'afs'), 'AFS reads no F'
        assert case.misalign != 'hist1' or case.nhist >= 2
        assert case.misalign not in ('m_out', 'x_out') or case.outs in ('both', case.misalign[0])
    vec4 = (case.h * case.w) % 4 == 0 and (case.misalign is None or (case.misalign == 'f' and rows))
    if not vec4:
        return 'scalar'
    fast = case.c in (3, 4) and (not rows or (case.mode == 'raw4' and case.misalign != 'f'))
    return 'fast' if fast else 'generic'


def update_inputs(case, seed=0):
    """Seeded operands of one case, fp32 on the CPU: xe, xb (xe itself unless the case wants it distinct), F as an NCHW tensor, three
    history tensors, and an [n, 8] coefficient table whose rows all differ ('devn') or repeat row 0 (one shared set of scalars).
    t and sigma are log-uniform in [0.002, 80], the combination coefficients uniform in [-2, 2]."""
    g = torch.Generator().manual_seed(1000 + seed)
    shape = (case.n, case.c, case.h, case.w)
    xe = torch.randn(shape, generator=g) * 3
    xb = torch.randn(shape, generator=g) * 3 if case.xb_distinct else xe
    f = torch.randn(shape, generator=g)
    hist = [torch.randn(shape, generator=g) for _ in range(3)]
    coefs = torch.zeros(case.n, 8)
    coefs[:, :5] = torch.rand(case.n, 5, generator=g) * 4 - 2
    lo, hi = math.log(0.002), math.log(80.0)
    coefs[:, 5:7] = torch.exp(torch.rand(case.n, 2, generator=g) * (hi - lo) + lo)
    if case.coef != 'devn':
        coefs[:] = coefs[0].clone()
    return dict(xe=xe, xb=xb, f=f, hist=hist[:case.nhist], coefs=coefs, sigma_data=0.5)


def nhwc_rows(f, f_ld):
    """NCHW [n, c, h, w] -> the raw network output's rows [n*h*w, f_ld]; the columns past c hold NaN (the kernel must not use them)."""
    n, c, h, w = f.shape
    rows = torch.full((n * h * w, f_ld), float('nan'), dtype=f.dtype)
    rows[:, :c] = f.permute(0, 2, 3, 1).reshape(-1, c)
    return rows


def _r4(v):
    return v.reshape(-1, 1, 1, 1)


def solver_update_ref(xe, xb, f, hist, coefs, sigma_data, mode, store_d):
    """fp64 (m, x', bound on |m - m_ref|, bound on |x' - x'_ref|), all [n, c, h, w], from fp32 operands and an fp32 [n, 8] table."""
    k = coefs.double()
    cx, cm, t, sig = _r4(k[:, 0]), _r4(k[:, 1]), _r4(k[:, 5]), _r4(k[:, 6])
    x = xe.double()
    if mode == 'afs':
        d = x / torch.sqrt(1 + t * t)
        D = x - t * d
        M = d.abs() if store_d else x.abs() + (t * d).abs()
    else:
        fd = f.double()
        if mode in ('raw4', 'raw8', 'planar'):
            sd = float(np.float32(sigma_data))
            c_skip = sd * sd / (sig * sig + sd * sd)
            c_out = sig * sd / torch.sqrt(sig * sig + sd * sd)
            D = c_skip * x + c_out * fd
            Dm = (c_skip * x).abs() + (c_out * fd).abs()
        else:
            D, Dm = fd, fd.abs()
        d = (x - D) / t
        M = (x.abs() + Dm) / t if store_d else Dm
    m = d if store_d else D
    xo = cx * xb.double() + cm * m
    mag = (cx * xb.double()).abs() + cm.abs() * M
    for j, h in enumerate(hist):
        ch = _r4(k[:, 2 + j])
        xo = xo + ch * h.double()
        mag = mag + (ch * h.double()).abs()
    return m, xo, 8 * U * M, 16 * U * mag


def solver_update_fp32(xe, xb, f, hist, coefs, sigma_data, mode, store_d):
    """The same formulas evaluated in fp32 by torch on the CPU (each operation rounded on its own): (m, x')."""
    k = coefs.float()
    cx, cm, t, sig = _r4(k[:, 0]), _r4(k[:, 1]), _r4(k[:, 5]), _r4(k[:, 6])
    x = xe.float()
    if mode == 'afs':
        d = x / torch.sqrt(1 + t * t)
        D = x - t * d
    else:
        if mode in ('raw4', 'raw8', 'planar'):
            sd = torch.tensor(sigma_data, dtype=torch.float32)
            c_skip = sd * sd / (sig * sig + sd * sd)
            c_out = sig * sd / torch.sqrt(sig * sig + sd * sd)
            D = c_skip * x + c_out * f.float()
        else:
            D = f.float()
        d = (x - D) / t
    m = d if store_d else D
    xo = cx * xb.float() + cm * m
    for j, h in enumerate(hist):
        xo = xo + _r4(k[:, 2 + j]) * h.float()
    return m, xo


# ------------------------------------------------------------------------------------------------------------------------------
# 2. quantile kernels (ds_dynamic_threshold, ds_dpmpp_x0_step): torch.quantile semantics at p = 0.995

QUANTILE_P = 0.995
QUANTILE_PERS = (2, 3, 200, 201, 513, 1001, 38144)
QUANTILE_LDS_CAP = 38144                       # (per + 256) * 4 <= 150 KiB
QUANTILE_KINDS = ('gauss3', 'equal', 'below1', 'ties', 'huge')
X0_STEP_SHAPES = ((5, 3, 7), (1, 1, 2), (3, 5, 5))
X0_STEP_REG_SHAPE = (3, 16, 16)                # 768 values per sample: the register-resident kernel


def fp32_rank(per, p=QUANTILE_P):
    """(rank, lo, hi) of torch.quantile's interpolation, rank = p * (per - 1) in fp32 as ATen and the kernels compute it."""
    rank = np.float32(p) * np.float32(per - 1)
    return float(rank), int(np.floor(rank)), int(np.ceil(rank))


def quantile_inputs(kind, per, seed=0):
    """[4, per] fp32 samples of one input kind (no NaN / Inf)."""
    g = torch.Generator().manual_seed(2000 + seed + per)
    n = 4
    if kind == 'gauss3':
        return torch.randn(n, per, generator=g) * 3
    if kind == 'equal':                         # every value of a sample equal: above 1, negative, below 1, exactly 1
        return torch.tensor([2.5, -3.0, 0.25, 1.0]).reshape(n, 1).repeat(1, per).contiguous()
    if kind == 'below1':                        # s clamps to 1: the output is the input
        return torch.rand(n, per, generator=g) * 1.98 - 0.99
    if kind == 'huge':
        x = torch.randn(n, per, generator=g) * 3
        for b in range(n):
            x[b, int(torch.randint(per, (1,), generator=g))] = 1e30 if b % 2 == 0 else -1e30
        return x
    if kind == 'ties':
        # the two order statistics around the rank carry the same |x| with both signs.  Sample 0: all +-0; sample 1: all +- one fp32
        # denormal; samples 2, 3: a run of +-2.5 across [lo - 1, hi + 1] inside sorted magnitudes, with signed zeros and denormals below it
        _, lo, hi = fp32_rank(per)
        sign = lambda k: (torch.randint(2, (k,), generator=g) * 2 - 1).float()
        x = torch.zeros(n, per)
        x[0] = 0.0 * sign(per)
        x[1] = 1e-40 * sign(per)
        for b in (2, 3):
            a, z = max(lo - 1, 0), min(hi + 2, per)
            mag = torch.empty(per)
            mag[:a] = torch.rand(a, generator=g) * 2.0
            mag[a:z] = 2.5
            mag[z:] = 2.5 + torch.rand(per - z, generator=g) * 1.5
            if a >= 4:
                mag[:4] = torch.tensor([0.0, 0.0, 1e-40, 3e-39])
            x[b] = (mag * sign(per))[torch.randperm(per, generator=g)]
        return x
    raise ValueError(kind)


# ------------------------------------------------------------------------------------------------------------------------------
# 3. GITS costs (csrc/gits.hip, gits_utils._cost_matrix_round): every pair i < j of a teacher trajectory, from the definition

TRAJ_SHAPES = ((2, 1, 1), (7, 3, 75), (9, 2, 1030))          # (n_pts, batch, per)


def synthetic_trajectory(n_pts, B, per, seed=0):
    """(traj [n_pts, B, per] fp32, eps [n_pts - 1, B, per] fp32, t: list of n_pts floats holding fp32 values) -- a curved path from noise
    at t_0 = 80 to a sample at t = 0.002, with directions that are not tangent to it.  Needs no network."""
    g = torch.Generator().manual_seed(3000 + seed)
    i = torch.arange(n_pts, dtype=torch.float32)
    t = (80.0 ** (1 / 7) + i / max(n_pts - 1, 1) * (0.002 ** (1 / 7) - 80.0 ** (1 / 7))) ** 7
    c = torch.randn(B, per, generator=g)
    e = torch.randn(B, per, generator=g)
    traj = torch.stack([c + t[k] * (e + 0.3 * torch.randn(B, per, generator=g)) for k in range(n_pts)])
    traj[-1] = c
    eps = torch.stack([e + 0.5 * torch.randn(B, per, generator=g) for _ in range(n_pts - 1)])
    return traj.contiguous(), eps.contiguous(), [float(v) for v in t.tolist()]


def degenerate_trajectory():
    """Every point ON the start->end chord and every direction along it, exactly in fp32 (small integers times dyadic fractions): the
    'dev' cost is 0 by definition and the closed form cancels down to the square root of its fp64 rounding noise."""
    g = torch.Generator().manual_seed(3999)
    B, per = 2, 40
    c = torch.randint(-8, 9, (B, per), generator=g).float()
    e = torch.randint(-4, 5, (B, per), generator=g).float()
    t = [8.0, 6.5, 5.0, 3.25, 2.0, 0.75, 0.0]
    traj = torch.stack([c + tk * e for tk in t])
    eps = torch.stack([a * e for a in (1.0, 0.5, 1.25, 2.0, 0.75, 1.5)])
    return traj.contiguous(), eps.contiguous(), t


def traj_moments_ref(traj, eps=None):
    """([n_pts, B, 6] fp64 {P, Q, R, S, T, N}, the same with |products| summed) by numpy dot products."""
    x = traj.double().numpy().reshape(traj.shape[0], traj.shape[1], -1)
    n = x.shape[0]
    d = np.zeros_like(x)
    if eps is not None:
        d[:n - 1] = eps.double().numpy().reshape(n - 1, x.shape[1], -1)
    c, bc = x[-1][None], (x[-1] - x[0])[None]
    cx = c - x
    prods = [cx * bc, d * bc, cx * cx, cx * d, d * d, np.broadcast_to(bc * bc, x.shape)]
    return np.stack([p.sum(-1) for p in prods], -1), np.stack([np.abs(p).sum(-1) for p in prods], -1)


def dev_closed_form(m, t):
    """The 'dev' cost matrix from the six moments (the closed form of csrc/gits.hip's header), restated: [n, n] fp64, zero where j <= i."""
    P, Q, R, S, T, N = (m[:, :, k] for k in range(6))
    n = m.shape[0]
    t = np.asarray(t, dtype=np.float64)
    tea = np.zeros(n)                                        # teacher deviation at point j (0 at both ends)
    tea[1:n - 1] = np.sqrt(np.maximum(R[1:n - 1] - P[1:n - 1] ** 2 / N[1:n - 1], 0.0)).mean(axis=1)
    cost = np.zeros((n, n))
    for i in range(n - 1):
        for j in range(i + 1, n):
            D = t[j] - t[i]
            val = R[i] - 2 * D * S[i] + D * D * T[i] - (P[i] - D * Q[i]) ** 2 / N[i]
            cost[i, j] = np.sqrt(np.maximum(val, 0.0)).mean() - tea[j]
    return cost


def _perp_norm(v, bc):
    """|v - (v.bc / |bc|^2) bc| per sample; v, bc: [B, per] fp64."""
    coef = (v * bc).sum(-1, keepdims=True) / (bc * bc).sum(-1, keepdims=True)
    return np.sqrt(((v - coef * bc) ** 2).sum(-1))


def pair_costs_ref(traj, eps, t, metric):
    """(cost [n, n], tol [n, n]) fp64, straight from the definition (gits-main/gits_utils.py:108-132), mean over the batch, zero where
    j <= i.  tol is the bound the device result is held to:
      'dev'  1e-12 * s,  s = sqrt(|c - x_i|^2 + D^2 |d_i|^2)           (fp64 closed form; `degenerate=True` callers use 1e-7 * s)
      'l1'   3 * 2^-24 * sum_e (|x_i| + |D d_i| + |x_j|)               (the kernel forms x_next and the difference in fp32)
      'l2'   the 2-norm of the same per-element bound"""
    x = traj.double().numpy().reshape(traj.shape[0], traj.shape[1], -1)
    n = x.shape[0]
    d = eps.double().numpy().reshape(n - 1, x.shape[1], -1)
    t = np.asarray(t, dtype=np.float64)
    c, bc = x[-1], x[-1] - x[0]
    cost, tol = np.zeros((n, n)), np.zeros((n, n))
    tea = np.zeros(n)
    for j in range(1, n - 1):
        tea[j] = _perp_norm(c - x[j], bc).mean()
    for i in range(n - 1):
        for j in range(i + 1, n):
            D = t[j] - t[i]
            x_next = x[i] + D * d[i]
            if metric == 'dev':
                cost[i, j] = _perp_norm(c - x_next, bc).mean() - tea[j]
                tol[i, j] = 1e-12 * np.sqrt(((c - x[i]) ** 2).sum(-1) + D * D * (d[i] ** 2).sum(-1)).mean()
            else:
                r = x_next - x[j]
                el = 3 * U * (np.abs(x[i]) + np.abs(D * d[i]) + np.abs(x[j]))
                if metric == 'l1':
                    cost[i, j], tol[i, j] = np.abs(r).sum(-1).mean(), el.sum(-1).mean()
                elif metric == 'l2':
                    cost[i, j], tol[i, j] = np.sqrt((r * r).sum(-1)).mean(), np.sqrt((el * el).sum(-1)).mean()
                else:
                    raise ValueError(metric)
    return cost, tol


def deviation_ref(traj):
    """cal_deviation from the definition: [B, n_pts - 2] fp64, and R = |c - x_j|^2 [B, n_pts - 2] (the scale of its closed form)."""
    x = traj.double().numpy().reshape(traj.shape[0], traj.shape[1], -1)
    c, bc = x[-1], x[-1] - x[0]
    dev = np.stack([_perp_norm(c - x[j], bc) for j in range(1, x.shape[0] - 1)], -1) if x.shape[0] > 2 else np.zeros((x.shape[1], 0))
    R = np.stack([((c - x[j]) ** 2).sum(-1) for j in range(1, x.shape[0] - 1)], -1) if x.shape[0] > 2 else np.zeros((x.shape[1], 0))
    return dev, R


# ------------------------------------------------------------------------------------------------------------------------------
# 4. glue kernels

def quantize_ref(x):
    """(x * 127.5 + 128).clip(0, 255).to(uint8) in fp32, product and sum rounded separately (ATen), as NHWC."""
    return (x * 127.5 + 128).clip(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def quantize_fma_ref(x):
    """The same with ONE rounding of x * 127.5 + 128 (what a fused multiply-add computes; exact in fp64 before the rounding)."""
    v = (x.double() * 127.5 + 128).float()
    return v.clip(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def quantize_edge_values():
    """fp32 inputs around every quantisation step: for each level k the input nearest (k - 128) / 127.5 and its 8 neighbours on each side
    (some land exactly on the integer after x * 127.5 + 128, some just below it), plus inputs below -1 and above 1."""
    base = ((torch.arange(0, 257, dtype=torch.float64) - 128) / 127.5).float()
    vals = [base]
    up, dn = base.clone(), base.clone()
    for _ in range(8):
        up = torch.nextafter(up, torch.tensor(float('inf')))
        dn = torch.nextafter(dn, torch.tensor(float('-inf')))
        vals += [up.clone(), dn.clone()]
    vals.append(torch.tensor([-1.0000001, -1.5, -1e30, -1.0, 1.0, 1.0000001, 2.0, 1e30, 0.0, -0.0, 0.99999994, -0.99999994]))
    return torch.cat(vals)


def quantize_inputs(n, c, h, w, seed=0):
    """[n, c, h, w] fp32: the edge values tiled through the tensor, the rest uniform in [-1.3, 1.3]."""
    g = torch.Generator().manual_seed(4000 + seed)
    x = torch.rand(n * c * h * w, generator=g) * 2.6 - 1.3
    e = quantize_edge_values()
    k = min(e.numel(), x.numel())
    x[torch.randperm(x.numel(), generator=g)[:k]] = e[torch.randperm(e.numel(), generator=g)[:k]]
    return x.reshape(n, c, h, w)


def c_in64(sigma, sigma_data):
    """EDM c_in = 1 / sqrt(sigma_data^2 + sigma^2) in fp64 from fp32 sigma / sigma_data."""
    sd = float(np.float32(sigma_data))
    return 1.0 / torch.sqrt(sd * sd + sigma.double() ** 2)


def stem_im2col_ref(x, sigma, sigma_data, kpad):
    """[n*h*w, kpad] fp64: F.unfold of c_in * x (3x3, zero padding 1), columns re-ordered to k = tap * c + ch, zero-padded to kpad.
    sigma: [n] or [1] fp32."""
    n, c, h, w = x.shape
    xs = x.double() * c_in64(sigma, sigma_data).reshape(-1, 1, 1, 1)
    cols = F.unfold(xs, 3, padding=1).reshape(n, c, 9, h * w)              # unfold's rows are ch * 9 + tap
    cols = cols.permute(0, 3, 2, 1).reshape(n * h * w, 9 * c)              # -> [pixel, tap * c + ch]
    out = torch.zeros(n * h * w, kpad, dtype=torch.float64)
    out[:, :9 * c] = cols
    return out


def channel_mean_bound(x_rows, c):
    """(ceil(c / 64) + 7) * 2^-24 * mean|x| per row; x_rows: [rows, c]."""
    return (math.ceil(c / 64) + 7) * U * x_rows.double().abs().mean(-1)


SOFTMAX_SHAPES = ((1, 1, 1), (5, 77, 80), (7, 130, 130), (4, 1000, 1000))        # (rows, cols, ld)


def softmax_inputs(rows, cols, seed=0):
    """[rows, cols] fp32: Gaussian * 8; where the rows exist, row 1 is constant, row 2 sits at an offset of 1e4 and row 3 has its maximum
    in the last column."""
    g = torch.Generator().manual_seed(5000 + seed)
    x = torch.randn(rows, cols, generator=g) * 8
    if rows > 1:
        x[1] = -3.75
    if rows > 2:
        x[2] += 1e4
    if rows > 3:
        x[3, -1] = x[3].max() + 5.0
    return x
