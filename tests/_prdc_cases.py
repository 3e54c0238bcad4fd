"""Inputs and the independent reference of the precision / recall / density / coverage tests (test_prdc_cpu.py, test_hip_prdc.py).

The reference here is the DIRECT restatement  d2(i, j) = sum_c (x_ic - y_jc)^2  in numpy fp64 -- no expansion into norms and a dot
product, no matrix pipe -- followed by a sort.  References are computed once per case (lru_cache) and never modified by a test."""
import functools

import numpy as np


def features(n, d, seed, shift=0.0, dtype=np.float32):
    """The generator of tests/test_hip_fid.py (correlated Gaussians, an offset per feature; ``shift`` moves the fake set)."""
    g = np.random.RandomState(seed)
    a = g.randn(d, d) / np.sqrt(d)
    return (g.randn(n, d) @ a + shift + 0.3 * g.randn(d)).astype(dtype)


def direct_sq(x, y, block=32):
    """sum_c (x_ic - y_jc)^2, features in order, in row blocks that stay in cache."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    out = np.zeros((x.shape[0], y.shape[0]), dtype=np.float64)
    yt = np.ascontiguousarray(y.T)
    tmp = np.empty((block, y.shape[0]), dtype=np.float64)
    for a in range(0, x.shape[0], block):
        xb, o = x[a:a + block], out[a:a + block]
        t = tmp[:xb.shape[0]]
        for c in range(x.shape[1]):
            np.subtract(xb[:, c:c + 1], yt[c][None, :], out=t)
            np.multiply(t, t, out=t)
            o += t
    return out


def radii_sq_of(d_self, k):
    """(k + 1)-th smallest of every row of a self-distance matrix (its diagonal is exactly 0 in the direct form), with multiplicity."""
    return np.sort(d_self, axis=1)[:, k]


def cross_ref(d, rr, rf, mask=None):
    """-> fake_count, real_hit, real_min_sq, realism_sq (None without a mask) from the squared distances d[real][fake], strict <."""
    count = (d < rr[:, None]).sum(0)
    hit = (d < rf[None, :]).sum(1)
    mn = d.min(1)
    rls = None
    if mask is not None:
        with np.errstate(divide='ignore', invalid='ignore'):
            rls = (rr[mask][:, None] / d[mask]).max(0)
    return count, hit, mn, rls


def metrics_ref(count, hit, mn, rr, k):
    """The reference's finalisation (its expression order) on the squared-domain statistics."""
    return dict(precision=(count > 0).mean(), recall=(hit > 0).mean(), density=(1. / float(k)) * count.mean(), coverage=(mn < rr).mean())


def realism_mask(rr):
    radii = np.sqrt(rr)
    return radii < np.median(radii)


# ---- Gaussian cases of the GPU tests: (n_real, n_fake, dim) -> seed.  A seed that fails `conditions` is REPLACED here, never skipped.
GAUSS_SEEDS = {(37, 41, 7): 101, (130, 333, 50): 102, (300, 257, 64): 103, (1000, 777, 96): 104}
GAUSS_K = 5


@functools.lru_cache(maxsize=None)
def gauss_case(n_real, n_fake, dim, f64=False):
    """real [n_real][dim + 8], fake [n_fake][dim + 8] (the kernel is handed ld = dim + 8 and must ignore the last 8 columns) and the
    direct reference on the first dim columns: radii_sq of both sets at k = 5, the cross statistics with the realism mask."""
    seed = GAUSS_SEEDS[(n_real, n_fake, dim)]
    dt = np.float64 if f64 else np.float32
    real = features(n_real, dim + 8, seed, dtype=dt)
    fake = features(n_fake, dim + 8, seed + 1000, shift=0.15, dtype=dt)
    r, f = real[:, :dim], fake[:, :dim]
    d = direct_sq(r, f)
    rr, rf = radii_sq_of(direct_sq(r, r), GAUSS_K), radii_sq_of(direct_sq(f, f), GAUSS_K)
    conditions(r, f, d, rr, rf)
    mask = realism_mask(rr)
    count, hit, mn, rls = cross_ref(d, rr, rf, mask)
    for a in (real, fake, d, rr, rf, mask, count, hit, mn, rls):
        a.setflags(write=False)
    return dict(real=real, fake=fake, d=d, rr=rr, rf=rf, mask=mask, count=count, hit=hit, mn=mn, rls=rls)


# ---- The case whose workgroups WALK several column tiles: the column split of a launch is min(512 // bands, tiles), so a workgroup
# keeps its per-row lists, minima and hit counts across tiles only when tiles > 512 // bands -- 32 bands x 32 tiles here: 16 splits of
# 2 tiles (the production size, 10 000 x 10 000, has 6 splits of 13 - 14).  dim = 16 keeps the direct reference at a second or two.
WALK_N_REAL, WALK_N_FAKE, WALK_DIM, WALK_SEED = 3990, 4001, 16, 301


@functools.lru_cache(maxsize=None)
def walk_case():
    """As gauss_case (fp32, ld = dim + 8, k = 5).  The fake radii come from the expanded form (a BLAS product): in the cross test radii are
    INPUTS handed to the kernel, and the decision gap is asserted against exactly these numbers; the real radii are the direct ones and
    are also what the radii test checks."""
    dim = WALK_DIM
    real = features(WALK_N_REAL, dim + 8, WALK_SEED)
    fake = features(WALK_N_FAKE, dim + 8, WALK_SEED + 1000, shift=0.15)
    r, f = real[:, :dim], fake[:, :dim]
    d = direct_sq(r, f)
    d_rr = direct_sq(r, r)
    rr = np.partition(d_rr, GAUSS_K, axis=1)[:, GAUSS_K]
    f64 = f.astype(np.float64)
    fn = (f64 * f64).sum(1)
    d_ff = np.maximum(fn[:, None] + fn[None, :] - 2.0 * (f64 @ f64.T), 0.0)
    np.fill_diagonal(d_ff, 0.0)
    rf = np.partition(d_ff, GAUSS_K, axis=1)[:, GAUSS_K]
    conditions(r, f, d, rr, rf)
    mask = realism_mask(rr)
    count, hit, mn, rls = cross_ref(d, rr, rf, mask)
    dmax_rr = float(d_rr.max())
    for a in (real, fake, rr, rf, mask, count, hit, mn, rls):
        a.setflags(write=False)
    return dict(real=real, fake=fake, dmax=float(d.max()), dmax_rr=dmax_rr, rr=rr, rf=rf, mask=mask, count=count, hit=hit, mn=mn, rls=rls)


def conditions(r, f, d, rr, rf):
    """What makes an exact comparison of counts against another summation order legitimate on these inputs:
      decision gap   every |d_ij - radius| that a comparison decides (coverage's row minimum included) is at least 1e-9 * radius, in the
                     distance domain -- six orders of magnitude above the rounding of an fp64 contraction of this length;
      separation     d2_ij >= 1e-2 * (|x_i|^2 + |y_j|^2): the expansion |x|^2 + |y|^2 - 2 x.y loses at most two digits to cancellation."""
    dist, r_r, r_f = np.sqrt(d), np.sqrt(rr), np.sqrt(rf)
    gap = min(float((np.abs(dist - r_r[:, None]) / r_r[:, None]).min()), float((np.abs(dist - r_f[None, :]) / r_f[None, :]).min()),
              float((np.abs(dist.min(1) - r_r) / r_r).min()))
    assert gap >= 1e-9, f'decision gap {gap:.2e}: replace the seed'
    sep = float((d / ((np.asarray(r, np.float64) ** 2).sum(1)[:, None] + (np.asarray(f, np.float64) ** 2).sum(1)[None, :])).min())
    assert sep >= 1e-2, f'separation {sep:.2e}: replace the seed'
    return gap, sep


# ---- Integer lattice: every squared distance is an exact integer in any summation order, so strict <, multiplicity and the zeroed
# diagonal are pinned by EXACT equality.
LATTICE_K = 5


@functools.lru_cache(maxsize=None)
def lattice_case():
    g = np.random.RandomState(7)
    real = g.randint(0, 3, size=(200, 6)).astype(np.float64)
    fake = g.randint(0, 3, size=(180, 6)).astype(np.float64)
    real[10:16] = real[10]                  # six identical real rows: five neighbours at distance 0 -> that radius is exactly 0
    real[150] = real[40]                    # duplicates within the real set, across two 128-row bands
    fake[5] = fake[6] = fake[140]           # ... within the fake set
    fake[0], fake[1], fake[170] = real[3], real[10], real[199]      # ... across the sets (fake[1] sits on the radius-0 rows)
    d = direct_sq(real, fake)
    d_rr, d_ff = direct_sq(real, real), direct_sq(fake, fake)
    for m in (d, d_rr, d_ff):
        assert np.array_equal(m, np.round(m))
    rr, rf = radii_sq_of(d_rr, LATTICE_K), radii_sq_of(d_ff, LATTICE_K)
    assert rr[10] == 0.0 and (rr > 0).sum() > 150
    mask = realism_mask(rr)
    count, hit, mn, rls = cross_ref(d, rr, rf, mask)
    assert np.isnan(rls[1]) and np.isinf(rls).any()                 # 0 / 0 and r / 0, as numpy gives them
    for a in (real, fake, rr, rf, mask, count, hit, mn, rls):
        a.setflags(write=False)
    return dict(real=real, fake=fake, rr=rr, rf=rf, mask=mask, count=count, hit=hit, mn=mn, rls=rls,
                metrics=metrics_ref(count, hit, mn, rr, LATTICE_K))
