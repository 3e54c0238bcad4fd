"""Inputs and the independent reference of the trajectory-analysis tests (test_analyzer_cpu.py, test_hip_analyzer.py).

``project_direct`` is a DIRECT fp64 restatement of the projection cell of the reference's main_extend.ipynb ("Regularity of Sampling
Trajectories") with exact linear algebra: per trajectory it applies the projector I - v v^T (v the unit chord) to the D-dimensional points,
centres them, takes an exact ``torch.linalg.svd``, orthogonalises (chord, PC1, PC2) by Gram-Schmidt, applies the cell's flip rules at row
T // 2 (with its final negation of the third axis) and reads the coordinates of the points relative to the trajectory's end.  It stands in
for the notebook's route -- a QR factorisation of a random (D - 1) x D matrix for the projector and a randomised ``pca_lowrank`` -- which
only approximates this and depends on the random state.  Nothing here touches a Gram matrix.

References are computed once per case (lru_cache) and never modified by a test."""
import functools

import numpy as np
import torch


def random_walk(seed, shape, scale=3.0):
    """scale * cumsum(randn(shape)) along the trajectory axis, fp32."""
    g = torch.Generator().manual_seed(seed)
    return scale * torch.cumsum(torch.randn(shape, generator=g), dim=0)


def project_direct(traj):
    """traj [T, B, ...] -> dict(xs, ys, zs [T, B], singular_values [B, min(T, 8)]) numpy fp64."""
    x = torch.as_tensor(traj).to(torch.float64)
    T, B = x.shape[0], x.shape[1]
    x = x.reshape(T, B, -1)
    D = x.shape[2]
    cols = []
    sv = []
    for b in range(B):
        data = x[:, b]
        end = data[-1]
        v = end - data[0]
        v = v / v.norm()
        proj = data @ (torch.eye(D, dtype=torch.float64) - torch.outer(v, v))
        proj = proj - proj.mean(0, keepdim=True)
        _, S, Vh = torch.linalg.svd(proj, full_matrices=False)
        u1, v2, v3 = v, Vh[0], Vh[1]
        u2 = v2 - (u1 @ v2) / (u1 @ u1) * u1
        u3 = v3 - (u1 @ v3) / (u1 @ u1) * u1 - (u2 @ v3) / (u2 @ u2) * u2
        u2, u3 = u2 / u2.norm(), u3 / u3.norm()
        rel = data - end
        probe = rel[T // 2]
        u1 = u1 if probe @ u1 < 0 else -u1
        u2 = u2 if probe @ u2 > 0 else -u2
        u3 = u3 if probe @ u3 > 0 else -u3
        u3 = -u3
        cols.append(torch.stack([rel @ u1, rel @ u2, rel @ u3]))
        sv.append(S[:min(T, 8)])
    c = torch.stack(cols).numpy()                                   # [B, 3, T]
    return dict(xs=c[:, 0].T.copy(), ys=c[:, 1].T.copy(), zs=c[:, 2].T.copy(), singular_values=torch.stack(sv).numpy())


# ---- projection cases: name -> (seed, shape).  A seed that fails `conditions` is REPLACED here, never skipped.
PROJECTION_CASES = {
    'walk9': (0, (9, 5, 3, 4, 4)),          # per = 48; smallest ratio 1.116
    'walk5': (3, (5, 3, 1, 5, 7)),          # per = 35: no multiple of the kernel's 16-feature chunk; T // 2 = 2
    'walk20': (5, (20, 2, 3, 8, 8)),        # even T, per = 192 (seeds 0 - 4 have a gap below 1.1)
}
MIN_GAP = 1.1            # s1 / s2 and s2 / s3: the eigenvectors of the Gram form are conditioned by these gaps
MIN_PROBE = 1e-6         # |coordinate at row T // 2| / max |coordinate|: the flip rules decide on that sign


@functools.lru_cache(maxsize=None)
def projection_case(name):
    seed, shape = PROJECTION_CASES[name]
    traj = random_walk(seed, shape)
    ref = project_direct(traj)
    for a in ref.values():
        a.setflags(write=False)
    return traj, ref


def conditions(name):
    """(smallest singular-value ratio, smallest relative probe coordinate) of a case; both must clear MIN_GAP / MIN_PROBE."""
    traj, ref = projection_case(name)
    s = ref['singular_values']
    gap = float(min((s[:, 0] / s[:, 1]).min(), (s[:, 1] / s[:, 2]).min()))
    mid = traj.shape[0] // 2
    probe = min(float((np.abs(ref[k][mid]) / np.abs(ref[k]).max(axis=0)).min()) for k in ('xs', 'ys', 'zs'))
    return gap, probe


# ---- Gram-kernel inputs
def lattice(seed, shape, lim=512):
    """Integers in [-lim, lim] as fp32: every difference, product and partial sum of the Gram matrix is an exact double."""
    return np.random.RandomState(seed).randint(-lim, lim + 1, size=shape).astype(np.float32)


def gram_int(x):
    """[B, T, T] int64 Gram of an integer-valued trajectory [T, B, per] relative to its last point."""
    y = x.astype(np.int64) - x[-1:].astype(np.int64)
    return np.einsum('tbe,sbe->bts', y, y)


def gram_f64(x):
    """(gram, abs_gram): numpy fp64 Gram [B, T, T] and sum_e |y_te y_se|, the scale of the summation-order bound."""
    y = x.astype(np.float64) - x[-1:].astype(np.float64)
    y = np.ascontiguousarray(y.transpose(1, 0, 2))
    a = np.abs(y)
    return y @ y.transpose(0, 2, 1), a @ a.transpose(0, 2, 1)
