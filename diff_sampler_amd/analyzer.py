"""Geometry of sampling trajectories (reference: diff-analyzer-main -- main_mp.ipynb, main_extend.ipynb, utils.cal_deviation).

Three things the notebooks do with a sampler's ``(inter_xt, inter_denoised, inter_eps)`` (``return_inters / return_denoised / return_eps`` of
``solvers``), each kept under the notebook's name where it has one:

``trajectory_stats``      main_mp.ipynb's per-(step, sample) statistics -- magnitude, deviation from the chord, distance to the end point, the
                          cosine between eps and ``x_t - x_0`` -- from the six inner products of ``gits_utils.trajectory_moments`` and the
                          row kernel ``dsm_row_sqdist``; ``trajectory_distance`` is the L2 distance between two trajectories.
``project_trajectories``  main_extend.ipynb's 3-D picture: per trajectory, the chord direction and the two leading principal components of
                          what is left of it.  The notebook QR-factorises a random (D - 1) x D matrix per trajectory to build a D x D
                          projector and runs a randomised ``pca_lowrank``; here the same coordinates come, exactly and deterministically,
                          from the T x T Gram matrix of the trajectory's points relative to its end (below), which ``dsm_traj_gram``
                          (csrc/metrics/traj.hip) forms on the fp64 matrix pipe reading the fp32 trajectory in place.
``align_trajectories``,   the rotation onto a base trajectory, the arc length and the local-fit curvature / torsion of the notebook's
``arc_length``,           "Calibrated Trajectories" and "Curvature and Torsion" cells: T x 3 work per trajectory, numpy fp64 on the host.
``cal_curv_tors``

The Gram form.  For one trajectory with rows x_0 .. x_{T-1} let Y_t = x_t - x_{T-1}, G = Y Y^T, g0 = G[:, 0], v = -Y_0 / |Y_0| the unit chord.
The notebook's projected, centred data is Z = H Y (I - v v^T) with H = I - 1/T, so Z Z^T = H M H =: K with M = G - g0 g0^T / G[0, 0].  With
K = W L W^T (descending) and s_k = sqrt(L_k), the k-th principal direction is Z^T w_k / s_k -- already orthogonal to v, so the notebook's
Gram-Schmidt step changes nothing -- and the coordinates of the points Y on (v, PC1, PC2) are
    xs = -g0 / sqrt(G[0, 0]),    ys = M H w_1 / s_1,    zs = M H w_2 / s_2
up to the notebook's sign rules (at row T // 2: xs < 0, ys > 0, zs > 0, then zs negated).  Everything after G is T x T, fp64, on the host.
M cancels the chord's energy out of G (PC1 and PC2 carry 1e-4 and 1e-6 of it on real trajectories): G has to be fp64.

CUDA tensors go through the kernels -- no fallback when a library is missing.  CPU tensors go through the same arithmetic in torch fp64,
so the host logic runs without a GPU.

Command line: ``python -m diff_sampler_amd.analyzer run --dataset_name=cifar10 --solver=euler --num_steps=21 --seeds=0-63 --outdir=DIR``
(the EDM networks, built as ``sample.py`` builds them) writes ``stat.npz`` -- the keys of ``trajectory_stats`` plus ``t_steps, xs, ys, zs, s,
curvatures, torsions`` -- and the first batch's ``inter_xt.npy / inter_denoised.npy / inter_eps.npy``.  No plotting.

Not here: the optimal (dataset) denoiser and the Gaussian / mixture-of-Gaussians score samplers of main_extend.ipynb, and with them the
notebook's ``diff_*`` statistics, which compare against optimal trajectories.
"""
from __future__ import annotations

import numpy as np
import torch

__all__ = ['trajectory_gram', 'project_from_gram', 'project_trajectories', 'drop_outliers', 'align_trajectories', 'arc_length',
           'cal_curv_tors', 'trajectory_stats', 'trajectory_distance']

_GRAM_BYTES = 1 << 30        # most bytes of `gram` (and of its workspace) one dsm_traj_gram call is given
_COS_EPS = 1e-8              # torch.nn.functional.cosine_similarity's clamp on each norm


def _rows(t, what='trajectory'):
    """[n, B, ...] -> contiguous fp32 [n, B, per]."""
    t = torch.as_tensor(t)
    if t.dim() < 3:
        raise ValueError(f'{what} must be [points, batch, ...], got {tuple(t.shape)}')
    return t.to(torch.float32).reshape(t.shape[0], t.shape[1], -1).contiguous()


# ------------------------------------------------------------------------------------------------------------------ Gram matrix
def _gram_host(x):
    y = x.to(torch.float64) - x[-1:].to(torch.float64)
    y = y.permute(1, 0, 2)
    return torch.bmm(y, y.transpose(1, 2))


def _gram_device(x):
    import ctypes as C
    from . import _lib, _metrics_lib
    lib = _metrics_lib.load()
    n, B, per = x.shape
    out = torch.empty(B, n, n, dtype=torch.float64, device=x.device)
    ws1 = lib.dsm_traj_gram_workspace_bytes(n, per, 1)
    if ws1 < 0:
        _metrics_lib.check(int(ws1), 'dsm_traj_gram_workspace_bytes')
    chunk = max(1, min(B, 65535, _GRAM_BYTES // max(n * n * 8, int(ws1), 1)))
    with torch.cuda.device(x.device):
        ws = torch.empty(max(int(ws1) * chunk, 8), dtype=torch.uint8, device=x.device)
        for b0 in range(0, B, chunk):
            nb = min(chunk, B - b0)
            _metrics_lib.check(lib.dsm_traj_gram(C.c_void_p(x.data_ptr()), n, B, per, b0, nb, C.c_void_p(out[b0].data_ptr()),
                                                 C.c_void_p(ws.data_ptr()), ws.numel(), _lib.stream_ptr()), 'dsm_traj_gram')
    return out


def trajectory_gram(traj):
    """[B, T, T] fp64: gram[b, t, s] = <x[t, b] - x[T-1, b], x[s, b] - x[T-1, b]> of a stacked trajectory [T, B, ...]."""
    x = _rows(traj)
    if x.shape[0] < 2:
        raise ValueError('a trajectory has at least two points')
    return _gram_device(x) if x.is_cuda else _gram_host(x)


# ------------------------------------------------------------------------------------------------------------------ 3-D projection
def project_from_gram(gram):
    """The host finalisation of ``project_trajectories``: [B, T, T] Gram matrices (torch or numpy, any device) -> dict(xs, ys, zs [T, B],
    singular_values [B, min(T, 8)]), numpy fp64.  A direction without energy (s_k = 0: T = 2, or a trajectory inside a plane through the
    chord) has coordinates 0."""
    G = torch.as_tensor(gram).detach().to('cpu', torch.float64)
    B, T, _ = G.shape
    g0 = G[:, :, 0]
    g00 = G[:, 0, 0]
    M = G - g0[:, :, None] * g0[:, None, :] / g00[:, None, None]
    H = torch.eye(T, dtype=torch.float64) - 1.0 / T
    K = H @ M @ H
    lam, W = torch.linalg.eigh(0.5 * (K + K.transpose(1, 2)))
    lam, W = lam.flip(1), W.flip(2)                                 # descending
    s = lam.clamp_min(0.0).sqrt()
    P = (M @ H) @ W[:, :, :2]                                       # [B, T, 2]
    s2 = s[:, None, :2]
    P = torch.where(s2 > 0, P / torch.where(s2 > 0, s2, torch.ones_like(s2)), torch.zeros_like(P))
    xs = -g0 / g00.sqrt()[:, None]
    ys, zs = P[:, :, 0], P[:, :, 1]
    mid = T // 2
    xs = torch.where((xs[:, mid] < 0)[:, None], xs, -xs)           # u1 kept where <y_mid, u1> < 0
    ys = torch.where((ys[:, mid] > 0)[:, None], ys, -ys)
    zs = -torch.where((zs[:, mid] > 0)[:, None], zs, -zs)          # ... and the cell's final u3 *= -1
    return dict(xs=xs.T.contiguous().numpy(), ys=ys.T.contiguous().numpy(), zs=zs.T.contiguous().numpy(),
                singular_values=s[:, :min(T, 8)].contiguous().numpy())


def project_trajectories(traj):
    """Coordinates of every trajectory point (relative to the trajectory's end) on the chord direction and on the two leading principal
    components of the rest: dict(xs, ys, zs [T, B] fp64 numpy, singular_values [B, min(T, 8)])."""
    return project_from_gram(trajectory_gram(traj))


def drop_outliers(xs, ys, zs, ratio_to_keep=0.8):
    """The notebook's outlier rule: order the trajectories by sum_t ys^2 + 10 zs^2 and keep the middle ``ratio_to_keep`` of them.
    Returns (xs, ys, zs, kept indices)."""
    xs, ys, zs = (np.asarray(a, dtype=np.float64) for a in (xs, ys, zs))
    B = xs.shape[1]
    order = np.argsort((ys ** 2 + 10 * zs ** 2).sum(axis=0), kind='stable')
    keep_n = int(B * ratio_to_keep)
    start = (B - keep_n) // 2
    keep = order[start:start + keep_n]
    return xs[:, keep], ys[:, keep], zs[:, keep], keep


def align_trajectories(xs, ys, zs, base_idx=0, proj_dim=2):
    """Rotate every projected trajectory onto trajectory ``base_idx``: the orthogonal O that minimises |A O - B|_F (A, B the [T, dim] point
    lists), O = U V^T from the SVD of A^T B -- of the (ys, zs) columns for proj_dim = 2 (xs is kept), of all three for proj_dim = 3.
    (The notebook multiplies U by the transpose of numpy's already transposed factor; that is the minimiser only where A^T B is symmetric.)
    Returns dict(xs, ys, zs [T, B], rotations [B, proj_dim, proj_dim])."""
    if proj_dim not in (2, 3):
        raise ValueError('proj_dim is 2 or 3')
    pts = np.stack([np.asarray(a, dtype=np.float64) for a in (xs, ys, zs)], axis=2).transpose(1, 0, 2)     # [B, T, 3]
    A = pts[:, :, 3 - proj_dim:]
    U, _, Vh = np.linalg.svd(A.transpose(0, 2, 1) @ A[base_idx][None])
    O = U @ Vh
    out = pts.copy()
    out[:, :, 3 - proj_dim:] = A @ O
    return dict(xs=out[:, :, 0].T.copy(), ys=out[:, :, 1].T.copy(), zs=out[:, :, 2].T.copy(), rotations=O)


def arc_length(xs, ys, zs):
    """[T, B]: cumulative length of the polygon through the projected points (0 at the first)."""
    p = np.stack([np.asarray(a, dtype=np.float64) for a in (xs, ys, zs)], axis=1)                          # [T, 3, B]
    seg = np.linalg.norm(p[1:] - p[:-1], axis=1)
    return np.cumsum(np.concatenate((np.zeros((1, seg.shape[1])), seg), axis=0), axis=0)


def cal_curv_tors(xs, ys, zs, s, window_size):
    """Curvature and torsion [T, B] of the projected curves from a local cubic fit r(s + h) - r(s) = r' h + r'' h^2 / 2 + r''' h^3 / 6 by
    least squares over a window of ``window_size`` (odd) neighbouring points in arc length; near the ends the window is filled with the
    points the notebook fills it with.  curvature = |r' x r''| / |r'|^3, torsion = (r' x r'') . r''' / |r' x r''|^2."""
    xs, ys, zs, s = (np.asarray(a, dtype=np.float64) for a in (xs, ys, zs, s))
    if window_size % 2 != 1 or window_size < 3 or xs.shape[0] < window_size:
        raise ValueError('window_size is odd, at least 3 and at most the number of points')
    h, T = window_size // 2, xs.shape[0]

    def padded(a):
        return np.concatenate([a[h + 1:2 * h + 1], a, a[-2 * h:-h]])

    sp, cp = padded(s), [padded(c) for c in (xs, ys, zs)]
    a = np.zeros((6,) + xs.shape)                                   # sums of h^2, h^3/2, h^4/4, h^4/6, h^5/12, h^6/36
    b = np.zeros((3, 3) + xs.shape)                                 # [power - 1][coordinate]
    for i in range(window_size):
        d = sp[i:i + T] - s
        a[0] += d ** 2
        a[1] += d ** 3 / 2
        a[2] += d ** 4 / 4
        a[3] += d ** 4 / 6
        a[4] += d ** 5 / 12
        a[5] += d ** 6 / 36
        for c in range(3):
            dc = cp[c][i:i + T] - cp[c][h:h + T]
            b[0, c] += d * dc
            b[1, c] += d ** 2 * dc / 2
            b[2, c] += d ** 3 * dc / 6
    A = np.array([[a[0], a[1], a[3]], [a[1], a[2], a[4]], [a[3], a[4], a[5]]]).transpose(2, 3, 0, 1)       # [T, B, 3, 3]
    X = np.matmul(np.linalg.inv(A), b.transpose(2, 3, 0, 1))       # [T, B, derivative, coordinate]
    r1, r2, r3 = X[:, :, 0], X[:, :, 1], X[:, :, 2]
    cr = np.cross(r1, r2)
    curvatures = np.linalg.norm(cr, axis=2) / np.linalg.norm(r1, axis=2) ** 3
    torsions = np.sum(cr * r3, axis=2) / np.linalg.norm(cr, axis=2) ** 2
    return curvatures, torsions


# ------------------------------------------------------------------------------------------------------------------ per-(step, sample) statistics
def _row_sq(a, b=None):
    """[n, B] fp64 numpy: sum_e (a - b)^2 (b None: sum a^2) of [n, B, per] fp32 rows."""
    n, B, per = a.shape
    if not a.is_cuda:
        d = a.to(torch.float64) if b is None else a.to(torch.float64) - b.to(torch.float64)
        return (d * d).sum(2).numpy()
    import ctypes as C
    from . import _lib, _metrics_lib
    lib = _metrics_lib.load()
    out = torch.empty(n, B, dtype=torch.float64, device=a.device)
    with torch.cuda.device(a.device):
        _metrics_lib.check(lib.dsm_row_sqdist(C.c_void_p(a.data_ptr()), None if b is None else C.c_void_p(b.data_ptr()), n * B, per,
                                              C.c_void_p(out.data_ptr()), _lib.stream_ptr()), 'dsm_row_sqdist')
    return out.cpu().numpy()


def _moments(x, eps=None):
    """[n, B, 6] fp64 numpy {P, Q, R, S, T, N} of csrc/gits.hip: c = x[-1], bc = c - x[0]; P = (c - x_i).bc, Q = d_i.bc, R = |c - x_i|^2,
    S = (c - x_i).d_i, T = |d_i|^2, N = |bc|^2, the eps terms 0 for the last point."""
    if x.is_cuda:
        from . import gits_utils
        return gits_utils.trajectory_moments(x, eps)
    x = x.to(torch.float64)
    cx = x[-1:] - x
    bc = (x[-1] - x[0])[None]
    d = torch.zeros_like(x)
    if eps is not None:
        d[:-1] = eps.to(torch.float64)
    m = torch.stack([(cx * bc).sum(2), (d * bc).sum(2), (cx * cx).sum(2), (cx * d).sum(2), (d * d).sum(2),
                     (bc * bc).sum(2).expand(x.shape[0], -1)], dim=2)
    return m.numpy()


def _chord_stats(m):
    """(distance to the end point [n, B], deviation of the interior points from the start -> end chord [n - 2, B])."""
    P, R, N = m[:, :, 0], m[:, :, 2], m[:, :, 5]
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.sqrt(R), np.sqrt(np.maximum(R - P * P / N, 0.0))[1:-1]


def trajectory_stats(inter_xt, inter_denoised=None, inter_eps=None):
    """main_mp.ipynb's statistics as a dict of [steps, batch] fp64 numpy arrays (the notebook's shapes):
      mag_xt [n], mag_denoised [nd], mag_eps [n - 1]      L2 norms
      dist_xt [n], dist_denoised [nd]                       L2 distance to the last point of the own trajectory
      dev_xt [n - 2], dev_denoised [nd - 2]                 distance of the interior points from the first -> last chord (utils.cal_deviation)
      cos_xt [n - 1]                                        cosine between eps_i and x_i - x_last (each norm clamped at 1e-8)
    The keys of an input that is not given are left out.  inter_eps has one row less than inter_xt."""
    x = _rows(inter_xt, 'inter_xt')
    n = x.shape[0]
    if n < 2:
        raise ValueError('a trajectory has at least two points')
    e = None
    if inter_eps is not None:
        e = _rows(inter_eps, 'inter_eps')
        if e.shape[0] != n - 1 or e.shape[1:] != x.shape[1:]:
            raise ValueError(f'inter_eps must be [{n - 1}, batch, ...] next to an inter_xt of {n} points, got {tuple(e.shape)}')
    out = {}
    m = _moments(x, e)
    out['mag_xt'] = np.sqrt(_row_sq(x))
    out['dist_xt'], out['dev_xt'] = _chord_stats(m)
    if inter_denoised is not None:
        dn = _rows(inter_denoised, 'inter_denoised')
        if dn.shape[0] < 2:
            raise ValueError('inter_denoised has at least two points')
        out['mag_denoised'] = np.sqrt(_row_sq(dn))
        out['dist_denoised'], out['dev_denoised'] = _chord_stats(_moments(dn))
    if e is not None:
        out['mag_eps'] = np.sqrt(_row_sq(e))
        R, S, T = m[:-1, :, 2], m[:-1, :, 3], m[:-1, :, 4]
        out['cos_xt'] = -S / (np.maximum(np.sqrt(T), _COS_EPS) * np.maximum(np.sqrt(R), _COS_EPS))
    return out


def trajectory_distance(a, b):
    """[steps, batch] fp64 numpy: the L2 distance between the points of two trajectories of one shape."""
    a, b = _rows(a, 'a'), _rows(b, 'b')
    if a.shape != b.shape or a.device != b.device:
        raise ValueError(f'two trajectories of one shape on one device, got {tuple(a.shape)} and {tuple(b.shape)}')
    return np.sqrt(_row_sq(a, b))


# ------------------------------------------------------------------------------------------------------------------ command line
def run(dataset_name, solver='euler', num_steps=21, seeds='0-63', outdir='./analysis', max_batch_size=64, model_path=None, random_init=False,
        device=None, window_size=None, schedule_type='polynomial', schedule_rho=7, max_order=None, afs=False, use_fp16=False):
    """Sample ``seeds`` with the trajectory, the denoised outputs and eps captured, and write ``outdir/stat.npz`` (module docstring)."""
    import os
    from . import sample, solvers, solver_utils
    seeds = sample.parse_int_list(seeds)
    device = torch.device('cuda') if device is None else torch.device(device)
    net, source = sample.create_model(dataset_name, model_path, random_init, device, use_fp16=use_fp16)
    if source != 'edm':
        raise ValueError('the analyzer samples the EDM networks')
    t_steps = solver_utils.get_schedule(num_steps, net.sigma_min, net.sigma_max, device=device, schedule_type=schedule_type,
                                        schedule_rho=schedule_rho, net=net)
    if max_order is None:
        max_order = 3 if solver == 'dpmpp' else 4
    kw = dict(num_steps=num_steps, sigma_min=net.sigma_min, sigma_max=net.sigma_max, schedule_type=schedule_type, schedule_rho=schedule_rho,
              afs=afs, denoise_to_zero=False, return_inters=True, return_denoised=True, return_eps=True, t_steps=t_steps, max_order=max_order)
    if solver not in sample.SOLVER_FNS or solver == 'unipc':
        raise ValueError(f'solver {solver!r}: one of euler, heun, dpm, ipndm, ipndm_v, deis, dpmpp')
    if solver == 'deis':
        kw['coeff_list'] = solver_utils.get_deis_coeff_list(t_steps, max_order, deis_mode='tab')
    sampler_fn = getattr(solvers, sample.SOLVER_FNS[solver])
    os.makedirs(outdir, exist_ok=True)
    parts = []
    for i in range(0, len(seeds), max_batch_size):
        batch_seeds = seeds[i:i + max_batch_size]
        B = len(batch_seeds)
        rnd = sample.StackedRandomGenerator(device, batch_seeds)
        latents = rnd.randn([B, net.img_channels, net.img_resolution, net.img_resolution], device=device)
        labels = None
        if net.label_dim:
            labels = torch.eye(net.label_dim, device=device)[rnd.randint(net.label_dim, size=[B], device=device)]
        inter_xt, inter_denoised, inter_eps = sampler_fn(net, latents, class_labels=labels, **kw)
        st = trajectory_stats(inter_xt, inter_denoised, inter_eps)
        st.update({k: v for k, v in project_trajectories(inter_xt).items() if k != 'singular_values'})
        parts.append(st)
        if i == 0:
            for name, t in (('inter_xt', inter_xt), ('inter_denoised', inter_denoised), ('inter_eps', inter_eps)):
                np.save(os.path.join(outdir, name + '.npy'), t.cpu().numpy())
    stat = {k: np.concatenate([p[k] for p in parts], axis=1) for k in parts[0]}
    stat['t_steps'] = solver_utils.host_times(t_steps)
    stat['s'] = arc_length(stat['xs'], stat['ys'], stat['zs'])
    n = stat['xs'].shape[0]
    if window_size is None:
        window_size = min(101, n - 1 + n % 2)                       # the notebook's 101 on its 1001 points; the largest odd size on fewer
    stat['curvatures'], stat['torsions'] = cal_curv_tors(stat['xs'], stat['ys'], stat['zs'], stat['s'], window_size)
    path = os.path.join(outdir, 'stat.npz')
    np.savez(path, **stat)
    print(f'Wrote {path}: ' + ', '.join(f'{k}{list(np.shape(v))}' for k, v in stat.items()))
    return path


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog='python -m diff_sampler_amd.analyzer')
    sub = ap.add_subparsers(dest='cmd', required=True)
    r = sub.add_parser('run', help='sample with captured trajectories and write stat.npz')
    r.add_argument('--dataset_name', required=True)
    r.add_argument('--solver', default='euler')
    r.add_argument('--num_steps', type=int, default=21)
    r.add_argument('--seeds', default='0-63')
    r.add_argument('--outdir', default='./analysis')
    r.add_argument('--batch', dest='max_batch_size', type=int, default=64)
    r.add_argument('--model_path', default=None)
    r.add_argument('--random_init', type=lambda v: str(v).lower() in ('1', 'true', 'yes'), default=False)
    r.add_argument('--window_size', type=int, default=None)
    r.add_argument('--schedule_type', default='polynomial')
    r.add_argument('--schedule_rho', type=float, default=7)
    r.add_argument('--max_order', type=int, default=None)
    r.add_argument('--afs', type=lambda v: str(v).lower() in ('1', 'true', 'yes'), default=False)
    r.add_argument('--use_fp16', type=lambda v: str(v).lower() in ('1', 'true', 'yes'), default=False)
    a = vars(ap.parse_args(argv))
    a.pop('cmd')
    run(**a)


if __name__ == '__main__':
    main()
