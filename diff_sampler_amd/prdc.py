"""Precision, recall, density, coverage and per-sample realism of a generated image set against a reference set.

Reference: sfd-main/prdc.py.  ``compute_prdc`` there builds three full distance matrices on the CPU
(``sklearn.metrics.pairwise_distances``: real x real, fake x fake, real x fake; prdc.py:85-87), takes the (k + 1)-th smallest value of
each row of the two square ones as that sample's radius (prdc.py:44-68) and compares the third against the radii (prdc.py:89-107).
The function names and results of prdc.py:29-125,222-248 are kept: ``compute_pairwise_distance``, ``get_kth_value``,
``compute_nearest_neighbour_distances``, ``compute_prdc``, ``compute_scores``; inputs may be numpy arrays or torch tensors.

On the GPU (CUDA tensors, or ``device='cuda'``) the metric is three passes of csrc/metrics/prdc.hip through libdsmetrics.so, one per
distance matrix: ``dsm_knn_radii_sq`` on each set and ``dsm_prdc_cross`` on the pair -- fp64 MFMA distance tiles whose k-smallest
selection and threshold counts run on the accumulators, so no n x n matrix exists anywhere.  There is no fallback when the library is
missing.  On the CPU (the gloo tests, the CLI without a GPU) it is the same arithmetic in torch fp64, in row blocks.  Both compare
SQUARED distances with squared radii -- ``sqrt(a) < sqrt(b)`` and ``a < b`` differ only where a and b are adjacent doubles, below what
the summation order of the dot products already moves -- and take square roots of outputs only (radii, realism).  The finalisation keeps
the reference's expression order (density is ``(1. / float(k)) * mean``: ``mean / k`` differs by one ulp).

``compute_pairwise_distance`` returns a full matrix and is kept for API parity only: it is host-side torch fp64 and the metric path does
not use it.

Command line: ``python -m diff_sampler_amd.prdc calc --images DIR --images_ref DIR --detector SPEC [--num N] [--seed S] [--batch B]
[--nearest_k 5] [--device D]`` with the detector injected as in ``fid.py`` (``fid.load_detector``).  Differences from the reference's
``calc`` (prdc.py:261-316), all three of them defects there:
  * the reference fills the first 5 000 rows of an ``np.empty((10000, dims))`` and scores all 10 000 (prdc.py:184-190); here the features
    of exactly the images found -- or ``--num`` of them under the dataset's subset rule (``fid.ImageFolder``) -- are scored;
  * the reference asserts exactly 5 000 generated images (prdc.py:284); here any count above ``nearest_k`` works;
  * the reference shards the batches over ranks but never gathers the features, so every rank scores its own shard (prdc.py:304-314);
    here the shards are combined and rank 0 computes and prints the numbers.
"""
from __future__ import annotations

import numpy as np
import torch

_BLOCK = 1024            # rows per block of the host path: [1024][n] fp64 at n = 10 000 is 80 MB


def _features(a, device=None):
    """numpy / torch [n, dim] -> contiguous torch tensor, fp32 or fp64 (narrower floats widen exactly to fp32), on ``device`` if given."""
    if isinstance(a, np.ndarray):
        a = np.ascontiguousarray(a)
        t = torch.from_numpy(a if a.flags.writeable else a.copy())      # torch refuses to alias a read-only array quietly
    else:
        t = torch.as_tensor(a)
    if t.dim() != 2:
        raise ValueError(f'features must be [n, dim], got {tuple(t.shape)}')
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float32 if t.dtype in (torch.float16, torch.bfloat16) else torch.float64)
    if device is not None:
        t = t.to(device)
    return t.contiguous()


def _target(device, *inputs):
    """The device that computes: ``device`` if given, else that of the first CUDA tensor among the inputs, else the CPU."""
    if device is not None:
        return torch.device(device)
    for t in inputs:
        if torch.is_tensor(t) and t.is_cuda:
            return t.device
    return torch.device('cpu')


def _sq_dists(x, xn, y, yn):
    """sklearn's euclidean_distances before the square root: max(|x|^2 + |y|^2 - 2 x.y, 0), fp64."""
    d = x @ y.T
    d *= -2.0
    d += xn[:, None]
    d += yn[None, :]
    return d.clamp_(min=0.0)


def _sq_norms(x):
    return (x * x).sum(1)


def _sqrt(t):
    """Square roots of an OUTPUT, on the host in numpy (correctly rounded, as the reference's are; torch's vectorised fp64 sqrt is
    not: sqrt(2.0) comes out one ulp low)."""
    with np.errstate(invalid='ignore'):
        return np.sqrt(t.cpu().numpy())


# ------------------------------------------------------------------------------------------------------------------ squared-domain cores
def _knn_radii_sq_host(x, k):
    x = x.to(torch.float64)
    n = x.shape[0]
    xn = _sq_norms(x)
    out = torch.empty(n, dtype=torch.float64)
    for a in range(0, n, _BLOCK):
        b = min(a + _BLOCK, n)
        d = _sq_dists(x[a:b], xn[a:b], x, xn)
        d[torch.arange(b - a), torch.arange(a, b)] = 0.0                         # the zeroed diagonal of a self-distance matrix
        out[a:b] = torch.topk(d, k + 1, dim=1, largest=False).values[:, k]
    return out


def _cross_host(real, fake, rr, rf, mask):
    real, fake = real.to(torch.float64), fake.to(torch.float64)
    nr, nf = real.shape[0], fake.shape[0]
    rn, fn = _sq_norms(real), _sq_norms(fake)
    count = torch.zeros(nf, dtype=torch.int64)
    hit = torch.empty(nr, dtype=torch.int64)
    mn = torch.empty(nr, dtype=torch.float64)
    rls = torch.full((nf,), -np.inf, dtype=torch.float64) if mask is not None else None
    for a in range(0, nr, _BLOCK):
        b = min(a + _BLOCK, nr)
        d = _sq_dists(real[a:b], rn[a:b], fake, fn)
        count += (d < rr[a:b, None]).sum(0)
        hit[a:b] = (d < rf[None, :]).sum(1)
        mn[a:b] = d.min(1).values
        if mask is not None and bool(mask[a:b].any()):
            m = mask[a:b]
            rls = torch.maximum(rls, (rr[a:b][m][:, None] / d[m]).max(0).values)
    return count, hit, mn, rls


def _workspace(lib, n_real, n_fake, k, device):
    nbytes = lib.dsm_prdc_workspace_bytes(n_real, n_fake, k)
    if nbytes < 0:
        from . import _metrics_lib
        _metrics_lib.check(int(nbytes), 'dsm_prdc_workspace_bytes')
    return torch.empty(max(int(nbytes), 8), dtype=torch.uint8, device=device)


def _knn_radii_sq_device(x, k, ws=None):
    import ctypes as C
    from . import _lib, _metrics_lib
    lib = _metrics_lib.load()
    n, dim = x.shape
    with torch.cuda.device(x.device):
        ws = _workspace(lib, n, n, k, x.device) if ws is None else ws
        out = torch.empty(n, dtype=torch.float64, device=x.device)
        _metrics_lib.check(lib.dsm_knn_radii_sq(C.c_void_p(x.data_ptr()), int(x.dtype == torch.float64), max(x.stride(0), dim), n, dim, k,
                                                C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(), _lib.stream_ptr()),
                           'dsm_knn_radii_sq')
    return out


def _cross_device(real, fake, rr, rf, mask, ws=None):
    import ctypes as C
    from . import _lib, _metrics_lib
    lib = _metrics_lib.load()
    (nr, dim), nf = real.shape, fake.shape[0]
    dev = real.device
    with torch.cuda.device(dev):
        ws = _workspace(lib, nr, nf, 1, dev) if ws is None else ws
        count = torch.empty(nf, dtype=torch.int32, device=dev)
        hit = torch.empty(nr, dtype=torch.int32, device=dev)
        mn = torch.empty(nr, dtype=torch.float64, device=dev)
        rls = torch.empty(nf, dtype=torch.float64, device=dev) if mask is not None else None
        m8 = mask.to(device=dev, dtype=torch.uint8).contiguous() if mask is not None else None
        _metrics_lib.check(lib.dsm_prdc_cross(
            C.c_void_p(real.data_ptr()), int(real.dtype == torch.float64), max(real.stride(0), dim), nr,
            C.c_void_p(fake.data_ptr()), int(fake.dtype == torch.float64), max(fake.stride(0), dim), nf, dim,
            C.c_void_p(rr.data_ptr()), C.c_void_p(rf.data_ptr()), C.c_void_p(count.data_ptr()), C.c_void_p(hit.data_ptr()),
            C.c_void_p(mn.data_ptr()), C.c_void_p(m8.data_ptr()) if m8 is not None else None,
            C.c_void_p(rls.data_ptr()) if rls is not None else None, C.c_void_p(ws.data_ptr()), ws.numel(), _lib.stream_ptr()), 'dsm_prdc_cross')
    return count, hit, mn, rls


# ------------------------------------------------------------------------------------------------------------------ the reference's surface
def compute_pairwise_distance(data_x, data_y=None):
    """prdc.py:29-41: the full [n_x, n_y] matrix of Euclidean distances, fp64 numpy, diagonal exactly 0 when ``data_y`` is None.
    Host-only (API parity): the metrics never form this matrix."""
    x = _features(data_x, 'cpu').to(torch.float64)
    y = x if data_y is None else _features(data_y, 'cpu').to(torch.float64)
    d = _sq_dists(x, _sq_norms(x), y, _sq_norms(y))
    if data_y is None:
        d.fill_diagonal_(0.0)
    return _sqrt(d)


def get_kth_value(unsorted, k, axis=-1):
    """prdc.py:44-55: the k-th smallest value along ``axis`` (numpy in, numpy out; torch in, torch out)."""
    if torch.is_tensor(unsorted):
        return torch.topk(unsorted, k, dim=axis, largest=False).values.max(dim=axis).values
    a = np.asarray(unsorted)
    return np.take(np.partition(a, k - 1, axis=axis), k - 1, axis=axis)


def compute_nearest_neighbour_distances(input_features, nearest_k, device=None):
    """prdc.py:58-68: distance of every sample to its ``nearest_k``-th nearest neighbour within the set (the sample itself is the
    0-th).  numpy in -> numpy fp64 out; torch in -> torch fp64 on the computing device."""
    x = _features(input_features, _target(device, input_features))
    _check_k(x.shape[0], nearest_k)
    r = _sqrt(_knn_radii_sq_device(x, nearest_k) if x.is_cuda else _knn_radii_sq_host(x, nearest_k))
    return torch.from_numpy(r).to(x.device) if torch.is_tensor(input_features) else r


def _check_k(n, k):
    if int(k) != k or k < 1:
        raise ValueError(f'nearest_k must be a positive integer, got {k!r}')
    if k + 1 > n:
        raise ValueError(f'nearest_k = {k} needs at least {k + 1} samples, got {n}')


def compute_prdc(real_features, fake_features, nearest_k, realism=False, device=None):
    """prdc.py:71-125 -> dict(precision, recall, density, coverage[, realism]) of numpy fp64 scalars (realism: one value per fake sample)."""
    target = _target(device, real_features, fake_features)
    real, fake = _features(real_features, target), _features(fake_features, target)
    dev = real.is_cuda
    if real.shape[1] != fake.shape[1]:
        raise ValueError(f'feature dimensions differ: {real.shape[1]} and {fake.shape[1]}')
    k = int(nearest_k)
    _check_k(real.shape[0], nearest_k)
    _check_k(fake.shape[0], nearest_k)
    if dev:
        from . import _metrics_lib
        with torch.cuda.device(real.device):
            ws = _workspace(_metrics_lib.load(), real.shape[0], fake.shape[0], k, real.device)
        rr, rf = _knn_radii_sq_device(real, k, ws), _knn_radii_sq_device(fake, k, ws)
    else:
        rr, rf = _knn_radii_sq_host(real, k), _knn_radii_sq_host(fake, k)
    mask = None
    if realism:                                                  # prdc.py:119: the half of the real spheres with the smaller radii
        radii = _sqrt(rr)
        mask = torch.from_numpy(radii < np.median(radii))
    count, hit, mn, rls = _cross_device(real, fake, rr, rf, mask, ws) if dev else _cross_host(real, fake, rr, rf, mask)
    count, hit = count.cpu().numpy().astype(np.int64), hit.cpu().numpy()
    precision = (count > 0).mean()
    recall = (hit > 0).mean()
    density = (1. / float(k)) * count.mean()
    coverage = (mn < rr).cpu().numpy().mean()
    d = dict(precision=precision, recall=recall, density=density, coverage=coverage)
    if realism:
        d['realism'] = _sqrt(rls)
    return d


def compute_scores(metrics, reps, labels=None, nearest_k=5, device=None, log=print):
    """prdc.py:222-248: at most 10 000 samples per set (the real set always subsampled at random, the fake set only when realism is not
    asked for, so that realism stays aligned with the file names), ``key: value`` lines for the scalar metrics."""
    scores = {}
    if 'prdc' in metrics:
        log('Computing precision, recall, density, and coverage')
        reduced_n = min(10000, reps[0].shape[0], reps[1].shape[0])
        inds0 = np.random.choice(reps[0].shape[0], reduced_n, replace=False)
        inds1 = np.arange(reps[1].shape[0])
        if 'realism' not in metrics:
            inds1 = np.random.choice(inds1, min(inds1.shape[0], reduced_n), replace=False)
        scores = dict(scores, **compute_prdc(reps[0][inds0], reps[1][inds1], nearest_k=nearest_k, realism='realism' in metrics, device=device))
    for key, value in scores.items():
        if key == 'realism':
            continue
        log(f'{key}: {value:.5f}')
    return scores


# ------------------------------------------------------------------------------------------------------------------ command line
def extract_features(image_path, detector, num_expected=None, seed=0, max_batch_size=250, device='cuda', log=print):
    """Detector features of an image folder, [n, dim] on ``device``: the batches are sharded over the ranks of the process group
    (``fid.shard_items``), every rank extracts its shard, and the shards are all-gathered (padded to the largest; every rank knows every
    shard's rows from the sharding rule) and put back into image order."""
    import torch.distributed as dist
    from . import fid
    ds = fid.ImageFolder(image_path, max_size=num_expected, random_seed=seed)
    if num_expected is not None and len(ds) < num_expected:
        raise ValueError(f'Found {len(ds)} images, but expected at least {num_expected}')
    log(f'Computing representations of {len(ds)} images from "{image_path}"...')
    rank, world = (dist.get_rank(), dist.get_world_size()) if (dist.is_available() and dist.is_initialized()) else (0, 1)
    feats = []
    for idx in fid.shard_items(len(ds), max_batch_size, rank, world):
        if len(idx) == 0:
            continue
        images = ds[idx].to(device)
        if images.shape[1] == 1:
            images = images.repeat([1, 3, 1, 1])
        with torch.no_grad():
            f = detector(images)
        feats.append(f.to(torch.float32) if f.dtype not in (torch.float32, torch.float64) else f)
    rows = [torch.cat([i for i in fid.shard_items(len(ds), max_batch_size, r, world)] or [torch.zeros(0, dtype=torch.int64)]) for r in range(world)]
    meta = torch.tensor([feats[0].shape[1] if feats else 0, int(feats[0].dtype == torch.float64) if feats else 0], dtype=torch.int64, device=device)
    if world > 1:
        dist.all_reduce(meta, op=dist.ReduceOp.MAX)              # a rank without images learns the feature width and type
    dim, dtype = int(meta[0]), torch.float64 if int(meta[1]) else torch.float32
    mine = torch.cat(feats).to(dtype) if feats else torch.zeros(0, dim, dtype=dtype, device=device)
    if world == 1:
        return mine
    padded = torch.zeros(max(len(r) for r in rows), dim, dtype=dtype, device=device)
    padded[:mine.shape[0]] = mine
    shards = [torch.empty_like(padded) for _ in range(world)]
    dist.all_gather(shards, padded)
    out = torch.empty(len(ds), dim, dtype=dtype, device=device)
    for r in range(world):
        out[rows[r].to(device)] = shards[r][:len(rows[r])]
    return out


try:
    import click
except ImportError:                        # pragma: no cover
    click = None

if click is not None:
    @click.group()
    def main():
        """Calculate precision, recall, density and coverage -- the reference's prdc.py surface with the detector injected."""

    @main.command()
    @click.option('--images', 'image_path', help='Path to the images', metavar='PATH', type=str, required=True)
    @click.option('--images_ref', 'ref_path', help='Path to the reference images', metavar='PATH', type=str, required=True)
    @click.option('--num', 'num_expected', help='Number of images to use from each folder', metavar='INT', type=click.IntRange(min=2), show_default=True)
    @click.option('--seed', help='Random seed for selecting the images', metavar='INT', type=int, default=0, show_default=True)
    @click.option('--batch', help='Maximum batch size', metavar='INT', type=click.IntRange(min=1), default=250, show_default=True)
    @click.option('--nearest_k', help='Neighbour rank that defines a radius', metavar='INT', type=click.IntRange(min=1), default=5, show_default=True)
    @click.option('--detector', help='Feature extractor: reference .pkl, TorchScript .pt/.ts, or module:factory', type=str, required=True)
    @click.option('--device', type=str, default=None)
    def calc(image_path, ref_path, num_expected, seed, batch, nearest_k, detector, device):
        """Calculate precision, recall, density and coverage for a given set of images."""
        import os
        from . import fid
        dist, rank = fid._init_dist()
        device = device or ('cuda:%d' % int(os.environ.get('LOCAL_RANK', 0)) if torch.cuda.is_available() else 'cpu')
        log = print if rank == 0 else (lambda *a, **k: None)
        det = fid.load_detector(detector, device)
        kw = dict(num_expected=num_expected, seed=seed, max_batch_size=batch, device=device, log=log)
        reps_ref = extract_features(ref_path, det, **kw)
        reps_gen = extract_features(image_path, det, **kw)
        log('Computing scores...')
        try:
            if rank == 0:
                scores = compute_prdc(reps_ref, reps_gen, nearest_k=nearest_k, device=device)
                for key, value in scores.items():
                    print(f'{key}: {value:.5f}')
        finally:                                                 # the other ranks wait here: release them also when rank 0 fails
            if dist.is_initialized():
                dist.barrier()

    if __name__ == '__main__':
        main()
