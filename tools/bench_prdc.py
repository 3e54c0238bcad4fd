"""The two kernels of csrc/metrics/prdc.hip at the metric's working size: N = 10 000 samples per set, D = 2048, fp32 features.
Reports time per call and fp64 TFLOP/s (2 * n_rows * n_cols * dim; v_mfma_f64_16x16x4_f64 peak 78.6) of dsm_knn_radii_sq and
dsm_prdc_cross (without and with realism), and of `compute_prdc` end to end, next to the stock-PyTorch fp64 expression of the same
quantities on the same GPU (rocBLAS fp64 GEMM into an N x N matrix, torch.topk / comparisons on it).

    python tools/bench_prdc.py [--n 10000] [--dim 2048] [--k 5] [--out profiles/prdc_bench.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diff_sampler_amd import prdc as P, _metrics_lib  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=10000)
    ap.add_argument('--dim', type=int, default=2048)
    ap.add_argument('--k', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    n, dim, k = a.n, a.dim, a.k
    lib = _metrics_lib.load()
    g = torch.Generator(device='cuda').manual_seed(0)
    real = torch.randn(n, dim, device='cuda', generator=g)
    fake = torch.randn(n, dim, device='cuda', generator=g) + 0.02
    ws = P._workspace(lib, n, n, k, real.device)
    flop = 2.0 * n * n * dim
    lines = [f'N = {n}, D = {dim}, k = {k}, fp32 features; {lib.dsm_prdc_splits(n, n)} column splits x {-(-n // 128)} row bands; '
             f'{torch.cuda.get_device_name(0)}']

    def row(name, ms, flops=flop):
        lines.append(f'{name:46s} {ms:9.2f} ms  {flops / ms / 1e9:6.1f} TF fp64  ({flops / ms / 1e9 / 78.6:.2f} of the matrix peak)')
        print(lines[-1], flush=True)

    rr = P._knn_radii_sq_device(real, k, ws)
    rf = P._knn_radii_sq_device(fake, k, ws)
    mask = torch.from_numpy(np.sqrt(rr.cpu().numpy()) < np.median(np.sqrt(rr.cpu().numpy())))
    row('dsm_knn_radii_sq', timed(lambda: P._knn_radii_sq_device(real, k, ws), a.reps))
    row('dsm_prdc_cross', timed(lambda: P._cross_device(real, fake, rr, rf, None, ws), a.reps))
    row('dsm_prdc_cross + realism', timed(lambda: P._cross_device(real, fake, rr, rf, mask, ws), a.reps))
    row('compute_prdc (3 passes, host finalisation)', timed(lambda: P.compute_prdc(real, fake, k), a.reps), 3 * flop)

    # stock PyTorch, fp64, the same quantities through a full N x N matrix
    r64, f64 = real.double(), fake.double()

    def sq(x, y):
        return ((x * x).sum(1)[:, None] + (y * y).sum(1)[None, :] - 2.0 * (x @ y.T)).clamp_(min=0.0)

    def torch_knn():
        d = sq(r64, r64)
        d.fill_diagonal_(0.0)
        return torch.topk(d, k + 1, dim=1, largest=False).values[:, k]

    def torch_cross():
        d = sq(r64, f64)
        return (d < rr[:, None]).sum(0), (d < rf[None, :]).sum(1), d.min(1).values

    row('torch fp64: GEMM only (rocBLAS, N x N out)', timed(lambda: r64 @ f64.T, a.reps))
    row('torch fp64: radii (GEMM + topk)', timed(torch_knn, a.reps))
    row('torch fp64: cross (GEMM + compares)', timed(torch_cross, a.reps))
    lines.append(f'max |radii_sq - torch| / max = {float((rr - torch_knn()).abs().max() / rr.max()):.2e}')
    print(lines[-1])
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
