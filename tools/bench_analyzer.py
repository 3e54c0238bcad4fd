"""dsm_traj_gram (csrc/metrics/traj.hip) at the two working shapes of the reference's notebooks: main_extend.ipynb's T = 1001 points,
B = 100 trajectories, and main_mp.ipynb's T = 21, B = 64, both D = 3072 (CIFAR-10), fp32 trajectories.  Reports time per call, fp64
TFLOP/s -- of the full product (2 T^2 D B, what the result is worth) and of what the kernel executes (whole 128 x 128 tiles on and below
the diagonal; v_mfma_f64_16x16x4_f64 peak 78.6) -- and the peak device memory beyond the trajectory itself, next to the stock-PyTorch
route on the same data: cast to fp64, subtract the end point, permute to [B, T, D], torch.bmm (rocBLAS).  Also times dsm_row_sqdist.

    python tools/bench_analyzer.py [--shapes 1001x100x3072,21x64x3072] [--reps 20] [--rounds 3] [--out profiles/analyzer_bench.txt]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diff_sampler_amd import analyzer, _metrics_lib  # noqa: E402


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


def peak_extra(fn):
    """Peak bytes allocated during fn() beyond what was allocated before it."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def stock(traj):
    y = traj.double()
    y = (y - y[-1:]).permute(1, 0, 2)
    return torch.bmm(y, y.transpose(1, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='1001x100x3072,21x64x3072')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    lib = _metrics_lib.load()
    lines = [f'{torch.cuda.get_device_name(0)}; fp32 trajectories [T][B][D], fp64 Gram matrices [B][T][T]; {a.rounds} alternating rounds of '
             f'{a.reps} timed calls, each after one warm-up call']

    def say(s):
        lines.append(s)
        print(s, flush=True)

    for shape in a.shapes.split(','):
        T, B, D = (int(v) for v in shape.split('x'))
        g = torch.Generator(device='cuda').manual_seed(0)
        traj = torch.cumsum(torch.randn(T, B, D, device='cuda', generator=g), dim=0)
        flop = 2.0 * T * T * D * B
        say(f'T = {T}, B = {B}, D = {D}: trajectory {traj.numel() * 4 / 1e6:.0f} MB, Gram {B * T * T * 8 / 1e6:.1f} MB, '
            f'{lib.dsm_traj_gram_splits(T, D)} split(s) x {-(-T // 128) * (-(-T // 128) + 1) // 2} lower tile(s) per sample')
        tiles = -(-T // 128) * (-(-T // 128) + 1) // 2
        executed = 2.0 * tiles * 128 * 128 * (-(-D // 16) * 16) * B    # what the kernel's MFMAs do: whole 128 x 128 tiles, lower ones only
        routes = (('dsm_traj_gram (analyzer.trajectory_gram)', lambda: analyzer.trajectory_gram(traj), executed),
                  ('torch: double, subtract, permute, bmm', lambda: stock(traj), flop))
        times = {name: [] for name, _, _ in routes}
        for _ in range(a.rounds):                                      # the two routes alternate: both see the same state of the box
            for name, fn, _ in routes:
                times[name].append(timed(fn, a.reps))
        for name, fn, done in routes:
            ms = sorted(times[name])[len(times[name]) // 2]
            mem = peak_extra(fn)
            say(f'  {name:44s} {ms:9.3f} ms (median of {a.rounds}: {min(times[name]):.3f} .. {max(times[name]):.3f})  '
                f'{flop / ms / 1e9:6.2f} TF of the full T x T product; executed {done / ms / 1e9:6.2f} TF = '
                f'{done / ms / 1e9 / 78.6:.3f} of the fp64 matrix peak;  peak extra memory {mem / 1e6:9.1f} MB')
        ref = stock(traj)
        got = analyzer.trajectory_gram(traj)
        say(f'  max |kernel - torch| / max |torch| = {float((got - ref).abs().max() / ref.abs().max()):.2e}')
        del ref, got
        ms = timed(lambda: analyzer._row_sq(traj), a.reps)
        say(f'  {"dsm_row_sqdist (T B rows of D)":44s} {ms:9.3f} ms  {traj.numel() * 4 / ms / 1e6:6.0f} GB/s read (incl. the copy of T B doubles to the host)')
        del traj
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
