#!/usr/bin/env python
"""LSUN-256 consistency-model net (cm_engine.CMDenoiser, random-init, fp16 mode): sampler throughput and the per-layer times of the 3x3
convolutions at 128 and 256 pixels with the wide fp16 block convolutions on (`wide16=True`: csrc/conv3x3_f16wide.hip, kernel ids 2575 / 2576)
and off (the fp32 routes the same layers take without them -- the parent's kernels on the same layers).

    python tools/bench_cm.py [--batch 8] [--steps 6] [--reps 5] [--out profiles/cm_lsun_wide16_ab.txt]

Both engines live in one process and alternate rep by rep (same clocks, same neighbours on the machine); every figure is a median over the reps.
Sampler: DPM-Solver++(2M), `--steps` - 1 evaluations per image.  Layer times: every launch of the plan bracketed by a device event pair inside
whole evaluations (tools/time_plan_ops.py's method), summed per layer shape.  A layer on the fp32 route costs its convolution AND the fp32
normalisation pass the route needs where the fp16 route has an fp16 pass; the table lists the convolutions, the end-to-end lines show the rest."""
import argparse
import collections
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diff_sampler_amd import _lib, solvers  # noqa: E402
from diff_sampler_amd.cm_engine import CMDenoiser  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--config', default='lsun_bedroom')
ap.add_argument('--batch', type=int, default=8)
ap.add_argument('--steps', type=int, default=6, help='num_steps of the sampler: steps - 1 evaluations')
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--out', default='')
args = ap.parse_args()
assert torch.cuda.is_available(), 'bench_cm.py measures on the GPU only'
lib = _lib.load()
st = _lib.stream_ptr()
lines = []


def say(s=''):
    print(s, flush=True)
    lines.append(s)


t0 = time.time()
nets = {flag: CMDenoiser.from_config(args.config, seed=0, use_fp16=True, wide16=flag) for flag in (True, False)}
R = nets[True].img_resolution
g = torch.Generator().manual_seed(1)
lat = torch.randn(args.batch, 3, R, R, generator=g).cuda()
x = lat * 3.0
sample = lambda net: solvers.dpm_pp_sampler(net, lat, num_steps=args.steps, sigma_min=0.002, sigma_max=80., schedule_type='polynomial', schedule_rho=7,
                                            max_order=2, predict_x0=True, lower_order_final=True)
for net in nets.values():             # warm-up: plan build (tile measurements on a table miss), code objects
    sample(net); net(x, 3.0)
torch.cuda.synchronize()
say(f'# {args.config} random-init fp16, batch {args.batch}, DPM-Solver++(2M) NFE {args.steps - 1}; set-up {time.time() - t0:.1f} s; medians of {args.reps} alternating reps')

# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
wall = {True: [], False: []}
for _ in range(args.reps):
    for flag, net in nets.items():
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = sample(net)
        torch.cuda.synchronize()
        wall[flag].append(time.perf_counter() - t)
med = {f: statistics.median(v) for f, v in wall.items()}
for flag in (True, False):
    say(f'sampler wide16={flag!s:5s}: {med[flag] * 1e3:9.1f} ms per batch (min {min(wall[flag]) * 1e3:.1f}, max {max(wall[flag]) * 1e3:.1f})  '
        f'{args.batch / med[flag]:7.2f} images/s')
say(f'speed-up of the sampler from wide16: {med[False] / med[True]:.2f} x')


# ---- per layer ------------------------------------------------------------------------------------------------------------------------------
def layer_times(net):
    """{op index: [us per rep]} and the plan of one evaluation at the benchmark batch."""
    net(x, 3.0)
    plan = net._last[0]
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in plan.ops]
    return plan, ev


state = {f: layer_times(n) for f, n in nets.items()}
acc = {f: collections.defaultdict(list) for f in nets}
for _ in range(args.reps):
    for flag, net in nets.items():
        plan, ev = state[flag]
        net(x, 3.0)
        for (e0, e1), op in zip(ev, plan.ops):
            e0.record()
            rc = op.fn(*op.args, st)
            e1.record()
            assert rc == 0, op.name
        torch.cuda.synchronize()
        for i, (e0, e1) in enumerate(ev):
            acc[flag][i].append(e0.elapsed_time(e1) * 1e3)


def table(flag):
    """{layer label: (launches, median us summed over them, kernel ids)} of the 3x3 convolutions above 64 pixels; + totals by op kind above 64 pixels."""
    plan, _ = state[flag]
    rows, kinds = collections.OrderedDict(), collections.defaultdict(float)
    for i, op in enumerate(plan.ops):
        a = op.keep[0] if op.keep else None
        us = statistics.median(acc[flag][i])
        if op.fn is lib.ds_conv2d_nhwc and a.taps == 9 and a.w >= 128 and a.cout >= 64:
            lab = f'{a.h}x{a.w} {a.c0 + a.c1}{"+" + str(a.ec0 + a.ec1) if a.ec0 else ""}->{a.cout}{" cbias" if a.cbias else ""}{" res" if a.res else ""}'
            r = rows.setdefault(lab, [0, 0.0, set(), 2.0 * a.n * a.h * a.w * a.cout * (9 * (a.c0 + a.c1) + a.ec0 + a.ec1)])
            r[0] += 1; r[1] += us; r[2].add(plan.kernel_ids[op.name])
            kinds['conv3x3'] += us
        elif a is not None and hasattr(a, 'w') and hasattr(a, 'h') and getattr(a, 'w', 0) >= 128:
            kinds[op.fn.__name__] += us
    return rows, kinds


on, kon = table(True)
off, koff = table(False)
say()
say(f'{"3x3 layer above 64 pixels":40s} {"n":>2s} {"wide16 us":>10s} {"ids":>10s} {"TFLOP/s":>8s} | {"off us":>10s} {"ids":>10s} {"TFLOP/s":>8s} | {"off/on":>6s}')
for lab in on:
    a, b = on[lab], off.get(lab)
    ids = lambda s: ','.join(str(v) for v in sorted(s))
    if b is None:
        say(f'{lab:40s} {a[0]:2d} {a[1]:10.1f} {ids(a[2]):>10s} {a[3] * a[0] / a[1] / 1e6:8.0f} | (no such launch)')
        continue
    say(f'{lab:40s} {a[0]:2d} {a[1]:10.1f} {ids(a[2]):>10s} {a[3] * a[0] / a[1] / 1e6:8.0f} | {b[1]:10.1f} {ids(b[2]):>10s} {b[3] * b[0] / b[1] / 1e6:8.0f} | '
        f'{b[1] / a[1]:6.2f}{"   <-- not faster" if b[1] <= a[1] else ""}')
say()
say('launch time above 64 pixels by entry point (us per evaluation; the fp32 route pays in its passes too):')
for k in sorted(set(kon) | set(koff)):
    say(f'  {k:24s} wide16 {kon.get(k, 0.0):10.1f}   off {koff.get(k, 0.0):10.1f}')
for flag in (True, False):
    plan, _ = state[flag]
    say(f'whole evaluation, sum of event pairs, wide16={flag}: {sum(statistics.median(v) for v in acc[flag].values()) / 1e3:.2f} ms ({len(plan.ops)} launches)')
if args.out:
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')
