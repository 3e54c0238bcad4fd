"""Cost of the batch-invariant mode: one network evaluation (the plan's launches, CUDA events, median of alternating repeats) under the
default route and under batch_invariant=True, per configuration and batch; then, per convolution of the CIFAR-10 fp32 plan at 8 images, the
launch under the default route against the same launch under the invariant route, next to the layer's chain-latency floor: K / 2 dependent
v_mfma_f32_32x32x2_f32 steps of 64 cycles at 2.4 GHz (the time one output's k-ordered chain takes without split-K, whatever the tile).
Writes profiles/batch_invariant_timing.txt.

    python tools/time_batch_invariant.py [--reps 20] [--out profiles/batch_invariant_timing.txt]
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from diff_sampler_amd import _lib  # noqa: E402

CASES = [('cifar10', 'edm', {}, b) for b in (1, 8, 64, 256)] + [('imagenet64', 'edm', dict(use_fp16=True), 64)] + \
        [('sd15', 'ldm', dict(use_fp16=True), b) for b in (1, 16)]


def _net(name, kind, kw, inv):
    if kind == 'edm':
        from diff_sampler_amd.engine import EDMDenoiser
        return EDMDenoiser.from_config(name, seed=0, batch_invariant=inv, **kw)
    from diff_sampler_amd.ldm_engine import CFGDenoiser
    return CFGDenoiser.from_config(name, seed=0, guidance_rate=7.5, batch_invariant=inv, **kw)


def _plan(net, kind, B):
    """The plan of a sampler call at B images (per-sample sigma, like the solvers) with its inputs filled once."""
    dev = torch.device('cuda')
    g = torch.Generator().manual_seed(B)
    if kind == 'edm':
        R, Cc = net.img_resolution, net.img_channels
        x = torch.randn(B, Cc, R, R, generator=g).to(dev)
        sig = torch.full((B,), 2.5, device=dev)
        lab = torch.eye(net.label_dim, device=dev)[torch.zeros(B, dtype=torch.long)] if net.label_dim else None
        net(x, sig, class_labels=lab)
        return net.engine.plan(B, B)
    x = torch.randn(B, 4, 64, 64, generator=g).to(dev)
    c, u = torch.randn(B, 77, 768, generator=g).to(dev), torch.randn(B, 77, 768, generator=g).to(dev)
    net(x, torch.full((B,), 2.5, device=dev), condition=c, unconditional_condition=u)
    return net.engine.plan(2 * B, 2 * B, 77)


def _time(plan, reps):
    st = _lib.stream_ptr()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        plan.run(st)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return sorted(ms)[len(ms) // 2]


CLOCK_GHZ = 2.4
CHAIN_CYCLES = 64          # dependent-accumulator latency of v_mfma_f32_32x32x2_f32 (cdna_hip_programming.md)


def _time_launch(lib, a, reps):
    """us per launch of one ds_conv2d_nhwc argument struct (median of three groups of `reps` back-to-back launches)."""
    import ctypes as C
    st = _lib.stream_ptr()
    for _ in range(2):
        _lib.check(lib.ds_conv2d_nhwc(C.byref(a), st), 'conv')
    ms = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            lib.ds_conv2d_nhwc(C.byref(a), st)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / reps)
    return sorted(ms)[1] * 1e3


def per_layer(B, reps):
    """Rows of the per-layer A/B of the CIFAR-10 fp32 plan at B images (per-sample sigma), default vs invariant route per launch."""
    import ctypes as C
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import _routing
    lib = _lib.load()
    net = _net('cifar10', 'edm', {}, True)
    P = _plan(net, 'edm', B)
    rows = [f'# per layer, CIFAR-10 fp32, B = {B}: the same launch under the default route (tune.invariant = 0) and the invariant route;',
            f'# floor = K / 2 x {CHAIN_CYCLES} cycles at {CLOCK_GHZ} GHz',
            f'{"layer":<28}{"K":>6}{"default":>16}{"us":>9}{"invariant":>16}{"us":>9}{"ratio":>7}{"floor us":>10}']
    tot = [0.0, 0.0, 0.0]
    for op in P.ops:
        if op.fn is not lib.ds_conv2d_nhwc:
            continue
        a = op.keep[0]
        inv = a.tune.invariant
        K = a.taps * (a.c0 + a.c1) + a.ec0 + a.ec1
        res = {}
        for flag in (0, inv):
            a.tune.invariant = flag
            r = _routing.conv_route(a)
            res[flag] = (f'{r.kernel_id}/s{r.splits}', _time_launch(lib, a, reps))
        a.tune.invariant = inv
        floor = K / 2 * CHAIN_CYCLES / (CLOCK_GHZ * 1e3)
        (kd, td), (ki, ti) = res[0], res[inv]
        tot[0] += td; tot[1] += ti; tot[2] += floor
        rows.append(f'{op.name:<28}{K:>6}{kd:>16}{td:>9.1f}{ki:>16}{ti:>9.1f}{ti / td:>7.2f}{floor:>10.1f}')
    rows.append(f'{"sum of the convolutions":<28}{"":>6}{"":>16}{tot[0]:>9.1f}{"":>16}{tot[1]:>9.1f}{tot[1] / tot[0]:>7.2f}{tot[2]:>10.1f}')
    P.close()
    del net
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--layer_batch', type=int, default=8)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'batch_invariant_timing.txt'))
    args = ap.parse_args()
    lines = [f'# tools/time_batch_invariant.py, {time.strftime("%Y-%m-%d")}, {torch.cuda.get_device_name(0)}',
             '# one network evaluation (ms, median of alternating groups of repeats): default route vs batch_invariant=True',
             f'{"config":<22}{"B":>5}{"default ms":>12}{"invariant ms":>14}{"ratio":>8}']
    for name, kind, kw, B in CASES:
        nets = {inv: _net(name, kind, kw, inv) for inv in (False, True)}
        plans = {inv: _plan(nets[inv], kind, B) for inv in (False, True)}
        for inv in (False, True):
            _time(plans[inv], 3)
        t = {False: [], True: []}
        for _ in range(3):                                    # alternate, so clock and thermal drift hit both alike
            for inv in (False, True):
                t[inv].append(_time(plans[inv], args.reps))
        d, i = sorted(t[False])[1], sorted(t[True])[1]
        mode = 'fp16' if kw.get('use_fp16') else 'fp32'
        lines.append(f'{name + "_" + mode:<22}{B:>5}{d:>12.3f}{i:>14.3f}{i / d:>8.3f}')
        print(lines[-1], flush=True)
        del nets, plans
        torch.cuda.empty_cache()
    lines += [''] + per_layer(args.layer_batch, args.reps)
    print('\n'.join(lines[-4:]), flush=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
