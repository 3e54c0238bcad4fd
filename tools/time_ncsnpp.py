#!/usr/bin/env python
"""Time the NCSN++ path on the GPU: the FIR resampler at the CIFAR-10 `ve` shapes, and one denoiser evaluation of `cifar10_ve` next to
`cifar10` (DDPM++) and next to the functional restatement of both (tests/_ncsnpp_ref.py) in stock PyTorch-ROCm fp32 on the same GPU in the
same process.

    python tools/time_ncsnpp.py [--batch 256] [--calls 7] [--out profiles/ncsnpp_timing.txt]

Kernel rows: `reps` launches between one pair of events on the current stream after warm-up launches, per-launch time = window / reps;
bytes = input rows + output rows (what the algorithm must move; the 4x re-read of the down form's input is served by the caches);
the launch floor is the same entry point on a 2 x 2 x 4 tensor, timed the same way.  Evaluation rows: an event pair around ONE call,
engine and stock calls alternating, median with min / max.  The per-launch table is one replay of the plan with an event pair per launch,
grouped by launch kind.  No GPU: the tool fails.
"""
import argparse
import collections
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

COPY_PEAK = 6.29e12        # bytes/s of a float4 copy kernel on this GPU (read + write)


def fmt(ms):
    return f'{statistics.median(ms):9.3f} ms (min {min(ms):.3f} max {max(ms):.3f}, n={len(ms)})'


def timed(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def fir_launcher(n, h, w, c, up, pad):
    from diff_sampler_amd import _lib, _metrics_lib as ML
    mlib = ML.load()
    ho, wo = (2 * h, 2 * w) if up else ((h + 2 * pad - 4) // 2 + 1, (w + 2 * pad - 4) // 2 + 1)
    x = torch.randn(n * h * w, c, device='cuda')
    out = torch.empty(n * ho * wo, c, device='cuda')
    a = ML.DsmFirArgs(x.data_ptr(), c, n, h, w, c, int(up), pad, (C.c_float * 4)(1, 3, 3, 1), None, None, 0, 1.0, out.data_ptr(), c)

    def go():
        rc = mlib.dsm_fir_resample(C.byref(a), _lib.stream_ptr())
        assert rc == 0, rc
    return go, (x.numel() + out.numel()) * 4, (x, out, a)


def launch_table(plan, say):
    from diff_sampler_amd import _lib
    st = _lib.stream_ptr()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in plan.ops]
    for (e0, e1), op in zip(ev, plan.ops):
        e0.record()
        rc = op.fn(*op.args, st)
        e1.record()
        assert rc == 0, op.name
    torch.cuda.synchronize()
    kinds = collections.OrderedDict()
    for (e0, e1), op in zip(ev, plan.ops):
        fn = op.fn.__name__
        kind = fn
        if fn == 'ds_conv2d_nhwc':
            kind = 'ds_conv2d_nhwc 3x3' if op.keep[0].taps == 9 else 'ds_conv2d_nhwc 1x1 / linear'
            if 'aux_residual' in op.name:
                kind = 'ds_conv2d_nhwc aux_residual'
        k = kinds.setdefault(kind, [0, 0.0])
        k[0] += 1
        k[1] += e0.elapsed_time(e1)
    total = sum(v[1] for v in kinds.values())
    for kind, (cnt, ms) in sorted(kinds.items(), key=lambda kv: -kv[1][1]):
        say(f'    {kind:34s} {cnt:4d} launches {ms:9.3f} ms  {100 * ms / total:5.1f} %')
    say(f'    {"all launches (event pairs)":34s} {len(plan.ops):4d} launches {total:9.3f} ms')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--calls', type=int, default=7)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ncsnpp_timing.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool measures on the GPU'
    import diff_sampler_amd.arch as arch
    from diff_sampler_amd.engine import EDMDenoiser
    import _ncsnpp_ref as R
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    B = args.batch
    pr = torch.cuda.get_device_properties(0)
    say(f'# tools/time_ncsnpp.py --batch {B} --calls {args.calls}   ({pr.name}, {pr.multi_processor_count} CUs, torch {torch.__version__})')
    say()
    say(f'dsm_fir_resample at the cifar10_ve shapes, B = {B}, 256 channels, taps [1,3,3,1] (bytes = input + output rows; copy figure 6.29 TB/s)')
    floor, _, keep0 = fir_launcher(1, 2, 2, 4, False, 1)
    for _ in range(20):
        floor()
    fl = [timed(floor, 200) for _ in range(5)]
    say(f'    launch floor (2 x 2 x 4 tensor, back-to-back launches)          {1e3 * statistics.median(fl):8.2f} us per launch')
    for tag, h, up in (('down 32 -> 16', 32, False), ('up    8 -> 16', 8, True), ('up   16 -> 32', 16, True)):
        go, nbytes, keep = fir_launcher(B, h, h, 256, up, 1)
        for _ in range(5):
            go()
        ms = [timed(go, 20) for _ in range(7)]
        med = statistics.median(ms)
        say(f'    {tag}   {nbytes / 2 ** 20:8.1f} MiB  {1e3 * med:8.2f} us per launch (min {1e3 * min(ms):.2f} max {1e3 * max(ms):.2f})  '
            f'{nbytes / med / 1e9:7.2f} TB/s  = {100 * nbytes / (med * 1e-3) / COPY_PEAK:5.1f} % of the copy figure,  {med / statistics.median(fl):6.1f} x the launch floor')
        del go, keep
    say()

    g = torch.Generator().manual_seed(11)
    x = (torch.randn(B, 3, 32, 32, generator=g) * 3.0).cuda()
    sigma = torch.full((B,), 2.5, device='cuda')
    nets, refs = {}, {}
    for name in ('cifar10', 'cifar10_ve'):
        spec = arch.edm_precond_spec(**arch.NAMED_CONFIGS[name])
        params = arch.init_params(spec, seed=5)
        nets[name] = EDMDenoiser(spec, params)
        p_dev = {k: v.cuda() for k, v in params.items()}
        refs[name] = (lambda p=p_dev, s=spec: R.edm_ncsnpp(p, s, x, sigma))
    fns = {}
    key = lambda name, what: f'{name:11s} {what}'
    for name in nets:
        fns[key(name, 'engine')] = (lambda n=nets[name]: n(x, sigma))
        fns[key(name, 'PyTorch-ROCm restatement')] = refs[name]
    for name in nets:
        out, ref = nets[name](x, sigma), refs[name]()
        torch.cuda.synchronize()
        say(f'{name}: engine vs PyTorch-ROCm restatement, max |a - b| / max |b| = {float((out - ref).abs().max() / ref.abs().max()):.2e}')
    acc = {k: [] for k in fns}
    for r in range(2 + args.calls):
        for k, fn in fns.items():
            ms = timed(fn)
            if r >= 2:
                acc[k].append(ms)
    say()
    say(f'one denoiser evaluation D(x; sigma), B = {B}, fp32, per-sample sigma (event pair around one call, alternating)')
    for k, ms in acc.items():
        say(f'    {k:40s} {fmt(ms)}   {B / statistics.median(ms) * 1e3:9.0f} img/s')
    med = {k: statistics.median(v) for k, v in acc.items()}
    eng, ref = (lambda n: med[key(n, 'engine')]), (lambda n: med[key(n, 'PyTorch-ROCm restatement')])
    say(f'    cifar10_ve / cifar10 on the engine: {eng("cifar10_ve") / eng("cifar10"):.3f} x;   PyTorch-ROCm / engine: cifar10 '
        f'{ref("cifar10") / eng("cifar10"):.2f} x, cifar10_ve {ref("cifar10_ve") / eng("cifar10_ve"):.2f} x')
    for name in nets:
        say()
        say(f'{name}: one replay of the plan (B = {B}), an event pair per launch, by launch kind')
        plan = nets[name].engine.plan(B, B)
        launch_table(plan, say)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
