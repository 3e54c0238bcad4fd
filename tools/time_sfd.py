#!/usr/bin/env python
"""Time the step-condition path of the SFD-distilled nets on the GPU: one evaluation with `step_condition=4` against `None` on the SAME engine,
the same for the SD-1.5 latent U-Net under classifier-free guidance,
the compose kernel (DS_OP_AFFINE_COMPOSE) alone at ImageNet-64's affine size, and the few-step Euler sampler the nets are distilled for.

    python tools/time_sfd.py [--rounds 5] [--out profiles/sfd_timing.txt]

Evaluation rows: `reps` raw evaluations (host-scalar sigma, as the samplers issue them) between one pair of events after warm-up, per-evaluation
time = window / reps; the two forms alternate, `rounds` windows each.  Kernel rows: 200 launches per window; bytes = both columns of every pair
read and written for every row, plus the step row once; the launch floor is the same operation on one row and one group.  No GPU: the tool fails.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_PEAK = 6.29e12        # bytes/s of a float4 copy kernel on this GPU (read + write)
# (config, batch, engine mode, evaluations per window: windows of 0.6 - 0.9 s)
CASES = [('cifar10', 256, {}, 16), ('cifar10', 8, {}, 150), ('imagenet64', 64, dict(use_fp16=True), 40)]
LDM_CASES = [('sd15', 16, dict(use_fp16=True), 20)]       # CFGDenoiser under guidance 7.5: 2 x 16 images per U-Net evaluation


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sfd_timing.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'this tool measures on the GPU'
    from diff_sampler_amd import _lib, solvers
    from diff_sampler_amd.engine import EDMDenoiser
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    pr = torch.cuda.get_device_properties(0)
    say(f'# tools/time_sfd.py --rounds {args.rounds}   ({pr.name}, {pr.multi_processor_count} CUs, torch {torch.__version__})')
    say()
    say('one raw evaluation F(x; sigma) with step_condition = 4 against None on the same engine (host-scalar sigma; windows alternate)')
    nets = {}
    for name, B, kw, reps in CASES:
        net = nets.get((name, bool(kw)))
        if net is None:
            net = nets[(name, bool(kw))] = EDMDenoiser.from_config(name, seed=5, step_condition=True, **kw)
        R = net.img_resolution
        g = torch.Generator().manual_seed(11)
        x = (torch.randn(B, 3, R, R, generator=g) * 2.5).cuda()
        lab = torch.eye(net.label_dim)[torch.randint(net.label_dim, (B,), generator=g)].cuda() if net.label_dim else None
        forms = {'None': (lambda: net.raw(x, 2.5, lab)), '4': (lambda: net.raw(x, 2.5, lab, step_condition=4))}
        for fn in forms.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        acc = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, fn in forms.items():
                acc[k].append(timed(fn, reps))
        rows = 1 if not net.label_dim else B
        nl = {k: len(net.engine.plan(B, rows, k != 'None').ops) for k in forms}
        mode = 'fp16' if kw else 'fp32'
        for k, ms in acc.items():
            say(f'    {name:10s} {mode} B={B:<4d} step_condition={k:5s} {nl[k]:4d} launches  ' + '  '.join(f'{v:9.4f}' for v in ms) +
                f' ms   median {statistics.median(ms):9.4f} ms')
        d = statistics.median(acc['4']) - statistics.median(acc['None'])
        spread = max(max(v) - min(v) for v in acc.values())
        say(f'    {"":10s} difference of the medians {1e3 * d:+8.1f} us = {100 * d / statistics.median(acc["None"]):+.3f} % of the None evaluation '
            f'(+{nl["4"] - nl["None"]} launches; largest spread inside one form {1e3 * spread:.1f} us)')
    from diff_sampler_amd.ldm_engine import CFGDenoiser
    for name, B, kw, reps in LDM_CASES:
        net = CFGDenoiser.from_config(name, seed=5, guidance_rate=7.5, step_condition=True, **kw)
        g = torch.Generator().manual_seed(12)
        R, ctx = net.img_resolution, net.spec.context_dim
        x = (torch.randn(B, net.img_channels, R, R, generator=g) * 2.5).cuda()
        c, uc = torch.randn(B, 77, ctx, generator=g).cuda(), torch.randn(B, 77, ctx, generator=g).cuda()
        forms = {'None': (lambda: net.raw(x, 2.5, c, uc)), '4': (lambda: net.raw(x, 2.5, c, uc, step_condition=4))}
        for fn in forms.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        acc = {k: [] for k in forms}
        for _ in range(args.rounds):
            for k, fn in forms.items():
                acc[k].append(timed(fn, reps))
        nl = {k: len(net.engine.plan(2 * B, 1, 77, k != 'None').ops) for k in forms}
        for k, ms in acc.items():
            say(f'    {name:10s} fp16 B={B:<4d} step_condition={k:5s} {nl[k]:4d} launches  ' + '  '.join(f'{v:9.4f}' for v in ms) +
                f' ms   median {statistics.median(ms):9.4f} ms')
        d = statistics.median(acc['4']) - statistics.median(acc['None'])
        spread = max(max(v) - min(v) for v in acc.values())
        wbytes = 4 * net.spec.time_embed_dim * net.engine.aff_total
        say(f'    {"":10s} difference of the medians {1e3 * d:+8.1f} us = {100 * d / statistics.median(acc["None"]):+.3f} % of the None evaluation '
            f'(+{nl["4"] - nl["None"]} launches; largest spread inside one form {1e3 * spread:.1f} us; emb_nfe_layers weights read per evaluation: '
            f'{wbytes / 1e6:.1f} MB)')
        del net
        torch.cuda.empty_cache()
    say()

    net = nets[('imagenet64', True)]
    eng = net.engine
    say(f'DS_OP_AFFINE_COMPOSE alone at ImageNet-64\'s affine size: {eng.aff_total} columns = {eng.w["step.pairs"].shape[0]} groups of four pairs')
    tiny_aff, tiny_step = torch.zeros(1, 8, device='cuda'), torch.zeros(8, device='cuda')
    tiny_pairs = torch.tensor([[0, 4]], dtype=torch.int32, device='cuda')
    ta = _lib.AffineComposeArgs(tiny_aff.data_ptr(), 8, 1, 8, tiny_step.data_ptr(), tiny_pairs.data_ptr(), 1)
    st = _lib.stream_ptr()
    handles = []

    def launcher(a):
        # a one-entry native plan, built once: the launch as ds_plan_run issues it
        import ctypes as C
        lib = _lib.load()
        h = C.c_void_p()
        _lib.check(lib.ds_plan_create(C.byref(h)), 'ds_plan_create')
        _lib.check(lib.ds_plan_add(h, _lib.DS_OP_AFFINE_COMPOSE, C.byref(a), C.sizeof(a)), 'ds_plan_add')
        handles.append(h)
        return lambda: _lib.check(lib.ds_plan_run(h, st), 'DS_OP_AFFINE_COMPOSE')

    floor = launcher(ta)
    for _ in range(20):
        floor()
    fl = [timed(floor, 200) for _ in range(5)]
    say(f'    launch floor (one row, one group, back-to-back launches)   {1e3 * statistics.median(fl):8.2f} us per launch')
    for rows in (64, 4, 1):
        aff = torch.zeros(rows, eng.aff_total, device='cuda')           # zeros stay zeros under the composition with a zero step row
        step = torch.zeros(eng.aff_total, device='cuda')
        a = _lib.AffineComposeArgs(aff.data_ptr(), eng.aff_total, rows, eng.aff_total, step.data_ptr(), eng.w['step.pairs'].data_ptr(),
                                   eng.w['step.pairs'].shape[0])
        go = launcher(a)
        for _ in range(10):
            go()
        ms = [timed(go, 200) for _ in range(5)]
        med = statistics.median(ms)
        nbytes = 2 * rows * eng.aff_total * 4 + eng.aff_total * 4 + eng.w['step.pairs'].numel() * 4
        say(f'    rows = {rows:3d}  {nbytes / 1024:8.1f} KiB  {1e3 * med:8.2f} us per launch (min {1e3 * min(ms):.2f} max {1e3 * max(ms):.2f})  '
            f'{nbytes / (med * 1e-3) / 1e9:8.2f} GB/s = {100 * nbytes / (med * 1e-3) / COPY_PEAK:5.2f} % of the copy figure, '
            f'{med / statistics.median(fl):5.2f} x the launch floor')
    say()

    net = nets[('cifar10', False)]
    lat = torch.randn(256, 3, 32, 32, generator=torch.Generator().manual_seed(3)).cuda()
    kw = dict(num_steps=4, afs=True)
    say('euler_sampler, AFS, num_steps = 4 (2 network evaluations), cifar10 fp32, B = 256 (4 calls per window, windows alternate)')
    forms = {'step_condition=4': (lambda: solvers.euler_sampler(net, lat, step_condition=4, **kw)), 'step_condition=None': (lambda: solvers.euler_sampler(net, lat, **kw))}
    for fn in forms.values():
        fn()
    acc = {k: [] for k in forms}
    for _ in range(args.rounds):
        for k, fn in forms.items():
            acc[k].append(timed(fn, 4))
    for k, ms in acc.items():
        say(f'    {k:20s} ' + '  '.join(f'{v:9.3f}' for v in ms) + f' ms per call   median {256 / statistics.median(ms) * 1e3:9.1f} images/s')
    for h in handles:
        _lib.load().ds_plan_destroy(h)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
