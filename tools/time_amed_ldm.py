#!/usr/bin/env python
"""Time the AMED-Plugin sampler on the SD-1.5 latent U-Net (fp16 mode, classifier-free guidance) -> profiles/amed_ldm_timing.txt.

    python tools/time_amed_ldm.py [--out FILE] [--batch 16]

The reference's Stable Diffusion recipe (amed-solver-main/launch.sh:55-62): AMED-Plugin on DPM-Solver++(2M), noise prediction, num_steps = 4,
AFS, scale_time = 0.2, discrete schedule rho = 1, guidance 7.5 -- 5 evaluations of 2B images.  Random-init weights and a seeded predictor
(timing does not depend on them).  In ONE child process (--child, under a time limit of its own; this parent never touches the GPU):
1. the AMED sampler call, plain DPM-Solver++(2M) at the same evaluation count (num_steps = 6) and the AMED call with the sigma rows on the
   host route (solvers_amed.DEVICE_SIGMA = False: CFGSchedule.sigma_inv per evaluation), taking turns: latents/s and time per evaluation;
2. what one AMED step adds around its two evaluations: tap mean + predictor + two coefficient-row launches + the sigma rows of both
   evaluations (ds_fill + 2 x DS_OP_CFG_SIGMA_ROWS), and the same with the sigma rows made on the host as CFGDenoiser.raw does without
   device_sigma.
Every timing is a pair of events around ONE call on the current stream; median of 5 after 2 warm-up rounds, with min / max."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fmt(ms):
    return f'{statistics.median(ms):9.3f} ms (min {min(ms):.3f} max {max(ms):.3f}, n={len(ms)})'


def alternate(fns, calls=5, warm=2):
    """{name: [ms]}: the callables take turns, `warm` untimed rounds first."""
    import torch
    acc = {k: [] for k in fns}
    for rnd in range(calls + warm):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rnd >= warm:
                acc[k].append(e0.elapsed_time(e1))
    return acc


def child(B):
    import torch
    from diff_sampler_amd import _lib, ops, sample, solvers, solvers_amed
    from diff_sampler_amd._lib import AmedCoefArgs
    from diff_sampler_amd.ldm_engine import CFGDenoiser
    say = lambda s='': print(s, flush=True)
    pr = torch.cuda.get_device_properties(0)
    say(f'# tools/time_amed_ldm.py on {pr.gcnArchName} / {pr.multi_processor_count} CUs; SD-1.5 latent U-Net, fp16 mode, B = {B} latents '
        f'({2 * B} images per evaluation), guidance 7.5; median of 5 timed calls after 2 warm-up rounds, variants alternated')
    net = CFGDenoiser.from_config('sd15', seed=0, guidance_rate=7.5, use_fp16=True)
    dev = net.device
    recipe = dict(solver='dpmpp', num_steps=4, afs=True, max_order=2, predict_x0=False, lower_order_final=True, schedule_type='discrete',
                  schedule_rho=1, guidance_type='cfg', guidance_rate=7.5, scale_dir=0, scale_time=0.2, dataset_name='ms_coco')
    pred = sample.load_predictor('random:7', dev, random_init=True, **recipe)
    g = torch.Generator().manual_seed(0)
    lat = torch.randn(B, 4, 64, 64, generator=g).to(dev)
    c, uc = torch.randn(B, 77, 768, generator=g).to(dev), torch.randn(B, 77, 768, generator=g).to(dev)
    common = dict(condition=c, unconditional_condition=uc, sigma_min=net.sigma_min, sigma_max=net.sigma_max, schedule_type='discrete',
                  schedule_rho=1, max_order=2, predict_x0=False, lower_order_final=True)

    def amed():
        return solvers_amed.dpm_pp_sampler(net, lat, num_steps=4, afs=True, AMED_predictor=pred, **common)

    def amed_host():
        solvers_amed.DEVICE_SIGMA = False
        try:
            return amed()
        finally:
            solvers_amed.DEVICE_SIGMA = True

    def plain():
        return solvers.dpm_pp_sampler(net, lat, num_steps=6, **common)

    say()
    say('## 1. one sampler call, 5 network evaluations each')
    acc = alternate({'AMED-Plugin DPM-Solver++(2M), num_steps 4, AFS': amed, 'plain DPM-Solver++(2M), num_steps 6': plain,
                     'AMED-Plugin, sigma rows on the host route': amed_host})
    for k, v in acc.items():
        m = statistics.median(v)
        say(f'{k:48s} {fmt(v)}  {B / m * 1e3:7.2f} latents/s  {m / 5:8.3f} ms per evaluation')
    ma, mp, mh = (statistics.median(v) for v in acc.values())
    say(f'AMED - plain = {ma - mp:+.3f} ms per call ({(ma / mp - 1) * 100:+.2f} %); host route - device route = {mh - ma:+.3f} ms per call '
        f'({(mh - ma) / 3:+.3f} ms per step)')

    say()
    say('## 2. what one AMED step adds around its two evaluations (no network evaluation inside the timed region)')
    lib, st = _lib.load(), _lib.stream_ptr
    plan, _, doubled = net._last
    f32 = dict(dtype=torch.float32, device=dev)
    out4, c1, c2, s1, s2, thist = (torch.empty(B, 4, **f32), torch.empty(B, 8, **f32), torch.empty(B, 8, **f32), torch.empty(B, **f32),
                                   torch.empty(B, **f32), torch.zeros(B, 4, **f32))
    table = net.log_alpha_array.to(dev, torch.float32).contiguous()
    bufs = plan.bufs

    def coefs(stage, outc):
        a = AmedCoefArgs(C.c_void_p(out4.data_ptr()), 5.0, 1.5, solvers_amed.MODE['dpmpp'], stage, 1, 0, C.c_void_p(thist.data_ptr()),
                         C.c_void_p(outc.data_ptr()), C.c_void_p(s2.data_ptr()) if stage == 1 else None, B)
        _lib.check(lib.ds_amed_coefs(C.byref(a), st()), 'ds_amed_coefs')

    def device_rows(sg):
        ops.cfg_sigma_rows(sg, B, table, 2, bufs['sigma'], bufs['c_noise'])

    def host_rows(sg):                                    # what CFGDenoiser.raw does with a [B] tensor and no device_sigma
        cn = (net.M * net.sigma_inv(sg) - 1.).to(torch.float32)
        bufs['sigma'].copy_(torch.cat([sg, sg]))
        bufs['c_noise'].copy_(torch.cat([cn, cn]))

    def step(rows):
        ops.fill(s1, 5.0)
        rows(s1)
        bott = net.bottleneck_mean(plan, B, doubled)
        pred.predict(bott, 5.0, 1.5, out4)
        coefs(1, c1)
        rows(s2)
        coefs(2, c2)
    acc = alternate({'tap mean + predictor + 2 x coefficient rows + sigma rows on the device': lambda: step(device_rows),
                     'the same with the sigma rows on the host route': lambda: step(host_rows),
                     'tap mean (DS_OP_CHANNEL_MEAN_F16, 1280 channels) alone': lambda: net.bottleneck_mean(plan, B, doubled),
                     '2 x DS_OP_CFG_SIGMA_ROWS alone': lambda: (device_rows(s1), device_rows(s2)),
                     '2 x host sigma rows alone': lambda: (host_rows(s1), host_rows(s2))})
    assert bufs[net.bottleneck_name].dtype == torch.float16
    for k, v in acc.items():
        say(f'{k:76s} {fmt(v)}')
    say(f'per step, as a share of its two evaluations ({2 * mp / 5:.2f} ms): device route {statistics.median(list(acc.values())[0]) / (2 * mp / 5) * 100:.3f} %, '
        f'host route {statistics.median(list(acc.values())[1]) / (2 * mp / 5) * 100:.3f} %')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'amed_ldm_timing.txt'))
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.batch)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--batch', str(args.batch)], capture_output=True, text=True, timeout=840)
    print(r.stdout, end='')
    if r.returncode:
        print(r.stderr[-3000:], file=sys.stderr)
        sys.exit(r.returncode)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(r.stdout)


if __name__ == '__main__':
    main()
