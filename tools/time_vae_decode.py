#!/usr/bin/env python
"""Time the AutoencoderKL decoder and its wide-image convolution kernel on the GPU -> profiles/vae_decode_timing.txt.

    python tools/time_vae_decode.py [--out FILE] [--quick]

1. Every distinct 3x3 layer of the sd15 decoder above 64 pixels wide, alone: the fp16-activation patch kernel (csrc/conv3x3_f16wide.hip, id 2575)
   against the only route those layers had before it -- the generic fp32 gather kernel (ds_conv_tune.mode = 1) on the fp32 copy of the same
   operands.  Old and new alternate inside one process; median of the timed calls with min / max; TFLOP/s = 2 x 9 x cin x cout x pixels / time.
2. The whole decode at B = 1 and 16 in both modes (one ds_plan_run each).
3. SD-1.5 DPM-Solver++(2M) NFE = 10 at B = 16 in fp16 mode, without and with the decode: images/s of BASELINE config 5 when an image is a picture.
Warm-up calls first; every timing is a pair of events around ONE call on the current stream."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP16_PEAK_TFLOPS = 2500.0      # MI355X dense fp16 matrix rate (README.md status table quotes fractions of it)


def timed(fn, calls, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def fmt(ms):
    return f'{statistics.median(ms):9.3f} ms  (min {min(ms):.3f}  max {max(ms):.3f}, n={len(ms)})'


def layer_args(n, side, cin, cout, f16, gen):
    from diff_sampler_amd import _lib, ops
    dev = 'cuda'
    rows = n * side * side
    x = torch.randn(rows, cin, generator=gen, device=dev)
    wt = torch.randn(cout, cin, 3, 3, generator=gen, device=dev) / (9 * cin) ** 0.5
    bias = torch.randn(cout, generator=gen, device=dev)
    keep = [bias]
    if f16:
        x = x.to(torch.float16)
        wp = ops.pack_conv_weight_f16(wt)
        out = torch.empty(rows, cout, dtype=torch.float16, device=dev)
    else:
        wp = ops.pack_conv_weight(wt)
        out = torch.empty(rows, cout, device=dev)
    a = _lib.ConvArgs(x.data_ptr(), None, cin, 0, cin, 0, n, side, side, 9, wp.data_ptr(), cout, bias.data_ptr(), None, 0, 1, None, 0, 1.0, 0,
                      out.data_ptr(), cout)
    if f16:
        a.wgt_f16, a.in_f16, a.out_f16 = 1, 1, 1
    else:
        a.tune.mode = 1
    keep += [x, wp, out]
    return a, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vae_decode_timing.txt'))
    ap.add_argument('--quick', action='store_true', help='fewer calls, no fp32 decode at B = 16, no sampler section')
    args = ap.parse_args()
    from diff_sampler_amd import _lib, solvers, vae_arch
    from diff_sampler_amd.vae_engine import VAEDecoder
    lib = _lib.load()
    calls = 5 if args.quick else 7
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    pr = torch.cuda.get_device_properties(0)
    say(f'# tools/time_vae_decode.py on {pr.gcnArchName} / {pr.multi_processor_count} CUs; median of {calls} timed calls after 2 warm-up calls, old and new alternated')
    spec = vae_arch.vae_decoder_spec(**vae_arch.NAMED_VAE_CONFIGS['sd15'])
    say(f'# decoder FLOPs per image (2 x MAC): {vae_arch.vae_flops_per_image(spec) / 1e12:.6f} TFLOP')
    say()
    say('## 1. wide 3x3 layers alone: fp16 patch kernel (id 2575) vs generic fp32 kernel (tune.mode = 1), random operands')
    shapes = sorted({(l.res_out, cin, cout) for l in spec.layers if l.res_out > 64 and l.kind in ('res', 'up')
                     for cin, cout in ([(l.cin, l.cout), (l.cout, l.cout)] if l.kind == 'res' else [(l.cin, l.cout)])})
    gen = torch.Generator(device='cuda')
    gen.manual_seed(1)
    st = _lib.stream_ptr()
    for n in (1, 4):
        for side, cin, cout in shapes:
            new, k1 = layer_args(n, side, cin, cout, True, gen)
            old, k2 = layer_args(n, side, cin, cout, False, gen)
            assert lib.ds_conv_kernel_id(C.byref(new)) == 2575 and lib.ds_conv_kernel_id(C.byref(old)) == 0
            t_new, t_old = [], []
            for rnd in range(calls + 2):                    # alternate; the first two rounds are warm-up
                for a, acc in ((old, t_old), (new, t_new)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    rc = lib.ds_conv2d_nhwc(C.byref(a), st)
                    e1.record()
                    e1.synchronize()
                    assert rc == 0
                    if rnd >= 2:
                        acc.append(e0.elapsed_time(e1))
            fl = 2.0 * 9 * cin * cout * n * side * side
            mn, mo = statistics.median(t_new), statistics.median(t_old)
            say(f'B={n} {side:3d}x{side:<3d} {cin:3d}->{cout:3d}  new {fmt(t_new)} {fl / mn / 1e9:7.1f} TFLOP/s = {fl / mn / 1e9 / FP16_PEAK_TFLOPS:.3f} of fp16 peak'
                f' | old {fmt(t_old)} {fl / mo / 1e9:6.1f} TFLOP/s | speed-up {mo / mn:5.2f}x (worst pair {min(t_old) / max(t_new):.2f}x)')
            del k1, k2
            torch.cuda.empty_cache()
    say()
    say('## 2. whole decode, one ds_plan_run (latents in the plan, output [B, 3, 512, 512] fp32)')
    for fp16 in (True, False):
        dec = VAEDecoder.from_config('sd15', seed=0, use_fp16=fp16)
        for B in (1, 16):
            if args.quick and not fp16 and B == 16:
                continue
            z = torch.randn(B, 4, 64, 64, device='cuda') * 0.7
            ms = timed(lambda: dec.raw(z), calls)
            m = statistics.median(ms)
            say(f'{"fp16" if fp16 else "fp32"} B={B:2d}  {fmt(ms)}  {m / B:8.3f} ms/image  {dec.flops(B) / m / 1e9:7.1f} TFLOP/s')
        del dec
        torch.cuda.empty_cache()
    if not args.quick:
        say()
        say('## 3. SD-1.5 fp16, DPM-Solver++(2M) NFE = 10, B = 16 (random init, fixed conditions): latents only vs latents + decode')
        from diff_sampler_amd.ldm_engine import CFGDenoiser
        B = 16
        net = CFGDenoiser.from_config('sd15', seed=0, guidance_rate=7.5, use_fp16=True)
        dec = VAEDecoder.from_config('sd15', seed=0, use_fp16=True)
        lat = torch.randn(B, 4, 64, 64, device='cuda')
        c, uc = torch.randn(B, 77, 768, device='cuda'), torch.randn(B, 77, 768, device='cuda')

        def sample():
            return solvers.dpm_pp_sampler(net, lat, condition=c, unconditional_condition=uc, num_steps=6, sigma_min=net.sigma_min,
                                          sigma_max=net.sigma_max, schedule_type='discrete', schedule_rho=1, max_order=2, predict_x0=False,
                                          lower_order_final=True)
        t_s, t_d = [], []
        for rnd in range(calls + 2):
            for fn, acc in ((sample, t_s), (lambda: dec.raw(sample()), t_d)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if rnd >= 2:
                    acc.append(e0.elapsed_time(e1))
        say(f'sampler only      {fmt(t_s)}  {B / statistics.median(t_s) * 1e3:7.2f} latents/s')
        say(f'sampler + decode  {fmt(t_d)}  {B / statistics.median(t_d) * 1e3:7.2f} images/s')
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
