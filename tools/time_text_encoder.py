#!/usr/bin/env python
"""Time the CLIP text encoder and its causal attention kernel on the GPU -> profiles/text_encoder_timing.txt.

    python tools/time_text_encoder.py [--out FILE] [--quick]

1. One encode of the sd15 encoder at B = 1, 16 and 17 (16 prompts plus ""): the engine's plan eager (ds_plan_run) and replayed from its
   hipGraph, and the same math through stock PyTorch (tests/_clip_ref.py on the GPU, fp32, TF32 off) -- the three alternate inside one process.
   FLOPs = clip_arch.clip_flops_per_prompt; the fraction is of the fp32 matrix peak.
2. ds_attention_causal alone on the encoder's shape (12 heads of 64 over 77 tokens, packed q|k|v) against ds_attention WITHOUT a mask on the
   same operands and against the masked softmax attention of stock PyTorch.
3. (not with --quick) SD-1.5 DPM-Solver++(2M) NFE = 10 at B = 16 in fp16 mode: the sampler call alone, and what encoding 16 prompts + "" adds.
4. The per-kernel split of the B = 17 encode: this script re-run as a fresh child process under `rocprofv3 --kernel-trace --stats` (--child).
Warm-up calls first; every timing is a pair of events around ONE call on the current stream; median with min / max."""
import argparse
import ctypes as C
import glob
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

FP32_MATRIX_PEAK_TFLOPS = 157.3      # MI355X dense fp32 matrix rate (v_mfma_f32_32x32x2_f32)


def fmt(ms):
    return f'{statistics.median(ms):8.3f} ms (min {min(ms):.3f} max {max(ms):.3f}, n={len(ms)})'


def alternate(fns, calls, warm=2):
    """{name: [ms]}: the callables take turns, `warm` untimed rounds first."""
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


def tokens_for(B, vocab, seed=0):
    t = torch.randint(0, vocab, (B, 77), generator=torch.Generator().manual_seed(seed))
    t[-1, 1:] = vocab - 1            # the last row is the empty prompt's shape: start token, then padding
    return t


def child():
    """What the profiler traces: five B = 17 encodes (the first builds the plan)."""
    from diff_sampler_amd.clip_engine import ClipTextEncoder
    enc = ClipTextEncoder.from_config('sd15', seed=0)
    t = tokens_for(17, enc.spec.vocab)
    for _ in range(5):
        enc.raw(t)
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'text_encoder_timing.txt'))
    ap.add_argument('--quick', action='store_true', help='fewer calls, no sampler section')
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--no-profile', action='store_true', help='skip the rocprofv3 child run')
    args = ap.parse_args()
    if args.child:
        return child()
    from _clip_ref import clip_text_ref
    from diff_sampler_amd import _lib, clip_arch, solvers
    from diff_sampler_amd.clip_engine import ClipTextEncoder
    lib = _lib.load()
    torch.backends.cuda.matmul.allow_tf32 = False
    calls = 7 if args.quick else 15
    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    pr = torch.cuda.get_device_properties(0)
    say(f'# tools/time_text_encoder.py on {pr.gcnArchName} / {pr.multi_processor_count} CUs; median of {calls} timed calls after 2 warm-up rounds, variants alternated')
    enc = ClipTextEncoder.from_config('sd15', seed=0)
    spec = enc.spec
    params = {k: v.cuda() for k, v in clip_arch.init_clip_params(spec, seed=0).items()}
    say(f'# encoder FLOPs per prompt (2 x MAC, attention unmasked): {enc.flops(1) / 1e9:.3f} GFLOP; fp32 matrix peak taken as {FP32_MATRIX_PEAK_TFLOPS} TFLOP/s')
    say()
    say('## 1. one encode: engine plan eager / hipGraph replay / stock PyTorch (tests/_clip_ref.py on the GPU, fp32)')
    st = _lib.stream_ptr()
    for B in (1, 16, 17):
        tok = tokens_for(B, spec.vocab)
        out, plan = enc.raw(tok)
        with torch.no_grad():
            ref = clip_text_ref(params, tok.cuda(), spec.heads, spec.layers, spec.eps)
        dist = float((out - ref).abs().max() / ref.abs().max())
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            sp = C.c_void_p(side.cuda_stream)
            plan.graph_capture(sp)
            side.synchronize()
        tok_d = tok.cuda()

        def stock():
            with torch.no_grad():
                clip_text_ref(params, tok_d, spec.heads, spec.layers, spec.eps)
        with torch.cuda.stream(side):            # everything on the captured plan's stream: the events see all three
            acc = alternate({'eager': lambda: plan.run(sp), 'graph': lambda: plan.graph_launch(sp), 'stock': stock}, calls)
            side.synchronize()
        g_ms = acc['graph']
        fl = enc.flops(B)
        me, mg, ms_ = (statistics.median(v) for v in (acc['eager'], g_ms, acc['stock']))
        say(f'B={B:2d} eager {fmt(acc["eager"])} {me / B:7.3f} ms/prompt {fl / me / 1e9:6.1f} TFLOP/s = {fl / me / 1e9 / FP32_MATRIX_PEAK_TFLOPS:.3f} of peak')
        say(f'     graph {fmt(g_ms)} {fl / mg / 1e9:6.1f} TFLOP/s = {fl / mg / 1e9 / FP32_MATRIX_PEAK_TFLOPS:.3f} of peak')
        say(f'     stock {fmt(acc["stock"])} {fl / ms_ / 1e9:6.1f} TFLOP/s | stock / eager {ms_ / me:5.2f}x  stock / graph {ms_ / mg:5.2f}x | engine vs stock output: {dist:.2e} of absmax')
    say()
    say('## 2. causal attention alone, batch 17 x 12 heads x 77 tokens x 64, packed q|k|v [rows][2304]')
    B, H, S, D, W = 17, spec.heads, 77, 64, spec.width
    qkv = torch.randn(B * S, 3 * W, device='cuda')
    o = torch.empty(B * S, W, device='cuda')
    a = _lib.AttnArgs(qkv.data_ptr(), qkv[:, W:].data_ptr(), qkv[:, 2 * W:].data_ptr(), o.data_ptr(), 3 * W, 3 * W, 3 * W, W, S * 3 * W, S * 3 * W,
                      S * 3 * W, S * W, B, H, S, S, D, D ** -0.5)
    q4 = qkv.view(B, S, 3, H, D)
    mask = torch.full((S, S), float('-inf'), device='cuda').triu(1)

    def stock_attn():
        q, k, v = (q4[:, :, i].transpose(1, 2) for i in range(3))
        return (torch.softmax(q @ k.transpose(-1, -2) * D ** -0.5 + mask, -1) @ v).transpose(1, 2).reshape(B * S, W)

    def sdpa():
        q, k, v = (q4[:, :, i].transpose(1, 2) for i in range(3))
        return torch.nn.functional.scaled_dot_product_attention(q, k, v, is_causal=True)
    assert lib.ds_attention_causal(C.byref(a), st) == 0
    variants = {'ds_attention_causal': lambda: lib.ds_attention_causal(C.byref(a), st), 'ds_attention (no mask)': lambda: lib.ds_attention(C.byref(a), st),
                'stock masked softmax': stock_attn}
    try:
        sdpa()
        variants['stock sdpa is_causal'] = sdpa
    except Exception as e:          # this torch build has no fp32 kernel behind it: the plain formulation is the yardstick
        say(f'# torch scaled_dot_product_attention(is_causal) not available here ({type(e).__name__})')
    err = float((o - stock_attn()).abs().max())
    acc = alternate(variants, 3 * calls, warm=3)
    base = statistics.median(acc['ds_attention_causal'])
    fl = 4.0 * B * H * S * S * D
    for k, v in acc.items():
        m = statistics.median(v)
        say(f'{k:24s} {fmt(v)}  {fl / m / 1e9:6.2f} TFLOP/s (unmasked count)  {m / base:5.2f}x of the causal kernel')
    say(f'max |ds_attention_causal - stock| on these operands: {err:.2e}')
    del enc, plan, params
    torch.cuda.empty_cache()
    if not args.quick:
        say()
        say('## 3. SD-1.5 fp16, DPM-Solver++(2M) NFE = 10, B = 16 (random init): the sampler call, and encoding 16 prompts + "" in front of it')
        from diff_sampler_amd.ldm_engine import CFGDenoiser
        net = CFGDenoiser.from_config('sd15', seed=0, guidance_rate=7.5, use_fp16=True)
        enc = ClipTextEncoder.from_config('sd15', seed=0)
        lat = torch.randn(16, 4, 64, 64, device='cuda')
        tok = tokens_for(17, spec.vocab)

        def sample(c, uc):
            return solvers.dpm_pp_sampler(net, lat, condition=c, unconditional_condition=uc, num_steps=6, sigma_min=net.sigma_min,
                                          sigma_max=net.sigma_max, schedule_type='discrete', schedule_rho=1, max_order=2, predict_x0=False,
                                          lower_order_final=True)
        c0, uc0 = torch.randn(16, 77, 768, device='cuda'), torch.randn(16, 77, 768, device='cuda')

        def with_encode():
            s = enc(tok)
            return sample(s[:16], s[16:].expand(16, -1, -1))
        acc = alternate({'sampler': lambda: sample(c0, uc0), 'encode + sampler': with_encode, 'encode': lambda: enc(tok)}, 5, warm=2)
        ms_s, ms_e = statistics.median(acc['sampler']), statistics.median(acc['encode'])
        for k, v in acc.items():
            say(f'{k:18s} {fmt(v)}')
        say(f'encode (host upload of the ids, plan run, copy of the result) / sampler call = {ms_e / ms_s * 100:.2f} %')
        del net, enc
        torch.cuda.empty_cache()
    if not args.no_profile:
        say()
        say('## 4. per-kernel split of the B = 17 encode (rocprofv3 --kernel-trace --stats; five encodes in a child process of their own)')
        import tempfile
        d = tempfile.mkdtemp(prefix='te_prof_')          # the trace database is read below and not kept
        r = subprocess.run(['rocprofv3', '--kernel-trace', '--stats', '-d', d, '-o', 'te', '--', sys.executable, os.path.abspath(__file__), '--child'],
                           capture_output=True, text=True, timeout=400)
        dbs = sorted(glob.glob(os.path.join(d, '**', '*.db'), recursive=True), key=os.path.getmtime)
        if r.returncode or not dbs:
            say(f'rocprofv3 run failed (rc {r.returncode}): {r.stderr[-300:]}')
        else:
            import sqlite3
            rows = list(sqlite3.connect(dbs[-1]).cursor().execute('select name, total_calls, total_duration, average, percentage from top_kernels'))
            tot = sum(r_[2] for r_ in rows)
            say(f'{"kernel":84s} {"calls":>6s} {"total_us":>10s} {"avg_us":>9s} {"pct":>6s}')
            for n, c_, t, av, p in rows:
                n = n.replace('(anonymous namespace)::', '')
                say(f'{(n if len(n) < 84 else n[:81] + "..."):84s} {c_:6d} {t:10.1f} {av:9.2f} {p:6.2f}')
            say(f'kernel time per encode: {tot / 5 / 1e3:.3f} ms (sum over the five encodes / 5; durations in microseconds as tools/rocprof_summary.py prints them)')
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
