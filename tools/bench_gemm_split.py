#!/usr/bin/env python
"""Time dsm_gemm_split (the fp16x3 Linear of the CLIP score, csrc/metrics/gemm_split.hip) against the fp32 launch of the same shape: the
ds_conv2d_nhwc (taps = 1) that the towers' plan Builder emits, plus the separate dsm_gelu_rows pass for fc1, whose GELU the split kernel
carries in its epilogue.  The four projection shapes of a ViT-g-14 layer of each tower at batch 64 (16 448 and 4 928 rows).

    python tools/bench_gemm_split.py [CALLS = 7] [OUT = profiles/clip_score_fp16x3_shapes.txt]

One process, the two launches alternating, two warm-up rounds, an event pair around every call; median with min and max.  "ranges apart":
the slowest fp16x3 call was faster than the fastest fp32 call.  No GPU: the tool fails."""
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diff_sampler_amd import _lib, _metrics_lib  # noqa: E402
from diff_sampler_amd.ops import pack_linear_weight, pack_linear_weight_split  # noqa: E402
from diff_sampler_amd.plan import Builder, ptr  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 7
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, 'profiles', 'clip_score_fp16x3_shapes.txt')
lines = []


def say(s=''):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    lib, mlib = _lib.load(), _metrics_lib.load()
    pr = torch.cuda.get_device_properties(0)
    say(f'# dsm_gemm_split vs the fp32 launch of the same shape on {pr.gcnArchName} / {pr.multi_processor_count} CUs; ViT-g-14 projections at batch 64; '
        f'one process, alternating, 2 warm-up rounds, median (min .. max) of {N} event-timed calls, ms')
    g = torch.Generator().manual_seed(0)
    st = _lib.stream_ptr()
    for tower, rows, W, Fn in (('image', 64 * 257, 1408, 6144), ('text', 64 * 77, 1024, 4096)):
        for name, k, cout, res, gelu in (('qkv', W, 3 * W, False, False), ('out_proj', W, W, True, False), ('fc1', W, Fn, False, True), ('fc2', Fn, W, True, False)):
            x = torch.randn(rows, k, generator=g).cuda()
            w = torch.randn(cout, k, generator=g) * 0.03
            bias = torch.randn(cout, generator=g).cuda()
            r = torch.randn(rows, cout, generator=g).cuda() if res else None
            w32 = pack_linear_weight(w).cuda()
            ws, shift = pack_linear_weight_split(w)
            ws = ws.cuda()
            o32, o16 = torch.empty(rows, cout, device='cuda'), torch.empty(rows, cout, device='cuda')
            bd = Builder(torch.device('cuda'), conv_mode=0, autotune=False, batch=64)
            bd.linear(x, k, rows, w32, cout, o32, name, bias=bias, **(dict(res=r, res_ld=cout) if res else {}))
            if gelu:
                bd.add(mlib.dsm_gelu_rows, (ptr(o32), cout, ptr(o32), cout, rows, cout), name + '.gelu')
            P = bd.finish()
            a = _metrics_lib.DsmGemmSplitArgs(ptr(x), k, rows, k, ptr(ws), shift, cout, ptr(bias), ptr(r), cout if res else 0, 1 if gelu else 0, ptr(o16), cout)

            def f32():
                for op in P.ops:
                    rc = op.fn(*op.args, st)
                    assert rc == 0, (op.name, rc)

            def f16():
                rc = mlib.dsm_gemm_split(C.byref(a), st)
                assert rc == 0, rc

            acc = {'fp32': [], 'fp16x3': []}
            for i in range(2 + N):
                for key, fn in (('fp32', f32), ('fp16x3', f16)):
                    ms = timed(fn)
                    if i >= 2:
                        acc[key].append(ms)
            torch.cuda.synchronize()
            err = float((o16 - o32).abs().max() / o32.abs().max())
            fl = 2.0 * rows * k * cout
            m32, m16 = statistics.median(acc['fp32']), statistics.median(acc['fp16x3'])
            apart = max(acc['fp16x3']) < min(acc['fp32'])
            say(f'{tower:5s} {name:8s} {rows:6d} x {k:5d} -> {cout:5d}  fp32 {m32:7.3f} ({min(acc["fp32"]):.3f} .. {max(acc["fp32"]):.3f}) {fl / m32 / 1e9:6.1f} TF/s   '
                f'fp16x3 {m16:7.3f} ({min(acc["fp16x3"]):.3f} .. {max(acc["fp16x3"]):.3f}) {fl / m16 / 1e9:6.1f} TF/s   fp32 / fp16x3 {m32 / m16:5.2f}  '
                f'ranges {"apart" if apart else "OVERLAP"}  max |difference| / absmax {err:.1e}')
            del x, w32, ws, o32, o16, r, P, bd
    os.makedirs(os.path.dirname(out_path) or '.', exist_ok=True)
    with open(out_path, 'w') as fh:
        fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
