#!/usr/bin/env python
"""Time the device resize and crop of the CLIP score (csrc/metrics/image_prep.hip) on the GPU, next to the host transform it replaces.

    python tools/time_clip_preprocess.py [--batch 64] [--source 512] [--calls 5] [--burst 50] [--config vit_g_14] [--images 256] [--session NAME] [--out FILE]

1. ``clip_score.preprocess`` (PIL, one thread) per image, PNG decoding not included.
2. The device path per image at `--batch`: the host-to-device copy of the decoded batch plus the kernel (what ``resize_center_crop``
   does with a host tensor), and the kernel alone on a batch already on the device; event pairs, median of `--calls` after two warm-up calls.
   The outputs are compared with the host transform's before anything is timed.
3. The kernel's rate: the bytes it has to move -- the source once and the output once, from the shapes -- over the kernel time, taken
   from `--burst` launches back to back (a single call's event pair also holds the host's preparation of the launch).
4. ``calc_clip_score`` on a folder of `--images` PNGs of `--source` x `--source` with seed weights of `--config`, with and without
   ``device_resize``, alternated, two rounds; wall clock around a call that ends in a synchronise; captions are token ids.
No GPU: the tool fails.
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(ms):
    return f'{statistics.median(ms):8.3f} ms (min {min(ms):.3f} max {max(ms):.3f}, n={len(ms)})'


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--source', type=int, default=512)
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--burst', type=int, default=50)
    ap.add_argument('--config', default='vit_g_14')
    ap.add_argument('--images', type=int, default=256, help='images of the end-to-end run; 0 skips it')
    ap.add_argument('--session', default='')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'tools/time_clip_preprocess.py measures on the GPU only'
    import PIL.Image
    from diff_sampler_amd import clip_score as CS, clip_score_arch as A
    from diff_sampler_amd.clip_preprocess import resize_center_crop

    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    pr = torch.cuda.get_device_properties(0)
    spec = A.named_spec(args.config)
    B, S, size = args.batch, args.source, spec.image_size
    say(f'# tools/time_clip_preprocess.py on {pr.gcnArchName} / {pr.multi_processor_count} CUs, session {args.session or "-"}: '
        f'{S} x {S} -> {size}, batch {B}; median of {args.calls} timed calls after 2 warm-up calls')
    rng = np.random.default_rng(0)
    batch = torch.from_numpy(rng.integers(0, 256, (B, S, S, 3), dtype=np.uint8))

    # 1. the host transform
    pil = [PIL.Image.fromarray(a) for a in batch[:16].numpy()]
    want = torch.stack([CS.preprocess(im, size) for im in pil])
    host = []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        for im in pil:
            CS.preprocess(im, size)
        host.append((time.perf_counter() - t0) * 1e3 / len(pil))
    host_ms = statistics.median(host)
    say(f'host preprocess (PIL, one thread, per image)        {med(host)}')

    # 2. the device path
    on_dev = batch.cuda()
    got = resize_center_crop(on_dev, size)
    torch.cuda.synchronize()
    assert torch.equal(got[:16].cpu(), want), 'the device resize differs from the host transform'
    say(f'device output equals the host transform on {len(want)} images: True')
    pinned, dst = batch.pin_memory(), torch.empty_like(on_dev)
    paths = {'copy + kernel (pageable host batch)': lambda: resize_center_crop(batch, size),
             'copy + kernel (pinned host batch)': lambda: resize_center_crop(dst.copy_(pinned, non_blocking=True), size),
             'kernel (batch on the device)': lambda: resize_center_crop(on_dev, size)}
    acc = {k: [] for k in paths}
    for r in range(2 + args.calls):
        for k, fn in paths.items():
            ms = timed(fn)
            if r >= 2:
                acc[k].append(ms)
    for k in paths:
        say(f'{k:40s} per batch {med(acc[k])}   per image {statistics.median(acc[k]) / B:.4f} ms   host / device {host_ms / (statistics.median(acc[k]) / B):.1f}')

    # 3. the kernel's rate: one call leaves the device idle while the host prepares the launch, so the kernel time is that of `--burst`
    #    launches through the C ABI back to back between one pair of events, over their number
    import ctypes as C
    from diff_sampler_amd import _lib, _metrics_lib
    from diff_sampler_amd.clip_preprocess import device_tables
    nh, nw, top, left, (hb, hc, hk, vb, vc, vk) = device_tables(S, S, size, on_dev.device)
    p = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)
    out = torch.empty(B, 3, size, size, dtype=torch.uint8, device='cuda')
    cargs = (p(on_dev), on_dev.stride(0), on_dev.stride(1), B, S, S, nh, nw, top, left, size, p(hb), p(hc), hk, p(vb), p(vc), vk, p(out), _lib.stream_ptr())
    fn = _metrics_lib.load().dsm_resize_crop_u8

    def burst():
        for _ in range(args.burst):
            assert fn(*cargs) == 0

    kern = [timed(burst) / args.burst for _ in range(2 + args.calls)][2:]
    assert torch.equal(out, got)
    say(f'kernel ({args.burst} launches back to back, per launch)   {med(kern)}')
    kernel_ms = statistics.median(kern)
    nbytes = B * (S * S * 3 + 3 * size * size)
    say(f'kernel: {nbytes / 1e6:.1f} MB (source once + output) in {kernel_ms:.3f} ms = {nbytes / kernel_ms / 1e6:.1f} GB/s = '
        f'{nbytes / kernel_ms / 1e6 / 8000:.1%} of the 8 TB/s HBM peak')

    # 4. end to end
    if args.images:
        with tempfile.TemporaryDirectory() as tmp:
            d = os.path.join(tmp, 'images')
            os.makedirs(d)
            for i in range(args.images):
                PIL.Image.fromarray(np.roll(batch[i % B].numpy(), i // B, axis=0), 'RGB').save(os.path.join(d, f'{i:06d}.png'), compress_level=1)
            g = torch.Generator().manual_seed(2)
            tokens = torch.randint(1, spec.vocab - 2, (args.images, spec.positions), generator=g)
            tokens[:, 0], tokens[:, 20], tokens[:, 21:] = spec.vocab - 2, spec.vocab - 1, 0
            captions = tokens.tolist()
            scorer = CS.ClipScorer(spec, A.init_clip_score_params(spec, 0))
            res, wall = {}, {False: [], True: []}
            for r in range(3):                                  # round 0 warms both paths up
                for flag in (False, True):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    res[flag] = CS.calc_clip_score(scorer, d, captions, max_batch_size=B, log=lambda *a: None, device_resize=flag)
                    torch.cuda.synchronize()
                    if r:
                        wall[flag].append(time.perf_counter() - t0)
            say(f'calc_clip_score, {args.config} seed weights, {args.images} PNGs of {S} x {S}, batch {B} (PNG decoding included): scores equal {res[False] == res[True]}')
            for flag in (False, True):
                t = min(wall[flag])
                say(f'  device_resize={flag!s:5s} {t:7.3f} s (best of {len(wall[flag])}: {", ".join(f"{x:.3f}" for x in wall[flag])})   {args.images / t:7.1f} pairs/s')
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
