#!/usr/bin/env python
"""Time the CLIP scorer on the GPU: both towers and the whole ``ClipScorer.score`` call at the full ViT-g-14 geometry with seed weights,
next to the plain-torch restatement of the same towers (tests/_clip_vit_ref.py) in stock PyTorch-ROCm fp32 on the same GPU in the same
process.

    python tools/time_clip_score.py [--config vit_g_14] [--batch 64] [--calls 5] [--session NAME] [--out profiles/clip_score_timing.txt] [--dtype fp32|fp16x3]

Every timing is a pair of events around ONE call on the current stream, after warm-up calls of every variant; engine and stock calls
alternate; median with min / max.  The per-launch table is one replay of each tower's plan with an event pair per launch, grouped by
launch kind.  The host preprocessing (PIL: 512 x 512 RGB -> uint8 224 x 224, the reference's own path) is timed on the host per image and
reported as a share of host + device time per image -- it is not part of the device numbers.  No GPU: the tool fails.
``--dtype fp16x3`` times the engine in that mode (ClipScorer(dtype='fp16x3')) and, alternating in the same rounds, the fp32 engine too.
"""
import argparse
import collections
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def fmt(ms):
    return f'{statistics.median(ms):9.2f} ms (min {min(ms):.2f} max {max(ms):.2f}, n={len(ms)})'


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def alternate(fns, calls, warm=2):
    acc = {k: [] for k in fns}
    for r in range(warm + calls):
        for k, fn in fns.items():
            ms = timed(fn)
            if r >= warm:
                acc[k].append(ms)
    return acc


def launch_table(plan, say, top=12):
    from diff_sampler_amd import _lib
    st = _lib.stream_ptr()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in plan.ops]
    for (e0, e1), op in zip(ev, plan.ops):
        e0.record()
        rc = op.fn(*op.args, st)
        e1.record()
        assert rc == 0, op.name
    torch.cuda.synchronize()
    groups = collections.OrderedDict()
    for (e0, e1), op in zip(ev, plan.ops):
        g = groups.setdefault(op.name.split('.')[-1], [0, 0.0])
        g[0] += 1
        g[1] += e0.elapsed_time(e1)
    total = sum(g[1] for g in groups.values())
    say(f'  {len(plan.ops)} launches, sum of event pairs {total:.2f} ms')
    say(f'  {"launch":22s} {"n":>4s} {"ms each":>9s} {"ms all":>9s} {"share":>6s}')
    for name, (n, ms) in sorted(groups.items(), key=lambda kv: -kv[1][1])[:top]:
        say(f'  {name:22s} {n:4d} {ms / n:9.3f} {ms:9.2f} {ms / total:6.3f}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='vit_g_14')
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--calls', type=int, default=5)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--session', default='')
    ap.add_argument('--out', default='')
    ap.add_argument('--dtype', default='fp32', choices=['fp32', 'fp16x3'])
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'tools/time_clip_score.py measures on the GPU only'
    import _clip_vit_ref as R
    from diff_sampler_amd import clip_score_arch as A
    from diff_sampler_amd.clip_score import ClipScorer, preprocess

    lines = []

    def say(s=''):
        print(s, flush=True)
        lines.append(s)

    pr = torch.cuda.get_device_properties(0)
    spec = A.named_spec(args.config)
    B = args.batch
    say(f'# tools/time_clip_score.py on {pr.gcnArchName} / {pr.multi_processor_count} CUs, session {args.session or "-"}: {args.config}, seed weights, '
        f'batch {B}, engine dtype {args.dtype} (stock: fp32); median of {args.calls} timed calls after 2 warm-up rounds, engine and stock calls alternated')
    params = A.init_clip_score_params(spec, args.seed)
    scorer = ClipScorer(spec, params, dtype=args.dtype)
    scorer32 = ClipScorer(spec, params) if args.dtype != 'fp32' else None
    dev = {k: v.cuda() for k, v in params.items()}
    images = R.seed_images(1, B, spec.image_size)
    g = torch.Generator().manual_seed(2)
    tokens = torch.randint(1, spec.vocab - 2, (B, spec.positions), generator=g)
    tokens[:, 0], tokens[:, 20], tokens[:, 21:] = spec.vocab - 2, spec.vocab - 1, 0
    images_d, tokens_d = images.cuda(), tokens.cuda()
    V, T = spec.vision, spec.text
    out = {}

    def stock_image():
        with torch.no_grad():
            out['si'] = R.clip_image_ref(dev, images_d, V.heads, V.layers, spec.eps, spec.act)[0]

    def stock_text():
        with torch.no_grad():
            out['st'] = R.clip_text_pooled_ref(dev, tokens_d, T.heads, T.layers, spec.eps, spec.act)[0]

    def stock_score():
        stock_image()
        stock_text()
        a, b = out['si'], out['st']
        out['ss'] = 100 * ((a / a.norm(dim=-1, keepdim=True)) * (b / b.norm(dim=-1, keepdim=True))).sum(-1)

    def engine_image():
        out['ei'] = scorer.image.raw(images_d)[0]

    def engine_text():
        out['et'] = scorer.text.raw(tokens)[0]

    def engine_score():
        out['es'] = scorer.score(images_d, tokens)

    fns = {'engine image': engine_image, 'stock image': stock_image, 'engine text': engine_text, 'stock text': stock_text,
           'engine scorer': engine_score, 'stock scorer': stock_score}
    if scorer32 is not None:
        fns['engine-fp32 image'] = lambda: scorer32.image.raw(images_d)
        fns['engine-fp32 text'] = lambda: scorer32.text.raw(tokens)
    acc = alternate(fns, args.calls)
    torch.cuda.synchronize()
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())
    say(f'agreement engine vs stock (max |a - b| / max |b|): image features {rel(out["ei"], out["si"]):.2e}, text features '
        f'{rel(out["et"], out["st"]):.2e}, scores max |difference| {float((out["es"] - out["ss"]).abs().max()):.2e}')
    fi, ft = A.clip_score_flops(spec)
    say()
    for what, unit, fl in (('image', 'images/s', fi), ('text', 'prompts/s', ft), ('scorer', 'pairs/s', fi + ft)):
        me, ms_ = statistics.median(acc[f'engine {what}']), statistics.median(acc[f'stock {what}'])
        say(f'{what:7s} engine {fmt(acc["engine " + what])}  {B / me * 1e3:9.1f} {unit}  {fl * B / me / 1e9:7.1f} TFLOP/s (algorithmic)')
        say(f'{what:7s} stock  {fmt(acc["stock " + what])}  {B / ms_ * 1e3:9.1f} {unit}  {fl * B / ms_ / 1e9:7.1f} TFLOP/s   engine / stock time {me / ms_:.3f}')
    if scorer32 is not None:
        for what in ('image', 'text'):
            me, m32 = statistics.median(acc[f'engine {what}']), statistics.median(acc[f'engine-fp32 {what}'])
            say(f'{what:7s} engine fp32 mode {fmt(acc["engine-fp32 " + what])}   {args.dtype} / fp32 time {me / m32:.3f}')
    say()
    say('per-launch, image tower (one replay, an event pair per launch):')
    launch_table(scorer.image.plan(B), say)
    say('per-launch, text tower:')
    launch_table(scorer.text.plan(B), say)

    # host preprocessing: the reference's own path (PIL per image), 512 x 512 inputs as the sampler writes them
    import PIL.Image
    src = [PIL.Image.fromarray(x.permute(1, 2, 0).numpy(), 'RGB') for x in R.seed_images(3, 16, 512)]
    preprocess(src[0], spec.image_size)
    t0 = time.perf_counter()
    for im in src:
        preprocess(im, spec.image_size)
    host_ms = (time.perf_counter() - t0) * 1e3 / len(src)
    dev_ms = statistics.median(acc['engine scorer']) / B
    say()
    say(f'host preprocessing (PIL, 512 x 512 -> {spec.image_size}, one thread, PNG decoding not included): {host_ms:.2f} ms per image = '
        f'{host_ms / (host_ms + dev_ms):.1%} of host + device time per pair ({dev_ms:.2f} ms per pair on the device)')
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
