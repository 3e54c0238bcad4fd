#!/usr/bin/env python
"""Reduce launch plans to an address-independent form and compare two trees' plans row by row (CPU only: plans are host logic).

One row per launch, in execution order (the per-context sub-plan `P.ctx` first): launch name, entry point, every field of the argument
struct (for the by-value entry points: of the struct plan._native_plan builds), the nested `tune` included -- with every pointer replaced
by WHAT it points at:

    weight                                  ('w', key in engine.w | 'fp16 packing of <key>', byte offset)
    tensor no launch has written so far     ('buf', P.bufs key(s), byte offset)                      -- the plan's inputs
    tensor an earlier launch wrote          ('ws', index of the LAST launch that wrote into that plan-owned tensor,
                                             byte offset of that write, byte offset of this read)    -- offsets from the tensor's base
    a pointer the launch writes             ('out', P.bufs key(s) | 'ws', byte offset from the tensor's base)
    scratch nobody reads across launches    'null' / 'set'   (workspace, partial, counters; also ds_conv_args.update)

plus the library's own routing answers (ds_conv_route for ds_conv2d_nhwc, ds_attention_variant for ds_attention).  Moving a temporary
into a recycled buffer leaves this form unchanged; reading a tensor that something else has overwritten in the meantime changes it.
A pointer that cannot be classified, or a read of a plan-owned tensor that nothing has written, is an error.

    python tools/plan_dump.py run --out A.json [--jobs 8] [--quick]      every plan of the matrix: per-row hashes, plan-owned bytes
    python tools/plan_dump.py compare A.json B.json                      row-by-row comparison of two runs (exit status 1 on a difference)
    python tools/plan_dump.py show 'edm/cifar10/fp32/-/B=4/rows=1'       the full rows of one plan
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import torch  # noqa: E402

from diff_sampler_amd import _lib, _metrics_lib  # noqa: E402

WRITES = {'ds_conv2d_nhwc': ('out', 'stats_out'), 'ds_norm_act': ('out', 'raw_out'), 'ds_gn_stats': ('mean', 'rstd', 'coefs'),
          'ds_gn_finalize': ('mean', 'rstd', 'coefs'), 'ds_attention': ('out',), 'ds_attention_f16': ('out',), 'ds_gemm_nt_batched': ('c',),
          'ds_layernorm_rows': ('y',), 'ds_layernorm_rows_f16': ('y',), 'ds_layernorm_rows_f16io': ('y',), 'ds_geglu': ('y',),
          'ds_noise_embed': ('out',), 'ds_stem_im2col': ('out',), 'dsm_fir_resample': ('out',), 'dsm_zero_border': ('out',),
          'affine_compose': ('aff',)}         # (in place: _lib.affine_compose, the DS_OP_AFFINE_COMPOSE launch of the step-conditioned ADM plans)
SCRATCH = ('workspace', 'partial', 'counters', 'update')
BY_VALUE = {'ds_layernorm_rows': _lib.LayerNormArgs, 'ds_layernorm_rows_f16': _lib.LayerNormArgs, 'ds_layernorm_rows_f16io': _lib.LayerNormArgs,
            'ds_geglu': _lib.GegluArgs, 'ds_noise_embed': _lib.NoiseEmbedArgs, 'ds_stem_im2col': _lib.StemIm2colArgs,
            'dsm_zero_border': _metrics_lib.DsmZeroBorderArgs}        # (libdsmetrics launches of the NCSN++ plans)


class DumpError(AssertionError):
    pass


def _tensors(v):
    if isinstance(v, torch.Tensor):
        yield v
    elif isinstance(v, (tuple, list)):
        for x in v:
            yield from _tensors(x)


def _span(t):
    s = t.untyped_storage()
    return s.data_ptr(), s.data_ptr() + s.nbytes()


def _find(spans, p):
    return [s for s in spans if s[0] <= p < s[1]]


def dump(engine, P):
    """The rows of plan P of `engine`: [(row, {dead word: value})], a row being JSON-able values."""
    lib = _lib.load()
    weights = []                                    # (start, end, label)
    for k, v in engine.w.items():
        weights += [(*_span(t), str(k)) for t in _tensors(v)]
    for packed, src in engine._w16_cache.values():
        of = [lab for a, b, lab in weights if a <= src.data_ptr() < b]
        weights.append((*_span(packed), 'fp16 packing of ' + (of[0] if of else '?')))
    bufs = [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), str(k)) for k, t in P.bufs.items() if isinstance(t, torch.Tensor)]
    owned = {}                                      # storage start -> [start, end, last write (launch, offset) or None]
    for t in list(P.keep) + [t for t in P.bufs.values() if isinstance(t, torch.Tensor)]:
        a, b = _span(t)
        owned.setdefault(a, [a, b, None])

    def keys_at(p):
        return '|'.join(sorted(lab for a, b, lab in bufs if a <= p < b))

    def read(p, what):
        own = _find(owned.values(), p)
        if own and own[0][2] is not None:
            return ['ws', own[0][2][0], own[0][2][1], p - own[0][0]]
        if keys_at(p):
            return ['buf', keys_at(p), p - own[0][0]]
        hit = _find(weights, p)
        if hit:
            return ['w', hit[0][2], p - hit[0][0]]
        raise DumpError(f'{what}: ' + ('reads a plan-owned tensor that nothing has written' if own else 'unclassified pointer'))

    ctx = getattr(P, 'ctx', None)
    ops = (list(ctx.ops) if ctx is not None else []) + list(P.ops)
    rows = []
    for i, op in enumerate(ops):
        fn = op.fn.__name__
        st = BY_VALUE[fn](*op.args) if fn in BY_VALUE else op.keep[0]
        row, written = [op.name, fn], []

        def fields(s, prefix=''):
            for f, ty in s._fields_:
                v = getattr(s, f)
                what = f'{op.name} ({fn}).{prefix}{f}'
                if isinstance(v, C.Structure):
                    fields(v, f + '.')
                elif ty is not C.c_void_p:
                    row.append([prefix + f, repr(list(v) if isinstance(v, C.Array) else v)])
                elif f in SCRATCH:
                    row.append([f, 'set' if v else 'null'])
                elif not v:
                    row.append([f, 'null'])
                elif f in WRITES[fn]:
                    own = _find(owned.values(), v)
                    if not own:
                        raise DumpError(f'{what}: writes through an unclassified pointer')
                    row.append([f, ['out', keys_at(v) or 'ws', v - own[0][0]]])
                    written.append((own[0], v - own[0][0]))
                else:
                    row.append([f, read(v, what)])
        fields(st)
        for own, off in written:            # after the reads: a launch may read the tensor it overwrites
            own[2] = (i, off)
        if fn == 'ds_conv2d_nhwc':
            r = _lib.ConvRouteInfo()
            rc = lib.ds_conv_route(C.byref(st), C.byref(r))
            # ds_conv_args.wino is a property on the struct's tail padding, not in _fields_: recorded here, with the route's own wino word,
            # where either is set -- a launch that changes form changes its row, rows of the direct form keep the hashes tests have recorded
            wino = [['wino', repr(st.wino)]] if st.wino else []
            row += wino + [['route', [rc, r.kernel_id, r.splits, list(r.f16_widths[:r.f16_groups])] + ([r.wino] if r.wino else [])]]
        dead = {}                           # words no kernel reads: kept out of the row's hash, compared on their own
        if fn == 'ds_attention':            # the library's answer decides (it is 2 for d >= 512 whatever the raw word says)
            row.append(['library_variant', lib.ds_attention_variant(C.byref(st))])
            dead['variant'] = st.variant
        if fn == 'ds_norm_act' and not st.raw_out:          # the pitch of a raw copy that is not written
            dead['raw_ld'] = st.raw_ld
        rows.append((row, dead))
    return rows


def row_record(row, dead):
    """'name:hash[:dead words]' -- the hash leaves the dead words out, so that compare can tell a row that differs ONLY in one of them
    (the library's routing answer, inside the hash, unchanged) from any other difference."""
    body = [x for x in row if not (isinstance(x, list) and x[0] in dead)]
    h = hashlib.sha256(json.dumps(body).encode()).hexdigest()[:16]
    return f'{row[0]}:{h}' + (':' + ','.join(f'{k}={v}' for k, v in dead.items()) if dead else '')


# ---- the matrix -------------------------------------------------------------------------------------------------------------------------
INV_BATCHES = (1, 2, 3, 4, 5, 8, 16)
MODES = {'fp32': {}, 'fp16': dict(use_fp16=True), 'split': dict(split_fp16=True)}


def extra_configs():
    """Geometries outside the named configurations: images wider than 64 pixels in both denoisers (the fp16-activation kernels of their
    layers end at 64 pixels) and decoders on other latent sizes (12: no power of two; 24 at reduced width)."""
    import diff_sampler_amd.arch as arch
    import diff_sampler_amd.ldm_arch as la
    import diff_sampler_amd.vae_arch as va
    return {'song128': dict(arch.NAMED_CONFIGS['tiny_song'], img_resolution=128, model_channels=64, channel_mult=[1, 2]),
            'adm128': dict(arch.NAMED_CONFIGS['tiny_adm'], img_resolution=128),
            'ldm128': dict(la.NAMED_LDM_CONFIGS['tiny_ldm'], img_resolution=128),
            'vae_lat12': dict(va.NAMED_VAE_CONFIGS['sd15'], latent_resolution=12),
            'vae_lat24': dict(va.NAMED_VAE_CONFIGS['tiny_vae'], ch=64, latent_resolution=24)}


def make_engine(kind, net, mode):
    kw = MODES[mode]
    extra = extra_configs()
    if kind == 'edm':
        import diff_sampler_amd.arch as arch
        from diff_sampler_amd.engine import UNetEngine
        spec = arch.edm_precond_spec(**dict(extra.get(net) or arch.NAMED_CONFIGS[net]))
        return UNetEngine(spec, arch.init_params(spec, seed=1), device='cpu', **kw)
    if kind == 'ldm':
        import diff_sampler_amd.ldm_arch as la
        from diff_sampler_amd.ldm_engine import LDMUNetEngine
        spec = la.ldm_unet_spec(**dict(extra.get(net) or la.NAMED_LDM_CONFIGS[net]))
        return LDMUNetEngine(spec, la.init_ldm_params(spec, seed=1), device='cpu', **kw)
    import diff_sampler_amd.vae_arch as va
    from diff_sampler_amd.vae_engine import VAEDecoder
    spec = va.vae_decoder_spec(**dict(extra.get(net) or va.NAMED_VAE_CONFIGS[net]))
    return VAEDecoder(spec, va.init_vae_params(spec, seed=1), device='cpu', **kw)


def matrix(quick=False):
    """{(kind, net, mode): [(variant, batch)]}: variant = 'inv' / 'fuse0' / 'fuse1' / 'nodown' / 'qkv32' / 'fold' flags joined by '+', '-' = default."""
    import _routing
    import diff_sampler_amd.arch as arch
    import diff_sampler_amd.ldm_arch as la
    import diff_sampler_amd.vae_arch as va
    m = {}
    for cfg, (net, kind, kw, rng, bench) in _routing.CONFIGS.items():
        mode = 'fp16' if kw.get('use_fp16') else 'split' if kw.get('split_fp16') else 'fp32'
        jobs = m.setdefault((kind, net, mode), [])
        jobs += [('-', B) for B in (list(rng)[:6] + [bench] if quick else rng)]
        some = INV_BATCHES + (bench, bench + 1)
        jobs += [('inv', B) for B in some]
        if mode == 'fp16':
            jobs += [(v, B) for v in ('fuse0', 'fuse1', 'inv+fuse0', 'inv+fuse1') for B in some]
            if net in ('imagenet64', 'sd15'):
                jobs += [('fold', B) for B in (1, 4, bench)]
        if (net, mode) == ('sd15', 'fp16'):
            jobs += [(v, B) for v in ('nodown', 'qkv32') for B in (1, 2, 16)]          # U-Net batches N = 2, 4, 32
    for kind, named in (('edm', arch.NAMED_CONFIGS), ('ldm', la.NAMED_LDM_CONFIGS)):
        for net in named:
            ncsnpp = kind == 'edm' and arch.edm_precond_spec(**named[net]).ncsnpp       # exact fp32 only, no batch-invariant route
            for mode in (('fp32',) if ncsnpp else ('fp32', 'fp16', 'split') if kind == 'edm' else ('fp32', 'fp16')):
                if (kind, net, mode) not in m:
                    m[(kind, net, mode)] = [(v, B) for v in (('-',) if ncsnpp else ('-', 'inv')) for B in (1, 2, 3, 4, 5)]
    for net in va.NAMED_VAE_CONFIGS:
        for mode in ('fp32', 'fp16'):
            m[('vae', net, mode)] = [(v, B) for v in ('-', 'inv') for B in (1, 2, 3, 4, 16)]
    for kind, net in (('edm', 'song128'), ('edm', 'adm128'), ('ldm', 'ldm128'), ('vae', 'vae_lat12'), ('vae', 'vae_lat24')):
        for mode in ('fp32', 'fp16') + (('split',) if kind == 'edm' else ()):
            m[(kind, net, mode)] = [(v, B) for v in ('-', 'inv') for B in (1, 2, 3)]
    return m


def build_plans(eng, kind, variant, B):
    """[(rows suffix, plan)] of one matrix entry: both sigma forms for the denoisers."""
    from diff_sampler_amd import plan as plan_mod
    flags = set(variant.split('+'))
    eng.batch_invariant = 'inv' in flags
    if kind != 'vae':
        eng.fuse_norm16 = False if 'fuse0' in flags else True if 'fuse1' in flags else 'auto'
    if kind == 'ldm':
        eng.f16_downsample = 'nodown' not in flags
        eng.qkv_f16_min_head = 10 ** 9 if 'qkv32' in flags else 40
    plan_mod.FOLD_FINALIZE = 'fold' in flags
    try:
        if kind == 'vae':
            return [('', eng.plan(B))]
        n = 2 * B if kind == 'ldm' else B
        forms = (n,) if getattr(eng.spec, 'label_dim', 0) else tuple(dict.fromkeys((n, 1)))
        return [(f'/rows={r}', eng.plan(n, r, 77) if kind == 'ldm' else eng.plan(n, r)) for r in forms]
    finally:
        plan_mod.FOLD_FINALIZE = False


def run_task(task):
    (kind, net, mode), jobs = task
    torch.set_num_threads(1)
    eng = make_engine(kind, net, mode)
    out = {}
    for variant, B in jobs:
        eng._plans.clear()
        for suffix, P in build_plans(eng, kind, variant, B):
            rows = dump(eng, P)
            out[f'{kind}/{net}/{mode}/{variant}/B={B}{suffix}'] = dict(
                rows=[row_record(*r) for r in rows], links=sum(1 for r, _ in rows for x in r[2:] if isinstance(x[1], list) and x[1][0] == 'ws'),
                bytes=sum(t.numel() * t.element_size() for t in P.keep), tensors=len(P.keep))
            P.close()
    return out


def cmd_run(args):
    import multiprocessing as mp
    tasks = []
    for key, jobs in matrix(args.quick).items():
        if not '/'.join(key).startswith(args.only):
            continue
        step = 10 if key[1] == 'sd15' else 40
        tasks += [(key, jobs[i:i + step]) for i in range(0, len(jobs), step)]
    tasks.sort(key=lambda t: -len(t[1]) * (8 if t[0][1] == 'sd15' else 1))
    res = {}
    with mp.get_context('spawn').Pool(args.jobs) as pool:
        for i, part in enumerate(pool.imap_unordered(run_task, tasks)):
            res.update(part)
            print(f'{i + 1}/{len(tasks)} tasks, {len(res)} plans', file=sys.stderr, flush=True)
    with open(args.out, 'w') as fh:
        json.dump(res, fh)
    print(f'{len(res)} plans, {sum(len(p["rows"]) for p in res.values())} rows, digest {digest(res)}')


def digest(res, dead_words=True):
    h = hashlib.sha256()
    for pid in sorted(res):
        h.update(pid.encode())
        for r in res[pid]['rows']:
            h.update((r if dead_words or '=' not in r.rsplit(':', 1)[1] else r.rsplit(':', 1)[0]).encode())
    return h.hexdigest()[:32]


BYTES_OF = ['ldm/sd15/fp32/-/B=1/rows=2', 'ldm/sd15/fp16/-/B=1/rows=2', 'ldm/sd15/fp32/-/B=16/rows=32', 'ldm/sd15/fp16/-/B=16/rows=32',
            'vae/sd15/fp32/-/B=16', 'vae/sd15/fp16/-/B=16', 'edm/cifar10/fp32/-/B=256/rows=256', 'edm/imagenet64/fp16/-/B=64/rows=64']


def cmd_compare(args):
    A, B = (json.load(open(f)) for f in (args.a, args.b))
    bad = 0
    if args.subset:
        A = {k: v for k, v in A.items() if k in B}
    if set(A) != set(B):
        print(f'plan sets differ: {sorted(set(A) ^ set(B))[:8]}')
        bad += 1
    groups, allowed = {}, {}
    for pid in sorted(set(A) & set(B)):
        g = groups.setdefault('/'.join(pid.split('/')[:3]), [0, 0, 0, 0])
        ra, rb = A[pid]['rows'], B[pid]['rows']
        g[0] += 1
        g[1] += len(ra)
        g[3] += A[pid]['links']
        if ra == rb:
            continue
        diffs = [(x, y) for x, y in zip(ra, rb) if x != y]
        # not a difference of behaviour: same row but for a dead word (row_record; the library's routing answer is inside the hash)
        ok = len(ra) == len(rb) and all(len(x.split(':')) == 3 and x.rsplit(':', 1)[0] == y.rsplit(':', 1)[0] for x, y in diffs)
        if ok:
            for x, y in diffs:
                allowed.setdefault((x.split(':')[0], x.rsplit(':', 1)[1], y.rsplit(':', 1)[1]), []).append(pid)
        else:
            g[2] += 1
            bad += 1
            where = next((i for i, (x, y) in enumerate(zip(ra, rb)) if x != y), min(len(ra), len(rb)))
            print(f'DIFFERENT {pid}: {len(ra)} vs {len(rb)} rows, first at row {where} ({(ra + ["-"])[where].split(":")[0]} / {(rb + ["-"])[where].split(":")[0]})')
    print('configuration                 plans     rows  producer links  plans that differ')
    for g, (n, r, d, k) in sorted(groups.items()):
        print(f'{g:28s} {n:6d} {r:8d} {k:15d} {d:6d}')
    print(f'total: {len(A)} / {len(B)} plans; digest over all rows  {digest(A)}  /  {digest(B)}')
    print(f'                        the same without the dead words  {digest(A, False)}  /  {digest(B, False)}')
    classes = {}
    for (name, va_, vb_), pids in allowed.items():
        c = classes.setdefault((va_.split('=')[0], va_ == vb_.replace(vb_.split('=')[1], '0')), [set(), set(), 0])
        c[0].add(name); c[1].update(pids); c[2] += len(pids)
    for (word, from0), (names, pids, n) in sorted(classes.items()):
        print(f'dead word only: `{word}`{" (was 0)" if from0 else ""} differs on {n} rows of {len(pids)} plans, rest of the row and the library\'s '
              f'routing answer unchanged; launches: {", ".join(sorted(names))}')
    both = set(A) & set(B)
    up = sorted(p for p in both if B[p]['bytes'] > A[p]['bytes'])
    print(f'plan-owned bytes: {len(up)} plans went up {up[:4]}, {sum(1 for p in both if B[p]["bytes"] < A[p]["bytes"])} went down, '
          f'{sum(1 for p in both if B[p]["bytes"] == A[p]["bytes"])} stayed equal')
    for pid in BYTES_OF:
        if pid in both:
            print(f'  {pid:36s} {A[pid]["bytes"] / 2 ** 30:7.2f} GiB in {A[pid]["tensors"]:4d} tensors -> {B[pid]["bytes"] / 2 ** 30:7.2f} GiB in {B[pid]["tensors"]:4d}')
    sys.exit(1 if bad or up else 0)


def cmd_show(args):
    kind, net, mode, variant, b = args.plan.split('/')[:5]
    eng = make_engine(kind, net, mode)
    for suffix, P in build_plans(eng, kind, variant, int(b.split('=')[1])):
        if args.plan.endswith(f'{b}{suffix}'):
            for i, (row, _) in enumerate(dump(eng, P)):
                print(i, json.dumps(row))


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    sub = ap.add_subparsers(dest='cmd', required=True)
    p = sub.add_parser('run'); p.add_argument('--out', required=True); p.add_argument('--jobs', type=int, default=8)
    p.add_argument('--only', default='', help="prefix of kind/net/mode, e.g. 'vae' or 'ldm/sd15/fp16'")
    p.add_argument('--quick', action='store_true', help='seven batches per scanned range instead of all of them')
    p = sub.add_parser('compare'); p.add_argument('a'); p.add_argument('b')
    p.add_argument('--subset', action='store_true', help='B holds only some of the plans of A (run --only / --quick)')
    p = sub.add_parser('show'); p.add_argument('plan')
    args = ap.parse_args()
    dict(run=cmd_run, compare=cmd_compare, show=cmd_show)[args.cmd](args)
