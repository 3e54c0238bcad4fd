"""Test helper: the kernel routing of a launch plan as a per-launch signature, and the batch sweep table the GPU tests run.

Plans are host logic and the launchers' routing rules use compile-time constants (256 CUs), so a plan built on the CPU tells which kernel
every launch of an evaluation at batch B takes.  `signature(plan)` reduces a plan to what the batch can switch:

  * the C entry point of every launch;
  * ds_conv2d_nhwc: the library's own routing decision (ds_conv_route): kernel id (tile shape / kernel family; 2573 = the <= 4-row projection
    kernel) and split-K factor, reported as f16_splits together with the column-tile widths on the stride-1 fp16-activation 3x3 launches;
  * ds_attention (fp32): channel-split or query-split block (ds_attention_variant);
  * ds_gn_stats: whether the launch carries the small-batch `partial` / `counters` scratch (several workgroups per image).

A *boundary* of a configuration is a batch b whose signature differs from that of b - 1.  SWEEP holds, per configuration, the batches
tests/test_hip_batch_sweep.py evaluates on the GPU; tests/test_batch_routing_cpu.py checks that it contains both sides of every boundary
and every batch size a real sampling run hands the engine (sample.shard_seeds)."""
import ctypes as C

from diff_sampler_amd import _lib

# configuration -> (network, engine kind, mode keywords, batch range scanned on the CPU, golden-pinned bench batch).  Batches count sampler
# images (SD-1.5: latents; the U-Net sees twice as many under classifier-free guidance).
CONFIGS = {
    'cifar10_fp32': ('cifar10', 'edm', {}, range(1, 321), 256),
    'cifar10_split': ('cifar10', 'edm', dict(split_fp16=True), range(1, 321), 256),
    'ffhq_fp32': ('ffhq', 'edm', {}, range(1, 161), 128),
    'ffhq_fp16': ('ffhq', 'edm', dict(use_fp16=True), range(1, 161), 128),
    'imagenet64_fp32': ('imagenet64', 'edm', {}, range(1, 81), 64),
    'imagenet64_fp16': ('imagenet64', 'edm', dict(use_fp16=True), range(1, 81), 64),
    'sd15_fp32': ('sd15', 'ldm', {}, range(1, 21), 16),
    'sd15_fp16': ('sd15', 'ldm', dict(use_fp16=True), range(1, 21), 16),
}

# configurations whose routing other tests read, outside the GPU sweep: the CLI tests' tiny SongUNet
OTHER_CONFIGS = {'tiny_song': ('tiny_song', 'edm', {}, range(1, 6), 4)}


def _cfg(config):
    return CONFIGS[config] if config in CONFIGS else OTHER_CONFIGS[config]


# Real sampling runs (sample.py defaults: --batch 64; FID: 50 000 seeds; MS-COCO: 30 000 prompts): (networks, seeds, --batch, GPUs).
# Every batch size sample.shard_seeds hands one rank must be in the sweep of the configurations of those networks.
RUNS = [
    (('cifar10',), 50000, 256, 1), (('cifar10',), 50000, 64, 1), (('cifar10', 'ffhq', 'imagenet64'), 50000, 64, 8),
    (('cifar10', 'ffhq'), 50000, 128, 8), (('sd15',), 30000, 16, 8), (('sd15',), 30000, 64, 1),
]

# The committed sweep: both sides of every boundary the CPU map finds (see test_batch_routing_cpu.py), the ragged batches of RUNS, and
# the bench batch.  A threshold that moves makes the CPU test fail and name the batches to add here.
SWEEP = {
    'cifar10_fp32': [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 32, 33, 37, 38, 40, 41, 42, 43, 44, 45, 48, 49, 50, 51, 52, 53, 54, 63, 64, 65, 66, 67, 72, 73, 75, 76, 80, 81, 84, 85, 86, 88, 89, 96, 97, 102, 103, 112, 113, 115, 116, 118, 119, 127, 128, 129, 144, 145, 149, 150, 160, 161, 170, 171, 176, 177, 192, 193, 204, 205, 213, 214, 255, 256, 257, 264, 265, 288, 289],
    'cifar10_split': [1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 15, 16, 17, 18, 19, 20, 21, 23, 24, 25, 27, 28, 29, 31, 32, 33, 35, 36, 37, 39, 40, 41, 42, 43, 44, 45, 47, 48, 49, 50, 51, 52, 53, 55, 56, 57, 59, 60, 61, 63, 64, 65, 67, 68, 69, 71, 72, 73, 75, 76, 77, 79, 80, 81, 83, 84, 85, 86, 87, 88, 89, 91, 92, 93, 95, 96, 97, 99, 100, 101, 102, 103, 104, 105, 107, 108, 109, 111, 112, 113, 115, 116, 117, 118, 119, 120, 121, 123, 124, 125, 127, 128, 129, 131, 132, 133, 135, 136, 137, 139, 140, 141, 143, 144, 145, 147, 148, 149, 151, 152, 153, 155, 156, 157, 159, 160, 161, 163, 164, 165, 167, 168, 169, 170, 171, 172, 173, 175, 176, 177, 179, 180, 181, 183, 184, 185, 187, 188, 189, 191, 192, 193, 195, 196, 197, 199, 200, 201, 203, 204, 205, 207, 208, 209, 211, 212, 213, 215, 216, 217, 219, 220, 221, 223, 224, 225, 227, 228, 229, 231, 232, 233, 235, 236, 237, 239, 240, 241, 243, 244, 245, 247, 248, 249, 251, 252, 253, 255, 256, 257, 259, 260, 261, 263, 264, 265, 267, 268, 269, 271, 272, 273, 275, 276, 277, 279, 280, 281, 283, 284, 285, 287, 288, 289, 291, 292, 293, 295, 296, 297, 299, 300, 301, 303, 304, 305, 307, 308, 309, 311, 312, 313, 315, 316, 317, 319, 320],
    'ffhq_fp32': [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 19, 20, 21, 22, 23, 24, 25, 26, 28, 29, 31, 32, 33, 34, 36, 37, 38, 40, 41, 42, 43, 44, 45, 48, 49, 50, 51, 52, 53, 54, 56, 57, 63, 64, 65, 66, 67, 72, 73, 75, 76, 80, 81, 82, 84, 85, 86, 88, 89, 96, 97, 98, 100, 101, 102, 103, 112, 113, 127, 128, 129, 144, 145, 149, 150],
    'ffhq_fp16': [2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13, 14, 15, 16, 17, 19, 20, 21, 22, 23, 24, 25, 27, 28, 29, 31, 32, 33, 35, 36, 37, 39, 40, 41, 43, 44, 45, 47, 48, 49, 51, 52, 53, 55, 56, 57, 59, 60, 61, 63, 64, 65, 67, 68, 69, 71, 72, 73, 75, 76, 77, 79, 80, 81, 82, 83, 84, 85, 86, 87, 88, 89, 91, 92, 93, 95, 96, 97, 98, 99, 100, 101, 102, 103, 104, 105, 107, 108, 109, 111, 112, 113, 115, 116, 117, 119, 120, 121, 123, 124, 125, 127, 128, 129, 131, 132, 133, 135, 136, 137, 139, 140, 141, 143, 144, 145, 147, 148, 149, 151, 152, 153, 155, 156, 157, 159, 160],
    'imagenet64_fp32': [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63, 64, 65, 68, 69, 70, 71, 72, 73, 74, 75, 76, 77],
    'imagenet64_fp16': [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 20, 21, 22, 24, 25, 26, 27, 28, 29, 32, 33, 36, 37, 39, 40, 41, 42, 43, 48, 49, 63, 64, 65],
    'sd15_fp32': [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20],
    'sd15_fp16': [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20],
}


def ragged_batches(net):
    """Every batch size sample.shard_seeds gives a rank in the RUNS that sample `net`."""
    from diff_sampler_amd import sample
    out = set()
    for nets, n, batch, world in RUNS:
        if net in nets:
            for rank in range(world):
                out.update(len(b) for b in sample.shard_seeds(list(range(n)), batch, rank, world))
    return sorted(out)


def make_engine(config, device='cpu', seed=1):
    """The engine of a configuration (weights: arch.init_params / init_ldm_params -- routing does not depend on them)."""
    net, kind, kw, _, _ = _cfg(config)
    if kind == 'edm':
        import diff_sampler_amd.arch as arch
        from diff_sampler_amd.engine import UNetEngine
        spec = arch.edm_precond_spec(**dict(arch.NAMED_CONFIGS[net]))
        return UNetEngine(spec, arch.init_params(spec, seed=seed), device=device, **kw)
    import diff_sampler_amd.ldm_arch as la
    from diff_sampler_amd.ldm_engine import LDMUNetEngine
    spec = la.ldm_unet_spec(**dict(la.NAMED_LDM_CONFIGS[net]))
    return LDMUNetEngine(spec, la.init_ldm_params(spec, seed=seed), device=device, **kw)


def sigma_forms(config, B):
    """emb_rows of the plans an evaluation at B images uses: per-sample sigma (one embedding row per U-Net image) and one shared sigma.
    Class-conditional nets embed one row per image either way."""
    net, kind = _cfg(config)[:2]
    n = 2 * B if kind == 'ldm' else B
    if net == 'imagenet64':
        return (n,)
    return (n, 1)


def plan_of(engine, config, B, emb_rows):
    if _cfg(config)[1] == 'ldm':
        return engine.plan(2 * B, emb_rows, 77)
    return engine.plan(B, emb_rows)


def conv_route(a):
    """ds_conv_route of a launch's ds_conv_args (kernel_id, splits, f16_groups, f16_widths)."""
    r = _lib.ConvRouteInfo()
    rc = _lib.load().ds_conv_route(C.byref(a), C.byref(r))
    assert rc == 0, rc
    return r


def signature(plan):
    """[(launch name, entry point, routing fields...)] of every launch of the plan (and of its per-context sub-plan, if any)."""
    lib = _lib.load()
    out = []
    ops = list(plan.ops) + list(getattr(plan, 'ctx', None).ops if getattr(plan, 'ctx', None) is not None else [])
    for op in ops:
        fn = op.fn
        sig = (op.name, fn.__name__)
        if fn is lib.ds_conv2d_nhwc:
            a = op.keep[0]
            r = conv_route(a)
            sig += (('kernel', r.kernel_id),)
            if a.in_f16 and a.taps == 9 and (a.stride or 1) == 1:
                sig += (('f16_splits', r.splits), ('f16_widths', tuple(r.f16_widths[:r.f16_groups])))
            else:
                sig += (('splits', r.splits),)
        elif fn is lib.ds_attention:
            sig += (('attention', 'channel_split' if lib.ds_attention_variant(C.byref(op.keep[0])) == 2 else 'query_split'),)
        elif fn is lib.ds_gn_stats:
            sig += (('gn_partial', bool(op.keep[0].partial)),)
        out.append(sig)
    return out


def diff(sig_a, sig_b, limit=6):
    """Human-readable differences between two signatures: 'name: field a -> b' per launch that changed (at most `limit`, plus a count)."""
    if len(sig_a) != len(sig_b):
        return [f'{len(sig_a)} -> {len(sig_b)} launches']
    out = []
    for x, y in zip(sig_a, sig_b):
        if x != y:
            fx, fy = dict(x[2:]), dict(y[2:])
            if x[:2] != y[:2]:
                out.append(f'{x[0]} ({x[1]}) -> {y[0]} ({y[1]})')
            else:
                ch = ', '.join(f'{k} {fx.get(k)} -> {fy.get(k)}' for k in sorted(set(fx) | set(fy)) if fx.get(k) != fy.get(k))
                out.append(f'{x[0]} ({x[1]}): {ch}')
    n = len(out)
    return out[:limit] + ([f'... {n - limit} more launches'] if n > limit else [])


def routing_map(config, batches=None, engine=None):
    """{B: [(sigma form, signature)]} for every B of the configuration's range (or `batches`); plans are dropped after each batch."""
    eng = engine or make_engine(config)
    res = {}
    for B in (batches or _cfg(config)[3]):
        sig = []
        for form, rows in zip(('per-sample sigma', 'shared sigma'), sigma_forms(config, B)):
            P = plan_of(eng, config, B, rows)
            sig.append((form, tuple(signature(P))))
            P.close()
            eng._plans.clear()
        res[B] = sig
    return res


def boundaries(rmap):
    """[(b, what changed between b - 1 and b)] over a routing map."""
    bs = sorted(rmap)
    out = []
    for b0, b in zip(bs, bs[1:]):
        if b != b0 + 1:
            continue
        if rmap[b] != rmap[b0]:
            why = []
            for (form, s0), (_, s) in zip(rmap[b0], rmap[b]):
                d = diff(list(s0), list(s))
                if d:
                    why.append(f'{form}: ' + '; '.join(d))
            if len(rmap[b0]) != len(rmap[b]):
                why.append('sigma forms differ')
            out.append((b, why))
    return out
