"""GPU: the batch-invariant mode (batch_invariant=True; ds_conv_tune.invariant, ABI 6) -- same seed, same bits at any batch.

Kernel level: every fp32 tile shape the invariant route may choose (tests/test_batch_invariant_cpu.py's chain classes) gives the same output
and GroupNorm column sums bit for bit on every layer class of CIFAR-10 / FFHQ / ImageNet-64 (fused norm, concatenation, fused skip projection,
residual, per-image bias, column sums); the 1x1 kernels likewise; the row kernel gives every row the bits of its one-row launch.
Network level: every configuration at batches on both sides of its default routing boundaries, each row against the same input evaluated
alone (B = 1), in both sigma forms; golden rows at the bench batch within the existing bounds.  Samplers, the CLI and graph replay: equal bits."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import _routing  # noqa: E402

pytestmark = pytest.mark.gpu
G = os.path.join(ROOT, 'tests', 'golden')
GOLDEN = {'cifar10': 'net_cifar10', 'ffhq': 'net_ffhq', 'imagenet64': 'net_imagenet64', 'sd15': 'ldm_sd15'}
# both sides of the default boundaries (tests/_routing.SWEEP): the 4 / 5-row projection rule, the attention at 128, the 256-pixel tiles at 256,
# the fp16x3 B % 4 rule, split-K factors of the small batches
NET_BATCHES = {
    'cifar10_fp32': [4, 5, 8, 127, 128, 256],
    'cifar10_split': [3, 4, 5, 8, 256],
    'ffhq_fp32': [4, 5, 8, 127, 128],
    'ffhq_fp16': [3, 4, 5, 128],
    'imagenet64_fp32': [5, 8, 64],
    'imagenet64_fp16': [3, 5, 64],
    'sd15_fp32': [2, 16],
    'sd15_fp16': [3, 5, 16],
}


@pytest.fixture
def no_autotune(monkeypatch):
    from diff_sampler_amd import plan
    monkeypatch.setattr(plan, 'AUTOTUNE', False)


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


def _sync_cpu(t):
    torch.cuda.synchronize()
    return t.cpu()


# ---- kernel level ---------------------------------------------------------------------------------------------------------------------
# (n, side, c0, c1, cout, skip projection, residual, per-image bias, fused norm)
CONV_CASES = [
    (64, 32, 128, 0, 128, False, True, True, True),        # CIFAR-10 32x32 conv1 (residual)
    (64, 32, 256, 128, 256, True, False, True, True),       # decoder 32x32: concatenation + fused skip projection
    (256, 16, 256, 0, 256, False, True, True, True),        # CIFAR-10 16x16 (256 x 256 tiles by default at 256 images)
    (64, 8, 256, 256, 256, True, False, True, True),        # 8x8, two images per tile, concatenation + skip projection
    (64, 32, 384, 0, 384, False, True, True, True),         # ImageNet-64 channel counts (256 x 192 tiles)
    (16, 64, 192, 0, 192, False, False, True, True),        # ImageNet-64 64x64
    (128, 16, 256, 0, 256, False, False, False, False),     # plain input
]
# tune (mode, variant) -> the tile it forces: the route's own choice, the 128- and 256-pixel tiles, the 256 x 256 tiles.  The 256 x 192 tiles
# (variant bit 14 forces them, kernel id 2568) leave the same outputs but other column sums: the invariant route never takes them (checked below)
TILE_TUNES = [(0, 0), (128, 0), (256, 0), (256, 6)]


def _conv_layer(case, gen, dev):
    from diff_sampler_amd.plan import Builder
    n, s, c0, c1, cout, skip, res, cb, norm = case
    bd = Builder(dev, invariant=True, batch=n)
    r = lambda *sh: torch.randn(*sh, generator=gen).to(dev)      # noqa: E731
    M = n * s * s
    x0, x1 = r(M, c0), (r(M, c1) if c1 else None)
    ec = (c0 + c1) if skip else 0
    K = 9 * (c0 + c1) + ec
    w = r(-(-cout // 128) * 128, K) * (1.0 / K ** 0.5)
    kw = dict(x1=x1, c1=c1, ld1=c1, bias=r(cout), stats=True)
    if skip:
        kw.update(e0=x0, ec0=c0, e1=x1, ec1=c1)
    if res:
        kw.update(res=r(M, cout), res_ld=cout)
    if cb:
        kw.update(cbias=r(n, cout + 64), cbias_ld=cout + 64, cbias_rows=n)
    if norm:
        planes = r(n, 3, c0 + c1)
        from diff_sampler_amd._lib import DS_ACT_SILU
        kw.update(norm_coefs=planes, norm_act=DS_ACT_SILU)
    out = bd.new(M, cout)
    bd.conv(x0, c0, c0, n, s, s, w, cout, out, cout, 9, 'layer', **kw)
    return bd, out


@pytest.mark.parametrize('case', CONV_CASES)
def test_fp32_tiles_of_the_invariant_route_are_bit_identical(case):
    from diff_sampler_amd import _lib
    lib = _lib.load()
    dev = torch.device('cuda')
    bd, out = _conv_layer(case, torch.Generator().manual_seed(sum(case[:5])), dev)
    a = bd.P.ops[-1].keep[0]
    sb = bd.stats_of[out.data_ptr()][0]
    ref, seen = None, {}
    for mode, variant in TILE_TUNES:
        a.tune.mode, a.tune.variant = mode, variant
        kid = _routing.conv_route(a).kernel_id
        if kid in seen:
            continue
        out.fill_(float('nan')); sb.fill_(float('nan'))
        _lib.check(lib.ds_conv2d_nhwc(C.byref(a), _lib.stream_ptr()), 'conv')
        got = (_sync_cpu(out).clone(), _sync_cpu(sb).clone())
        assert torch.isfinite(got[0]).all() and torch.isfinite(got[1]).all(), (case, kid)
        seen[kid] = (mode, variant)
        if ref is None:
            ref = got
            continue
        assert torch.equal(got[0], ref[0]), (case, kid, 'output', _rel(got[0], ref[0]))
        assert torch.equal(got[1], ref[1]), (case, kid, 'column sums', _rel(got[1], ref[1]))
    assert 128 in seen and len(seen) >= 2 and 2568 not in seen, (case, seen)
    a.tune.mode, a.tune.variant = 256, 16384
    assert _routing.conv_route(a).kernel_id != 2568, case


@pytest.mark.parametrize('rows,cout,res', [(65536, 768, False), (65536, 256, True), (16384, 1280, False)])
def test_fp32_1x1_kernels_of_the_invariant_route_are_bit_identical(rows, cout, res):
    from diff_sampler_amd import _lib
    from diff_sampler_amd.plan import Builder
    lib = _lib.load()
    dev = torch.device('cuda')
    gen = torch.Generator().manual_seed(rows + cout)
    bd = Builder(dev, invariant=True, batch=rows // 256)
    k = 256 if cout != 1280 else 320
    x, w = torch.randn(rows, k, generator=gen).to(dev), torch.randn(-(-cout // 128) * 128, k, generator=gen).to(dev)
    out = bd.new(rows, cout)
    kw = dict(res=torch.randn(rows, cout, generator=gen).to(dev), res_ld=cout, stats=True) if res else {}
    bd.linear(x, k, rows, w, cout, out, 'proj', bias=torch.randn(cout, generator=gen).to(dev), **kw)
    a = bd.P.ops[-1].keep[0]
    sb = bd.stats_of[out.data_ptr()][0] if res else None
    results = {}
    for mode in (0, 6):                                             # the route's own choice (gemm_dma8 at these sizes) / the generic GEMM
        a.tune.mode = mode
        kid = _routing.conv_route(a).kernel_id
        out.fill_(float('nan'))
        if sb is not None:
            sb.fill_(float('nan'))
        _lib.check(lib.ds_conv2d_nhwc(C.byref(a), _lib.stream_ptr()), 'linear')
        results[kid] = (_sync_cpu(out).clone(), None if sb is None else _sync_cpu(sb).clone())
        assert torch.isfinite(results[kid][0]).all(), kid
    assert sorted(results) == [0, 2561], sorted(results)
    assert torch.equal(results[0][0], results[2561][0]), _rel(results[0][0], results[2561][0])
    if sb is not None:                                              # the GroupNorm column sums of the proj layers (stats=True)
        assert torch.isfinite(results[0][1]).all()
        assert torch.equal(results[0][1], results[2561][1]), _rel(results[0][1], results[2561][1])


def test_row_kernel_gives_every_row_its_one_row_bits():
    from diff_sampler_amd import _lib
    from diff_sampler_amd.plan import Builder
    dev = torch.device('cuda')
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(256, 512, generator=gen).to(dev)
    w, b = torch.randn(8448, 512, generator=gen).to(dev) * 0.05, torch.randn(8448, generator=gen).to(dev)

    def rows_out(xs):
        bd = Builder(dev, invariant=True, batch=xs.shape[0])
        out = bd.new(xs.shape[0], 8448)
        bd.linear(xs.contiguous(), 512, xs.shape[0], w, 8448, out, 'emb', bias=b, act=_lib.DS_ACT_SILU, emb=True)
        assert _routing.conv_route(bd.P.ops[-1].keep[0]).kernel_id == 2573
        bd.P.run_python(_lib.stream_ptr())
        return _sync_cpu(out)
    full = rows_out(x)
    for m in (1, 4, 5, 256):
        assert torch.equal(rows_out(x[:m]), full[:m]), m
    for i in (3, 4, 5, 130, 255):
        assert torch.equal(rows_out(x[i:i + 1]), full[i:i + 1]), i
    ref = (x.double() @ w.double().T + b.double())
    ref = ref * torch.sigmoid(ref)
    assert _rel(full, ref.cpu()) < 2e-5


# ---- network level ----------------------------------------------------------------------------------------------------------------------
def _net(config):
    net_name, kind, kw, _, bench = _routing.CONFIGS[config]
    z = np.load(os.path.join(G, GOLDEN[net_name] + '.npz'))
    if kind == 'edm':
        from diff_sampler_amd.engine import EDMDenoiser
        return EDMDenoiser.from_config(net_name, seed=int(z['seed']), batch_invariant=True, **kw), z
    from diff_sampler_amd.ldm_engine import CFGDenoiser
    return CFGDenoiser.from_config(net_name, seed=int(z['seed']), guidance_rate=7.5, batch_invariant=True, **kw), z


@pytest.mark.parametrize('config', list(_routing.CONFIGS))
def test_network_rows_equal_their_one_image_evaluation(config, no_autotune):
    _network_rows(config, NET_BATCHES[config], golden=True)


@pytest.mark.parametrize('config,batches', [('imagenet64_fp16', [3, 64]), ('sd15_fp16', [3, 16])])
def test_fp16_network_rows_with_the_default_tile_measurement(config, batches, monkeypatch):
    """The same check with plan.AUTOTUNE as users run it (the default): fp16-activation tile widths from the persisted table or measured
    while the plan is built, per batch.  Only launches whose bits do not depend on the width are measured (plan._tile_neutral)."""
    from diff_sampler_amd import plan
    monkeypatch.setattr(plan, 'AUTOTUNE', True)
    _network_rows(config, batches, golden=False)


def _network_rows(config, batches, golden):
    net_name, kind, kw, _, bench = _routing.CONFIGS[config]
    mode = 'fp16' if kw.get('use_fp16') else 'fp32'
    net, z = _net(config)
    dev = torch.device('cuda')
    n_max = bench
    g = torch.Generator().manual_seed(99)
    if kind == 'edm':
        R, Cc = net.img_resolution, net.img_channels
        x = torch.randn(n_max, Cc, R, R, generator=g)
        sig = torch.exp(torch.randn(n_max, generator=g) * 1.2 - 0.4)
        x = x * torch.sqrt(sig ** 2 + 0.25).view(-1, 1, 1, 1)
        lab = torch.eye(net.label_dim)[torch.randint(net.label_dim, (n_max,), generator=g)] if net.label_dim else None
        gx, gs = torch.from_numpy(z['x']), torch.from_numpy(z['sigma']).reshape(-1).expand(z['x'].shape[0])
        gl = torch.from_numpy(z['labels']) if z['labels'].size else None

        def ev(idx, s):
            out = net(x[idx].to(dev), s.to(dev) if torch.is_tensor(s) else s, class_labels=None if lab is None else lab[idx].to(dev))
            return _sync_cpu(out)
    else:
        x = torch.randn(n_max, 4, 64, 64, generator=g)
        sig = torch.rand(n_max, generator=g) * 13 + 0.5
        x = x * torch.sqrt(sig ** 2 + 1).view(-1, 1, 1, 1)
        c, u = torch.randn(n_max, 77, 768, generator=g), torch.randn(n_max, 77, 768, generator=g)

        def ev(idx, s):
            out = net(x[idx].to(dev), s.to(dev) if torch.is_tensor(s) else s, condition=c[idx].to(dev), unconditional_condition=u[idx].to(dev))
            return _sync_cpu(out)
    # each row alone (B = 1: the shared-sigma form, one embedding row) -- per-sample sigma; and at one common sigma
    alone = torch.cat([ev(torch.tensor([i]), sig[i:i + 1]) for i in range(n_max)])
    s0 = float(sig[0])
    shared_rows = sorted({0, 1, 4, n_max - 1})
    alone_s0 = {i: ev(torch.tensor([i]), s0) for i in shared_rows}
    net.engine._plans.clear()
    for B in batches:
        idx = torch.arange(B)
        out = ev(idx, sig[:B])                                             # per-sample sigma form
        bad = [i for i in range(B) if not torch.equal(out[i], alone[i])]
        assert not bad, (config, B, bad[:8], max(_rel(out[i], alone[i]) for i in bad))
        out_s = ev(idx, s0)                                                # shared sigma form
        for i in shared_rows:
            if i < B:
                assert torch.equal(out_s[i:i + 1], alone_s0[i]), (config, B, 'shared sigma', i)
        net.engine._plans.clear()
        torch.cuda.empty_cache()
    # the bench batch within the existing golden bounds
    if not golden:
        pass
    elif kind == 'edm':
        n_gold = gx.shape[0]
        xs, ss = x.clone(), sig.clone()
        xs[:n_gold], ss[:n_gold] = gx, gs
        if lab is not None:
            lab[:n_gold] = gl
        x, sig = xs, ss
        out = ev(torch.arange(bench), sig)
        eg = max(_rel(out[i:i + 1], torch.from_numpy(z['out_vec'])[i:i + 1]) for i in range(n_gold))
        assert eg < (5e-3 if mode == 'fp16' else 2e-4), (config, eg)
    else:
        gx, gs = torch.from_numpy(z['x']), torch.from_numpy(z['sigma']).reshape(-1)
        n_gold = gx.shape[0]
        x[:n_gold], sig[:n_gold] = gx, gs
        c[:n_gold], u[:n_gold] = torch.from_numpy(z['cond']), torch.from_numpy(z['uncond'])
        out = ev(torch.arange(bench), sig)
        gout = torch.from_numpy(z['out_vec'])
        eg = max(_rel(out[i:i + 1], gout) for i in range(n_gold))
        if mode == 'fp16':
            z16 = np.load(os.path.join(G, 'ldm_sd15_f16ops.npz'))
            assert eg < min(1.5 * float(z16['rel_vs_fp32_golden']), 6.5e-3), (config, eg)
        else:
            assert eg < 2e-4, (config, eg)
    net.engine._plans.clear()
    torch.cuda.empty_cache()


# ---- samplers, CLI, graph replay -------------------------------------------------------------------------------------------------------------
def _dpmpp(net, lat, **kw):
    from diff_sampler_amd import solvers
    out = solvers.dpm_pp_sampler(net, lat, num_steps=11, sigma_min=0.002, sigma_max=80., schedule_type='logsnr', schedule_rho=7,
                                 max_order=2, predict_x0=True, lower_order_final=True, **kw)
    return _sync_cpu(out)


def test_cifar10_dpmpp2m_nfe10_at_1_and_256(no_autotune):
    from diff_sampler_amd.engine import EDMDenoiser
    dev = torch.device('cuda')
    net = EDMDenoiser.from_config('cifar10', seed=3, batch_invariant=True)
    lat = torch.randn(256, 3, 32, 32, generator=torch.Generator().manual_seed(256))
    full = _dpmpp(net, lat.to(dev))
    net.engine._plans.clear()
    for i in (0, 1, 3, 4, 5, 63, 127, 128, 200, 255):
        assert torch.equal(_dpmpp(net, lat[i:i + 1].to(dev)), full[i:i + 1]), i


def test_amed_per_sample_sigma_at_1_4_and_8(no_autotune):
    from oracle import cases
    from diff_sampler_amd import solvers_amed
    from diff_sampler_amd.engine import EDMDenoiser
    dev = torch.device('cuda')
    net = EDMDenoiser.from_config('cifar10', seed=5, batch_invariant=True)
    pred = solvers_amed.AMEDPredictor(cases.amed_predictor_params(11, 0.01, 0), device=dev, num_steps=4, sampler_stu='amed',
                                      schedule_type='time_uniform', schedule_rho=1, afs=True, scale_dir=0.01, scale_time=0)
    lat = torch.randn(8, 3, 32, 32, generator=torch.Generator().manual_seed(8))

    def run(x):
        out = solvers_amed.amed_sampler(net, x.to(dev), num_steps=4, sigma_min=0.002, sigma_max=80., schedule_type='time_uniform',
                                        schedule_rho=1, afs=True, AMED_predictor=pred)
        return _sync_cpu(out)
    full = run(lat)
    assert torch.isfinite(full).all()
    assert torch.equal(run(lat[:4]), full[:4])
    for i in range(8):
        assert torch.equal(run(lat[i:i + 1]), full[i:i + 1]), i


def test_sd15_fp16_dpmpp_at_1_and_16(no_autotune):
    from diff_sampler_amd import solvers
    from diff_sampler_amd.ldm_engine import CFGDenoiser
    dev = torch.device('cuda')
    net = CFGDenoiser.from_config('sd15', seed=2, guidance_rate=7.5, use_fp16=True, batch_invariant=True)
    g = torch.Generator().manual_seed(16)
    lat = torch.randn(16, 4, 64, 64, generator=g)
    cond, uncond = torch.randn(16, 77, 768, generator=g), torch.randn(1, 77, 768, generator=g).expand(16, 77, 768).contiguous()

    def run(idx):
        out = solvers.dpm_pp_sampler(net, lat[idx].to(dev), condition=cond[idx].to(dev),
                                     unconditional_condition=uncond[idx].to(dev), num_steps=6, sigma_min=net.sigma_min, sigma_max=net.sigma_max,
                                     schedule_type='discrete', schedule_rho=1, max_order=2, predict_x0=False, lower_order_final=True)
        return _sync_cpu(out)
    full = run(torch.arange(16))
    assert torch.isfinite(full).all()
    net.engine._plans.clear()
    for i in (0, 7, 15):
        assert torch.equal(run(torch.tensor([i])), full[i:i + 1]), i


def test_cli_writes_the_same_png_bytes_at_batch_1_7_and_64(tmp_path):
    """As users run the CLI: the default plan settings (tile measurement on)."""
    from diff_sampler_amd import sample
    files = {}
    for batch in (1, 7, 64):
        out, n = sample.run('cifar10', max_batch_size=batch, seeds='0-63', outdir=str(tmp_path / f'b{batch}'), solver='dpmpp', max_order=2,
                            num_steps=4, random_init=True, batch_invariant=True)
        assert n == 64
        got = {}
        for d, _, fs in os.walk(out):
            for f in fs:
                if f.endswith('.png'):
                    with open(os.path.join(d, f), 'rb') as fh:
                        got[f] = fh.read()
        assert len(got) == 64
        files[batch] = got
    assert files[1] == files[7] == files[64]


def test_graph_replay_equals_eager_and_the_one_image_run(no_autotune):
    from diff_sampler_amd import solvers
    from diff_sampler_amd.engine import EDMDenoiser
    from diff_sampler_amd.graph import GraphedSampler
    dev = torch.device('cuda')
    net = EDMDenoiser.from_config('cifar10', seed=4, batch_invariant=True)
    kw = dict(num_steps=6, max_order=2, schedule_type='logsnr')
    g = GraphedSampler(solvers.dpm_pp_sampler, net, (8, 3, 32, 32), **kw)
    lat = torch.randn(8, 3, 32, 32, generator=torch.Generator().manual_seed(1)).to(dev)
    graphed = _sync_cpu(g(lat))
    eager = _sync_cpu(solvers.dpm_pp_sampler(net, lat, **kw))
    assert torch.equal(graphed, eager)
    for i in (0, 5):
        assert torch.equal(_sync_cpu(solvers.dpm_pp_sampler(net, lat[i:i + 1].contiguous(), **kw)), graphed[i:i + 1]), i
