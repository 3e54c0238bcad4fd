"""GPU: every network at every batch of the sweep table (tests/_routing.SWEEP: both sides of every routing boundary the CPU map finds,
and the ragged batches real sampling runs hand the engine), and the sampler trajectories at the ragged CLI batches.

Network sweep, per configuration and batch B, one evaluation with per-sample sigma.  The shared-sigma plans differ from the per-sample ones
only in the embedding path, and every boundary of that form is also one of the per-sample form (tests/test_batch_routing_cpu.py asserts it), so
the per-sample evaluations run every routing the map finds; the sampler tests below run the shared form at the ragged CLI batches:
  * golden slots -- the real reference's items (net_cifar10 / net_ffhq / net_imagenet64 / ldm_sd15, + ldm_sd15_f16ops for SD-1.5 fp16)
    in slot 0, slot B - 1 (the last, usually partial, tile) and one slot of every residue class mod 4, each checked at the bound of its
    existing test (fp32 2e-4; ImageNet-64 fp16 5e-3; SD-1.5 fp16 the f16-oracle bounds);
  * every row -- the same inputs evaluated at the configuration's golden-pinned bench batch (chunked / padded): each row at B must agree
    with its own row there, normalised by that row's own scale, at the mode's evaluation bound, and every output must be finite.
Outputs are batch-invariant only to the mode's rounding: a different batch can take a different kernel, tile or
split-K order, so no comparison here is bit for bit.

Tile measurement is off (plan.AUTOTUNE): a tile-table miss would time every candidate at every batch; tile shapes are bit-neutral
(tests/test_hip_fp16.py).  Plans and device memory are freed between batches.  What every test observed goes through tests/_parity.record."""
import os
import sys
import time

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import _routing  # noqa: E402
from _parity import per_step_rel, record  # noqa: E402

pytestmark = pytest.mark.gpu
G = os.path.join(ROOT, 'tests', 'golden')
GOLDEN = {'cifar10': 'net_cifar10', 'ffhq': 'net_ffhq', 'imagenet64': 'net_imagenet64', 'sd15': 'ldm_sd15'}
# one evaluation against the same evaluation at the bench batch, per row: the mode's per-evaluation bound.  SD-1.5 fp16 compares GUIDED
# outputs: two placements of the fp16 roundings (another split-K order moves ~0.2 % of them across a boundary) differ there by the bound of
# the guided output against the fp16-operand oracle, 7.5e-3 (tests/test_hip_fp16.py; the ~4e-3 noise of the mode on each side, 7.5x guidance)
ROW_TOL = {'fp32': 2e-4, 'split': 2e-4, 'fp16': 5e-3, 'sd15_fp16': 7.5e-3}


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


def _row_rel(a, b):
    """[rows] max |a_i - b_i| / max |b_i|: each image against its own scale."""
    a, b = a.double().flatten(1), b.double().flatten(1)
    return ((a - b).abs().amax(1) / b.abs().amax(1).clamp_min(1e-6)).tolist()


def golden_slots(B):
    """Slot 0, slot B - 1 and, where B allows, one slot of every residue class mod 4 (around the middle of the batch)."""
    mid = (B // 2) // 4 * 4
    return sorted({0, B - 1} | {mid + r for r in range(4) if mid + r < B})


@pytest.fixture
def no_autotune(monkeypatch):
    from diff_sampler_amd import plan
    monkeypatch.setattr(plan, 'AUTOTUNE', False)


def _free(net):
    net.engine._plans.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _edm_eval(net, x, sig, lab, dev):
    out = net(x.to(dev), sig.to(dev), class_labels=None if lab is None else lab.to(dev)).cpu()
    torch.cuda.synchronize()
    return out


def _ldm_eval(net, x, sig, c, u, dev):
    out = net(x.to(dev), sig.to(dev), condition=c.to(dev), unconditional_condition=u.to(dev)).cpu()
    torch.cuda.synchronize()
    return out


def _chunked(fn, n_rows, bench, *tensors):
    """fn over the first n_rows rows of `tensors` evaluated in chunks of exactly `bench` rows (the last chunk padded with rows from the
    front): the reference evaluation at the bench batch."""
    outs = []
    for s in range(0, n_rows, bench):
        idx = torch.arange(s, s + bench) % n_rows
        outs.append(fn(*(t[idx] for t in tensors))[:min(bench, n_rows - s)])
    return torch.cat(outs)


@pytest.mark.parametrize('config', list(_routing.CONFIGS))
def test_network_at_every_swept_batch(config, no_autotune):
    net_name, kind, kw, _, bench = _routing.CONFIGS[config]
    mode = 'fp16' if kw.get('use_fp16') else ('split' if kw.get('split_fp16') else 'fp32')
    batches = _routing.SWEEP[config]
    dev = torch.device('cuda')
    z = np.load(os.path.join(G, GOLDEN[net_name] + '.npz'))
    t0 = time.time()
    n_max = max(batches)
    g = torch.Generator().manual_seed(4242)
    if kind == 'edm':
        from diff_sampler_amd.engine import EDMDenoiser
        net = EDMDenoiser.from_config(net_name, seed=int(z['seed']), **kw)
        R, C = net.img_resolution, net.img_channels
        gx, gs = torch.from_numpy(z['x']), torch.from_numpy(z['sigma']).reshape(-1).expand(z['x'].shape[0])
        gl = torch.from_numpy(z['labels']) if z['labels'].size else None
        gout = torch.from_numpy(z['out_vec'])
        x = torch.randn(n_max, C, R, R, generator=g)
        sig = torch.exp(torch.randn(n_max, generator=g) * 1.2 - 0.4)      # EDM sigma distribution (P_mean -1.2 scaled down, P_std 1.2)
        x = x * torch.sqrt(sig ** 2 + 0.25).view(-1, 1, 1, 1)
        lab = torch.eye(net.label_dim)[torch.randint(net.label_dim, (n_max,), generator=g)] if net.label_dim else None
        evaluate = (lambda x_, s_, l_=None: _edm_eval(net, x_, s_, l_, dev)) if lab is not None else (lambda x_, s_: _edm_eval(net, x_, s_, None, dev))
        inputs = (x, sig, lab) if lab is not None else (x, sig)
    else:
        from diff_sampler_amd.ldm_engine import CFGDenoiser
        net = CFGDenoiser.from_config(net_name, seed=int(z['seed']), guidance_rate=7.5, **kw)
        gx, gs = torch.from_numpy(z['x']), torch.from_numpy(z['sigma']).reshape(-1)
        gc, gu = torch.from_numpy(z['cond']), torch.from_numpy(z['uncond'])
        gout = torch.from_numpy(z['out_vec'])
        x = torch.randn(n_max, 4, 64, 64, generator=g)
        sig = torch.rand(n_max, generator=g) * 13 + 0.5
        x = x * torch.sqrt(sig ** 2 + 1).view(-1, 1, 1, 1)
        c, u = torch.randn(n_max, 77, 768, generator=g), torch.randn(n_max, 77, 768, generator=g)
        evaluate = lambda x_, s_, c_, u_: _ldm_eval(net, x_, s_, c_, u_, dev)  # noqa: E731
        inputs = (x, sig, c, u)
        z16 = np.load(os.path.join(G, 'ldm_sd15_f16ops.npz')) if mode == 'fp16' else None
    n_gold = gx.shape[0]
    golden_tol = 5e-3 if mode == 'fp16' else 2e-4

    # the reference rows: every master row at the bench batch
    ref = _chunked(evaluate, n_max, bench, *inputs)
    _free(net)
    assert torch.isfinite(ref).all()
    worst_row, worst_gold, per_batch = 0.0, 0.0, {}
    for B in batches:
        slots = golden_slots(B)
        items = [j % n_gold for j in range(len(slots))]
        xs = [t[:B].clone() for t in inputs]
        xs[0][slots], xs[1][slots] = gx[items], gs[items]
        if kind == 'edm' and lab is not None:
            xs[2][slots] = gl[items]
        if kind == 'ldm':
            xs[2][slots], xs[3][slots] = gc[items], gu[items]
        out = evaluate(*xs)
        if kind == 'ldm' and mode == 'fp16':
            from _f16_names import ldm_prefixes
            # the raw U-Net outputs of the golden slots (unconditional / conditional halves) against the fp16-operand oracle's: 2.5e-3
            f_rows, plan, _ = net.raw(xs[0].to(dev), xs[1].to(dev), xs[2].to(dev), xs[3].to(dev))
            eps = f_rows.reshape(2 * B, 64, 64, 4).permute(0, 3, 1, 2).cpu()
            e_eps = max(_rel(eps[[s, B + s]], torch.from_numpy(z16['eps_f16ops'])) for s in slots)
            assert sorted(ldm_prefixes(plan)) == [str(v) for v in z16['f16_layers']], B      # the f16 oracle rounded exactly these layers
        _free(net)
        assert torch.isfinite(out).all(), (config, B)
        others = [i for i in range(B) if i not in slots]
        rr = max(_row_rel(out[others], ref[others]), default=0.0)
        if kind == 'ldm' and mode == 'fp16':
            eg32 = max(_rel(out[s:s + 1], gout) for s in slots)
            eg = max(_rel(out[s:s + 1], torch.from_numpy(z16['out_f16ops'])) for s in slots)
            noise = float(z16['rel_vs_fp32_golden'])
            per_batch[B] = dict(rows=rr, golden_vs_f16_oracle=eg, golden_vs_fp32=eg32, golden_unet_outputs_vs_f16_oracle=e_eps)
            assert eg < 7.5e-3 and eg32 < min(1.5 * noise, 6.5e-3) and e_eps < 2.5e-3, (config, B, eg, eg32, e_eps)
        else:
            eg = max(_rel(out[s:s + 1], gout[it:it + 1]) for s, it in zip(slots, items))
            per_batch[B] = dict(rows=rr, golden=eg)
            assert eg < golden_tol, (config, B, slots, eg)
        assert rr < ROW_TOL.get(config, ROW_TOL[mode]), (config, B, rr)
        worst_row, worst_gold = max(worst_row, rr), max(worst_gold, eg)
    del net
    torch.cuda.empty_cache()
    record(f'batch_sweep_{config}', batches=len(batches), worst_row_vs_bench_batch=worst_row, worst_golden=worst_gold,
           per_batch={str(k): v for k, v in per_batch.items()}, wall_s=round(time.time() - t0, 1))


# ---- sampler trajectories at the ragged batches of real runs (sample.shard_seeds): golden latents in slot 0, slot B - 1 and inner slots ----
def _scatter(B, gold, seed):
    """[B] latents with the golden ones in golden_slots(B) plus, when there are more golden latents than that, evenly spaced inner
    slots (golden latents cycled over the slots), and the slot -> golden index lists."""
    slots = set(golden_slots(B))
    need = gold.shape[0] - len(slots)
    if need > 0:                                             # inner slots not taken yet, evenly spaced
        free = [i for i in range(1, B - 1) if i not in slots]
        slots |= set(free[j * len(free) // need] for j in range(need))
    slots = sorted(slots)
    items = [j % gold.shape[0] for j in range(len(slots))]
    lat = torch.randn(B, *gold.shape[1:], generator=torch.Generator().manual_seed(seed))
    lat[slots] = gold[items]
    return lat, slots, items


def _pad(t, bench):
    """t padded to the bench batch with rows from its front."""
    return t[torch.arange(bench) % t.shape[0]]


@pytest.mark.parametrize('B', [255, 127])
def test_headline_sampler_at_ragged_batches(B, no_autotune):
    from diff_sampler_amd import solvers
    from diff_sampler_amd.engine import EDMDenoiser
    dev = torch.device('cuda')
    z = np.load(os.path.join(G, 'sampler_cifar10_dpmpp2m_nfe10_b64.npz'))
    net = EDMDenoiser.from_config('cifar10', seed=int(z['seed']))
    gold_lat = torch.randn(64, 3, 32, 32, generator=torch.Generator().manual_seed(int(z['latent_seed'])))
    lat, slots, items = _scatter(B, gold_lat, 5150 + B)

    def run(x):
        o = solvers.dpm_pp_sampler(net, x.to(dev), num_steps=11, sigma_min=0.002, sigma_max=80., schedule_type='logsnr', schedule_rho=7,
                                   max_order=2, predict_x0=True, lower_order_final=True).cpu()
        torch.cuda.synchronize()
        _free(net)
        return o
    out = run(lat)
    ref = run(_pad(lat, 256))[:B]
    assert torch.isfinite(out).all()
    eg = max(_rel(out[s:s + 1], torch.from_numpy(z['out'][it:it + 1])) for s, it in zip(slots, items))
    rr = max(_row_rel(out, ref))
    record(f'headline_dpmpp2m_nfe10_b{B}', golden_slots=len(slots), final_golden=eg, worst_row_vs_b256=rr, bound=5e-4)
    assert eg < 5e-4 and rr < 5e-4, (B, eg, rr)


@pytest.mark.parametrize('mode', ['fp32', 'fp16'])
def test_ffhq64_sampler_at_ragged_batch_127(mode, no_autotune):
    from diff_sampler_amd import solvers
    from diff_sampler_amd.engine import EDMDenoiser
    dev = torch.device('cuda')
    z = np.load(os.path.join(G, 'sampler_ffhq_dpmpp2m_nfe10_b2.npz'))
    net = EDMDenoiser.from_config('ffhq', seed=int(z['seed']), use_fp16=(mode == 'fp16'))
    B, tol = 127, (1e-2 if mode == 'fp16' else 5e-4)
    lat, slots, items = _scatter(B, torch.from_numpy(z['latents']), 127)

    def run(x):
        o = solvers.dpm_pp_sampler(net, x.to(dev), num_steps=11, sigma_min=0.002, sigma_max=80., schedule_type='logsnr', schedule_rho=7,
                                   max_order=2, predict_x0=True, lower_order_final=True).cpu()
        torch.cuda.synchronize()
        _free(net)
        return o
    out = run(lat)
    ref = run(_pad(lat, 128))[:B]
    assert torch.isfinite(out).all()
    eg = max(_rel(out[s:s + 1], torch.from_numpy(z['out'][it:it + 1])) for s, it in zip(slots, items))
    rr = max(_row_rel(out, ref))
    record(f'ffhq64_dpmpp2m_nfe10_b127_{mode}', final_golden=eg, worst_row_vs_b128=rr, bound=tol)
    assert eg < tol and rr < tol, (mode, eg, rr)


def test_imagenet64_fp16_ipndm_gits_at_ragged_batch_63(no_autotune):
    from diff_sampler_amd import solvers
    from diff_sampler_amd.engine import EDMDenoiser
    dev = torch.device('cuda')
    z = np.load(os.path.join(G, 'sampler_imagenet64_ipndm_gits_nfe10_b1.npz'))
    net = EDMDenoiser.from_config('imagenet64', seed=int(z['seed']), use_fp16=True)
    B = 63
    lat, slots, _ = _scatter(B, torch.from_numpy(z['latents']), 63)
    labels = torch.eye(1000)[torch.randint(1000, (B,), generator=torch.Generator().manual_seed(630))]
    labels[slots] = torch.from_numpy(z['labels'])

    def run(x, lab):
        o = solvers.ipndm_sampler(net, x.to(dev), class_labels=lab.to(dev), max_order=4, t_steps=torch.from_numpy(z['t_steps']).to(dev),
                                  num_steps=11, return_inters=True).cpu()
        torch.cuda.synchronize()
        _free(net)
        return o
    out = run(lat, labels)
    ref = run(_pad(lat, 64), _pad(labels, 64))[:, :B]
    assert torch.isfinite(out).all()
    gold = torch.from_numpy(z['traj'])
    worst = [0.0] * gold.shape[0]
    for s in slots:
        worst = [max(a, b) for a, b in zip(worst, per_step_rel(out[:, s:s + 1], gold))]
    rr = max(_row_rel(out[-1], ref[-1]))
    record('imagenet64_ipndm4_gits_b63_fp16', golden_slots=slots, per_step=worst, final=worst[-1], worst_row_vs_b64=rr, bound=1e-2)
    assert max(worst) < 1e-2 and worst[-1] < 1e-2 and rr < 1e-2, (worst, rr)


def test_sd15_fp16_sampler_at_ragged_batch_15(no_autotune):
    """The bounds of test_config5_sd15_at_the_benchmark_batch_b16 (fp16): every step within 1.5 x the fp16-stream oracle's own distance from
    the fp32 golden (ceiling 2e-2) and within 2 x that noise of the oracle's fp16 trajectory; other rows within 1e-2 of the run at 16."""
    from diff_sampler_amd import solvers
    from diff_sampler_amd.ldm_engine import CFGDenoiser
    dev = torch.device('cuda')
    z = np.load(os.path.join(G, 'ldm_sd15_traj_b2.npz'))
    z16 = np.load(os.path.join(G, 'ldm_sd15_traj_b2_f16ops.npz'))
    net = CFGDenoiser.from_config('sd15', seed=int(z['seed']), guidance_rate=7.5, use_fp16=True)
    B = 15
    lat, slots, items = _scatter(B, torch.from_numpy(z['latents']), 15)
    g = torch.Generator().manual_seed(1515)
    cond, uncond = torch.randn(B, 77, 768, generator=g), torch.randn(B, 77, 768, generator=g)
    cond[slots], uncond[slots] = torch.from_numpy(z['cond'])[items], torch.from_numpy(z['uncond'])[items]

    def run(x, c, u):
        o = solvers.dpm_pp_sampler(net, x.to(dev), condition=c.to(dev), unconditional_condition=u.to(dev), num_steps=6, sigma_min=net.sigma_min,
                                   sigma_max=net.sigma_max, schedule_type='discrete', schedule_rho=1, return_inters=True,
                                   max_order=2, predict_x0=False, lower_order_final=True).cpu()
        torch.cuda.synchronize()
        _free(net)
        return o
    tr = run(lat, cond, uncond)
    ref = run(_pad(lat, 16), _pad(cond, 16), _pad(uncond, 16))[:, :B]
    assert torch.isfinite(tr).all()
    gold, gold16 = torch.from_numpy(z['traj']), torch.from_numpy(z16['traj_f16ops'])
    noise = [float(v) for v in z16['per_step_rel_vs_fp32_golden']]
    errs = [0.0] * gold.shape[0]
    errs16 = [0.0] * gold.shape[0]
    for s, it in zip(slots, items):
        errs = [max(a, b) for a, b in zip(errs, per_step_rel(tr[:, s:s + 1], gold[:, it:it + 1]))]
        errs16 = [max(a, b) for a, b in zip(errs16, per_step_rel(tr[:, s:s + 1], gold16[:, it:it + 1]))]
    rr = max(_row_rel(tr[-1], ref[-1]))
    record('sd15_dpmpp2m_b15_fp16', golden_slots=slots, per_step_vs_fp32_golden=errs, per_step_vs_fp16_oracle=errs16, oracle_noise_per_step=noise,
           worst_row_vs_b16=rr)
    assert errs[0] < 1e-6
    for i in range(1, len(errs)):
        assert errs[i] < min(max(1.5 * noise[i], 2e-3), 2e-2), (i, errs[i], noise[i])
        assert errs16[i] < max(2.0 * noise[i], 2e-3), (i, errs16[i], noise[i])
    assert rr < 1e-2, rr
