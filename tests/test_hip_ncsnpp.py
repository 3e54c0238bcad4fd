"""GPU: the NCSN++ networks (Fourier embedding, residual encoder, [1,3,3,1] resampling) on the engine against goldens recorded from the
reference classes (tools/gen_ncsnpp_golden.py) and against the functional restatement (tests/_ncsnpp_ref.py).

Metric and bound are the denoiser's own (tests/test_hip_denoiser.py): max |a - b| / max |b| < 2e-4 per evaluation, for the per-sample and the
scalar sigma form.  The Fourier argument c_noise * 2 pi freqs reaches a few hundred radians, so one ulp of the device logf moves an
embedding entry by ~3e-5; `_report` prints every observed value next to the bound.  Observed on the MI355X: out_vec /
out_scalar 1.1e-6 / 6.3e-8 (tiny_ncsnpp), 1.0e-6 / 6.0e-8 (tiny_ncsnpp_cond), 1.1e-6 / 6.9e-8 (cifar10_ve), 7.8e-7 / 5.9e-8 (ffhq_ve); worst skip
tap 1.2e-6; mixed configs 1.6e-6; sampler steps 1.1e-6 (dpm_pp 2M) and 6.4e-6 (Heun) -- the embedding does not show, the bound stays 2e-4.
"""
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import diff_sampler_amd.arch as arch  # noqa: E402
import _ncsnpp_ref as R  # noqa: E402
import _ref_like_ncsnpp as duck  # noqa: E402
from _parity import per_step_rel  # noqa: E402

pytestmark = pytest.mark.gpu
G = os.path.join(ROOT, 'tests', 'golden')
TOL = 2e-4
MIXED = {'positional_residual_fir': dict(arch.NAMED_CONFIGS['tiny_ncsnpp'], embedding_type='positional', channel_mult_noise=1),
         'fourier_standard_box': dict(arch.NAMED_CONFIGS['tiny_ncsnpp'], encoder_type='standard', resample_filter=[1, 1])}


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


def _report(what, value, bound=TOL):
    print(f'ncsnpp parity: {what}: {value:.3e} (bound {bound:.0e})')
    return value


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda')


def _skip_taps(net, spec, B):
    """{name: NCHW tensor} of the skip stack of the last evaluation: an aux_residual entry replaces its down block's."""
    plan = net.engine.plan(B, B)
    names = []
    for b in spec.enc:
        if b.kind == 'aux':
            names[-1] = b
        else:
            names.append(b)
    return {b.name: plan.bufs[b.name][:B * b.res_out ** 2 * b.cout].reshape(B, b.res_out, b.res_out, b.cout).permute(0, 3, 1, 2).cpu() for b in names}


@pytest.mark.parametrize('name', ['tiny_ncsnpp', 'tiny_ncsnpp_cond', 'cifar10_ve', 'ffhq_ve'])
def test_denoiser_matches_reference_golden(name, dev):
    from diff_sampler_amd.engine import EDMDenoiser
    z = np.load(os.path.join(G, f'ncsnpp_net_{name}.npz'))
    net = EDMDenoiser.from_config(name, seed=int(z['seed']))
    spec = net.spec
    assert net.engine.plan(2, 2).foreign and spec.ncsnpp
    x = torch.from_numpy(z['x']).to(dev)
    B = x.shape[0]
    lab = torch.from_numpy(z['labels']).to(dev) if z['labels'].size else None
    out_vec = net(x, torch.from_numpy(z['sigma']).to(dev), class_labels=lab)
    torch.cuda.synchronize()
    taps = _skip_taps(net, spec, B) if name.startswith('tiny') else {}
    out_sc = net(x, torch.tensor(0.6), class_labels=lab)
    torch.cuda.synchronize()
    e_vec = _report(f'{name} out_vec', _rel(out_vec.cpu(), torch.from_numpy(z['out_vec'])))
    e_sc = _report(f'{name} out_scalar', _rel(out_sc.cpu(), torch.from_numpy(z['out_scalar'])))
    # every skip-stack tensor of the tiny nets (after the aux replacement): localises a wrong aux layer or filter
    worst = {k: _rel(t, torch.from_numpy(z['tap_' + k])) for k, t in taps.items()}
    if taps:
        assert sorted(taps) == sorted(k[4:] for k in z.files if k.startswith('tap_'))
        _report(f'{name} worst skip tap ({max(worst, key=worst.get)})', max(worst.values()))
    assert all(v < TOL for v in worst.values()), worst
    assert e_vec < TOL and e_sc < TOL, (e_vec, e_sc)


@pytest.mark.parametrize('name', sorted(MIXED))
def test_mixed_configs_match_the_restatement(name, dev):
    """(positional, residual, [1,3,3,1]) and (fourier, standard, [1,1]): the options are independent of each other."""
    from diff_sampler_amd.engine import EDMDenoiser
    kw = MIXED[name]
    spec = arch.edm_precond_spec(**kw)
    params = arch.init_params(spec, seed=31)
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(32))
    sig = torch.tensor([9.0, 0.3])
    x = x * sig.reshape(-1, 1, 1, 1)
    ref = R.edm_ncsnpp(params, spec, x, sig)
    net = EDMDenoiser(spec, params)
    out = net(x.to(dev), sig.to(dev))
    torch.cuda.synchronize()
    assert _report(f'{name} vs restatement', _rel(out.cpu(), ref)) < TOL


def test_from_reference_module_equals_from_config(dev):
    from diff_sampler_amd.engine import EDMDenoiser
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(4)).to(dev) * 3
    sig = torch.tensor([3.0, 0.5]).to(dev)
    a = EDMDenoiser.from_config('tiny_ncsnpp', seed=6)
    b = EDMDenoiser.from_reference_module(duck.build('tiny_ncsnpp', seed=6))
    assert b.spec == a.spec and b.spec.embedding_type == 'fourier' and b.spec.encoder_type == 'residual'
    oa, ob = a(x, sig), b(x, sig)
    torch.cuda.synchronize()
    assert torch.equal(oa, ob)


def test_sampler_trajectories_match_the_reference(dev):
    """dpm_pp_sampler (2M, x0 form, 6 steps) and heun_sampler (4 steps) on tiny_ncsnpp against the reference's solvers.py: every step within
    5e-4 of that step's own scale, the bound of the fp32 EDM trajectory tests (tests/test_hip_full_goldens.py)."""
    from diff_sampler_amd import solvers
    from diff_sampler_amd.engine import EDMDenoiser
    z = np.load(os.path.join(G, 'ncsnpp_sampler_tiny.npz'))
    net = EDMDenoiser.from_config('tiny_ncsnpp', seed=int(z['seed']))
    lat = torch.from_numpy(z['latents']).to(dev)
    runs = {'dpmpp2m': (solvers.dpm_pp_sampler, dict(num_steps=6, schedule_type='logsnr', schedule_rho=7, max_order=2, predict_x0=True,
                                                      lower_order_final=True)),
            'heun': (solvers.heun_sampler, dict(num_steps=4, schedule_type='polynomial', schedule_rho=7))}
    for tag, (fn, kw) in runs.items():
        tr = fn(net, lat, sigma_min=0.002, sigma_max=80., return_inters=True, **kw)
        torch.cuda.synchronize()
        errs = per_step_rel(tr.cpu(), torch.from_numpy(z[tag]))
        _report(f'sampler {tag} worst step', max(errs), 5e-4)
        assert max(errs) < 5e-4 and errs[-1] < 5e-4, (tag, errs)


def test_graphed_sampler_equals_eager(dev):
    """Whole-sampler capture (torch.cuda.CUDAGraph) of a plan that runs through Plan.run_python: replay == eager, bit for bit, twice."""
    from diff_sampler_amd import solvers
    from diff_sampler_amd.engine import EDMDenoiser
    from diff_sampler_amd.graph import GraphedSampler
    net = EDMDenoiser.from_config('tiny_ncsnpp', seed=9)
    kw = dict(num_steps=5, max_order=2, schedule_type='logsnr')
    g = GraphedSampler(solvers.dpm_pp_sampler, net, (2, 3, 32, 32), **kw)
    gen = torch.Generator().manual_seed(0)
    for trial in range(2):
        lat = torch.randn(2, 3, 32, 32, generator=gen).to(dev)
        eager = solvers.dpm_pp_sampler(net, lat, **kw)
        graphed = g(lat)
        torch.cuda.synchronize()
        assert torch.equal(eager, graphed), trial


def test_amed_bottleneck_tap_and_block_outputs(dev):
    """block_output names and the AMED bottleneck tap are those of DDPM++ ('enc.8x8_block3' of a 4-block net)."""
    from diff_sampler_amd.engine import EDMDenoiser
    kw = dict(arch.NAMED_CONFIGS['tiny_ncsnpp'], num_blocks=4)
    spec = arch.edm_precond_spec(**kw)
    params = arch.init_params(spec, seed=12)
    net = EDMDenoiser(spec, params)
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(13)) * 2
    sig = torch.tensor([2.0, 0.4])
    taps = {}
    R.edm_ncsnpp(params, spec, x, sig, taps=taps)
    net(x.to(dev), sig.to(dev))
    got = net.block_output('enc.8x8_block3')
    mean = net.bottleneck_mean(net._last[0], 2, class_cond=False)
    torch.cuda.synchronize()
    assert tuple(got.shape) == tuple(taps['enc.8x8_block3'].shape) == (2, 64, 8, 8)
    assert _rel(got.cpu(), taps['enc.8x8_block3']) < TOL
    assert _rel(mean.cpu(), taps['enc.8x8_block3'].mean(dim=1)) < TOL
    assert _rel(net.block_output('enc.16x16_aux_residual').cpu(), taps['enc.16x16_aux_residual']) < TOL


# launch-list hashes (tools/plan_dump.py rows: every argument of every launch, pointers replaced by what they point at, plus the library's
# routing answers) of the plans the NCSN++ work must not touch, recorded on the commit before it: (rows, sha256 of the row records)
PARENT_PLANS = {('edm', 'cifar10', 4): {'/rows=4': (178, 'be6e8ed302cc5e59371ecb0e094cb523'), '/rows=1': (178, '85e40ac6578a44d0062ba83f8dbc4234')},
                ('edm', 'ffhq', 2): {'/rows=2': (226, 'd82222054be0ea45e617b7d1e5b72acb'), '/rows=1': (226, 'e94891334fb2e8c8c06d3f681c05e62b')},
                ('edm', 'imagenet64', 2): {'/rows=2': (275, '848694acb987887e46d7a352267f9948')},
                ('ldm', 'sd15', 1): {'/rows=2': (361, '1bce91e815afb2e5d9255daa8fd005f0'), '/rows=1': (361, '284b656dc531f38a641d9316c4f5b449')}}


@pytest.mark.parametrize('key', sorted(PARENT_PLANS), ids=lambda k: '-'.join(map(str, k)))
def test_existing_plans_hash_as_before(key):
    import plan_dump as pd
    kind, net, B = key
    eng = pd.make_engine(kind, net, 'fp32')
    for suffix, P in pd.build_plans(eng, kind, '-', B):
        assert not P.foreign
        rows = [pd.row_record(*r) for r in pd.dump(eng, P)]
        got = (len(rows), hashlib.sha256('\n'.join(rows).encode()).hexdigest()[:32])
        print(f'plan {kind}/{net}/fp32/-/B={B}{suffix}: {got}')
        want = PARENT_PLANS[key][suffix]
        assert want is not None and got == want, (key, suffix, got, want)
