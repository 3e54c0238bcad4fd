"""GPU: SFD's step-conditioned EDM networks on the engine against goldens recorded from the reference classes (tools/gen_sfd_golden.py).

Metric and bound are the denoiser's own (tests/test_hip_denoiser.py): max |a - b| / max |b| < 2e-4 per evaluation for the exact modes, the fp16
mode's 5e-3 against the fp32 reference (tests/test_hip_fp16.py), every trajectory step within 5e-4 of that step's own scale
(tests/test_hip_full_goldens.py).  The goldens separate `no step` / 4 / 6 by 10 - 40 % of the output scale (asserted by the generator and by
tests/test_sfd_cpu.py), so none of these can pass with the condition ignored or frozen.  `_report` prints every observed value next to its bound.
"""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import diff_sampler_amd.arch as arch  # noqa: E402
import _sfd_ref as R  # noqa: E402
import _ref_like_sfd as duck  # noqa: E402
from _parity import per_step_rel, rel  # noqa: E402

pytestmark = pytest.mark.gpu
G = os.path.join(ROOT, 'tests', 'golden')
TOL = 2e-4
OUTS = ('out_none', 'out_step4', 'out_step6')


def _report(what, value, bound=TOL):
    print(f'sfd parity: {what}: {value:.3e} (bound {bound:.0e})')
    return value


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need the MI355X'
    return torch.device('cuda')


def _golden(name, dev):
    z = np.load(os.path.join(G, f'sfd_net_{name}.npz'))
    x, sig = torch.from_numpy(z['x']).to(dev), torch.from_numpy(z['sigma']).to(dev)
    lab = torch.from_numpy(z['labels']).to(dev) if z['labels'].size else None
    return z, x, sig, lab


def _errors(net, z, x, sig, lab, scalar=True):
    """{golden key: rel} of one denoiser over the recorded evaluations: no step, 4 and 6 with the per-sample sigma, 4 with the scalar one."""
    e = {}
    for key, step in (('out_none', None), ('out_step4', 4), ('out_step6', 6)):
        out = net(x, sig, class_labels=lab, step_condition=step)
        torch.cuda.synchronize()
        e[key] = rel(out.cpu(), z[key])
    if scalar:
        out = net(x, torch.tensor(0.6), class_labels=lab, step_condition=torch.tensor([4.0]))
        torch.cuda.synchronize()
        e['out_step4_scalar'] = rel(out.cpu(), z['out_step4_scalar'])
    return e


@pytest.mark.parametrize('name', ['tiny_song', 'tiny_song_cond', 'tiny_adm', 'tiny_ncsnpp', 'cifar10', 'imagenet64'])
def test_denoiser_matches_reference_golden(name, dev):
    from diff_sampler_amd.engine import EDMDenoiser
    z, x, sig, lab = _golden(name, dev)
    net = EDMDenoiser.from_config(name, seed=int(z['seed']), step_condition=True)
    e = _errors(net, z, x, sig, lab)
    for k, v in e.items():
        _report(f'{name} {k}', v)
    assert max(e.values()) < TOL, e
    # the three evaluations are three different results on the device too
    a, b = net(x, sig, class_labels=lab, step_condition=4).clone(), net(x, sig, class_labels=lab, step_condition=6).clone()
    c = net(x, sig, class_labels=lab).clone()
    torch.cuda.synchronize()
    assert rel(a, c) > 1e-2 and rel(a, b) > 2e-3


@pytest.mark.parametrize('name,kw,bound', [('cifar10', dict(winograd=False), 2e-4), ('cifar10', dict(split_fp16=True), 2e-4),
                                           ('cifar10', dict(up_phase=False), 2e-4),
                                           ('imagenet64', dict(use_fp16=True, fuse=False), 5e-3), ('imagenet64', dict(use_fp16=True, fuse=True), 5e-3)],
                         ids=['cifar10-direct', 'cifar10-split', 'cifar10-no_up_phase', 'imagenet64-fp16-fuse0', 'imagenet64-fp16-fuse1'])
def test_modes_match_the_same_golden(name, kw, bound, dev):
    from diff_sampler_amd.engine import EDMDenoiser
    kw = dict(kw)
    fuse = kw.pop('fuse', None)
    z, x, sig, lab = _golden(name, dev)
    net = EDMDenoiser.from_config(name, seed=int(z['seed']), step_condition=True, **kw)
    if fuse is not None:
        net.engine.fuse_norm16 = fuse
    e = _errors(net, z, x, sig, lab)
    for k, v in e.items():
        _report(f'{name} {kw} fuse={fuse} {k}', v, bound)
    assert max(e.values()) < bound, e


@pytest.mark.parametrize('name', ['tiny_song', 'tiny_adm'])
def test_euler_trajectories_match_the_reference(name, dev):
    from diff_sampler_amd import solvers
    from diff_sampler_amd.engine import EDMDenoiser
    z = np.load(os.path.join(G, 'sfd_sampler_tiny.npz'))
    net = EDMDenoiser.from_config(name, seed=int(z[f'{name}_seed']), step_condition=True)
    lat = torch.from_numpy(z[f'{name}_latents']).to(dev)
    lab = torch.from_numpy(z[f'{name}_labels']).to(dev) if z[f'{name}_labels'].size else None
    for tag, kw in (('afs4', dict(afs=True, num_steps=4)), ('plain3', dict(afs=False, num_steps=3))):
        tr = solvers.euler_sampler(net, lat, class_labels=lab, sigma_min=0.002, sigma_max=80., schedule_type='polynomial', schedule_rho=7,
                                   step_condition=4, return_inters=True, **kw)
        torch.cuda.synchronize()
        errs = per_step_rel(tr.cpu(), torch.from_numpy(z[f'{name}_{tag}']))
        _report(f'euler {name} {tag} worst step', max(errs), 5e-4)
        assert max(errs) < 5e-4 and errs[-1] < 5e-4, (tag, errs)
        # without the condition the sampler lands elsewhere: the keyword reaches the evaluations
        other = solvers.euler_sampler(net, lat, class_labels=lab, sigma_min=0.002, sigma_max=80., return_inters=True, **kw)
        torch.cuda.synchronize()
        assert rel(other[-1].cpu(), z[f'{name}_{tag}'][-1]) > 1e-2


def test_denoise_to_zero_evaluation_gets_no_step_condition(dev):
    """sfd-main/solvers.py:95: the last evaluation is the plain one."""
    from diff_sampler_amd import solvers
    from diff_sampler_amd.engine import EDMDenoiser
    net = EDMDenoiser.from_config('tiny_song', seed=3, step_condition=True)
    lat = torch.randn(2, 3, 16, 16, generator=torch.Generator().manual_seed(4)).to(dev)
    tr = solvers.euler_sampler(net, lat, num_steps=3, step_condition=4, denoise_to_zero=True, return_inters=True)
    last = tr[-2].contiguous()
    want = net(last, torch.tensor(0.002), step_condition=None)
    torch.cuda.synchronize()
    assert rel(tr[-1], want) < 1e-6 and rel(tr[-1], net(last, torch.tensor(0.002), step_condition=4)) > 1e-3


@pytest.mark.parametrize('name', ['tiny_adm', 'cifar10'])
def test_batch_invariant_bits_with_a_step_condition(name, dev):
    from diff_sampler_amd.engine import EDMDenoiser
    net = EDMDenoiser.from_config(name, seed=5, step_condition=True, batch_invariant=True)
    R_ = net.img_resolution
    g = torch.Generator().manual_seed(6)
    x = (torch.randn(3, 3, R_, R_, generator=g) * 2).to(dev)
    sig = torch.tensor([2.0, 0.7, 11.0]).to(dev)
    lab = torch.eye(net.label_dim)[torch.tensor([1, 4, 7])].to(dev) if net.label_dim else None
    full = net(x, sig, class_labels=lab, step_condition=4).clone()
    one = net(x[:1].contiguous(), sig[:1].contiguous(), class_labels=(lab[:1] if lab is not None else None), step_condition=4).clone()
    torch.cuda.synchronize()
    assert torch.equal(full[0], one[0])
    assert not torch.equal(full[0], net(x[:1].contiguous(), sig[:1].contiguous(), class_labels=(lab[:1] if lab is not None else None))[0])


@pytest.mark.parametrize('name', ['tiny_song', 'tiny_adm'])
def test_native_plan_walk_equals_the_python_walk(name, dev):
    from diff_sampler_amd import _lib
    from diff_sampler_amd.engine import EDMDenoiser
    z, x, sig, lab = _golden(name, dev)
    net = EDMDenoiser.from_config(name, seed=int(z['seed']), step_condition=True)
    plan, _ = net._prepare(x, sig, lab, 4.0)
    assert not plan.foreign and 'step' in plan.bufs
    plan.run(_lib.stream_ptr())
    a = plan.bufs['out'].clone()
    aff_a = plan.bufs['aff'].clone()
    plan.bufs['out'].zero_()
    plan.run_python(_lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.equal(a, plan.bufs['out']) and torch.equal(aff_a, plan.bufs['aff']) and bool(a.abs().max() > 0)


@pytest.mark.parametrize('name', ['tiny_song', 'tiny_adm'])
def test_graphed_sampler_equals_eager(name, dev):
    from diff_sampler_amd import solvers
    from diff_sampler_amd.engine import EDMDenoiser
    from diff_sampler_amd.graph import GraphedSampler
    net = EDMDenoiser.from_config(name, seed=9, step_condition=True)
    kw = dict(step_condition=4, afs=True, num_steps=4)
    g = GraphedSampler(solvers.euler_sampler, net, (2, 3, 16, 16), **kw)
    gen = torch.Generator().manual_seed(0)
    for trial in range(2):
        lat = torch.randn(2, 3, 16, 16, generator=gen).to(dev)
        eager = solvers.euler_sampler(net, lat, **kw)
        graphed = g(lat)
        torch.cuda.synchronize()
        assert torch.equal(eager, graphed), trial


@pytest.mark.parametrize('name', ['tiny_song', 'tiny_adm', 'tiny_ncsnpp'])
def test_from_reference_module_equals_from_config_and_none_equals_a_plain_engine(name, dev):
    from diff_sampler_amd.engine import EDMDenoiser
    z, x, sig, lab = _golden(name, dev)
    a = EDMDenoiser.from_config(name, seed=6, step_condition=True)
    b = EDMDenoiser.from_reference_module(duck.build(name, seed=6))
    assert b.spec == a.spec and b.spec.step_condition
    oa, ob = a(x, sig, class_labels=lab, step_condition=4), b(x, sig, class_labels=lab, step_condition=4)
    torch.cuda.synchronize()
    assert torch.equal(oa, ob)
    # None on the step-capable engine == an engine built from the same weights without the step keys
    plain_spec = arch.edm_precond_spec(**arch.NAMED_CONFIGS[name])
    keep = {k for k, _, _ in arch.param_table(plain_spec)}
    plain = EDMDenoiser(plain_spec, {k: v for k, v in arch.init_params(a.spec, seed=6).items() if k in keep})
    on, op = a(x, sig, class_labels=lab), plain(x, sig, class_labels=lab)
    torch.cuda.synchronize()
    assert torch.equal(on, op) and not torch.equal(on, oa)


# ---- the compose kernel alone ---------------------------------------------------------------------------------------------------------------
GAP_BLOCKS = [(0, 32), (72, 48), (176, 192)]          # couts 32 / 48 / 192; columns 64..71 and 168..175 belong to no block; width 560
WIDTH, LD = 560, 564                                   # four padding columns behind every row


@pytest.mark.parametrize('rows', [1, 3])
def test_affine_compose_kernel(rows, dev):
    from diff_sampler_amd import _lib
    g = torch.Generator().manual_seed(60 + rows)
    vals = torch.randn(rows, LD, generator=g) * 0.7
    step = torch.randn(WIDTH, generator=g) * 0.7
    vals[:, 5], step[3] = -1.0 + 2.0 ** -20, -1.0 + 2.0 ** -18           # near-cancelling 1 + s / 1 + ss
    touched = torch.zeros(LD, dtype=torch.bool)
    for off, c in GAP_BLOCKS:
        touched[off:off + 2 * c] = True
    assert int(touched.sum()) == 2 * (32 + 48 + 192) and int((~touched).sum()) == 8 + 8 + 4
    aff = torch.where(touched, vals, torch.full_like(vals, float('nan')))
    ref, bound = R.compose_ref64(torch.where(touched, vals, torch.zeros_like(vals)), torch.cat([step, torch.zeros(LD - WIDTH)]), GAP_BLOCKS)
    d_aff, d_step, d_pairs = aff.to(dev), step.to(dev), R.compose_pairs(GAP_BLOCKS).to(dev)
    a = _lib.AffineComposeArgs(d_aff.data_ptr(), LD, rows, WIDTH, d_step.data_ptr(), d_pairs.data_ptr(), d_pairs.shape[0])
    _lib.run_op(_lib.DS_OP_AFFINE_COMPOSE, a, 'DS_OP_AFFINE_COMPOSE')
    torch.cuda.synchronize()
    got = d_aff.cpu()
    assert bool(torch.isnan(got[:, ~touched]).all()) and not bool(torch.isnan(got[:, touched]).any())
    err = (got.double() - ref).abs()[:, touched]
    ratio = float((err / bound[:, touched].clamp_min(1e-300)).max())
    _report(f'affine_compose rows={rows}: worst err / bound', ratio, 1.0)
    assert ratio <= 1.0
    # a table entry outside the width, or off the four-column grid, is skipped: nothing is written out of bounds
    bad = torch.tensor([[WIDTH, 0], [0, WIDTH - 2], [-4, 8], [2, 8]], dtype=torch.int32).to(dev)
    d2 = aff.to(dev)
    b = _lib.AffineComposeArgs(d2.data_ptr(), LD, rows, WIDTH, d_step.data_ptr(), bad.data_ptr(), 4)
    _lib.run_op(_lib.DS_OP_AFFINE_COMPOSE, b, 'DS_OP_AFFINE_COMPOSE')
    torch.cuda.synchronize()
    back = d2.cpu()
    assert torch.equal(back[:, touched], aff[:, touched]) and bool(torch.isnan(back[:, ~touched]).all())


# ---- the routes a user takes: the persistence hook and the command line -----------------------------------------------------------------------
def test_persistence_route_takes_the_step_condition(dev):
    """A routed module with map_step_layer0: forward(..., step_condition=v) runs on the engine (before: any model_kwargs meant the reference forward)."""
    from diff_sampler_amd import persistence_hook as hook
    from diff_sampler_amd.engine import EDMDenoiser
    z, x, sig, lab = _golden('tiny_adm', dev)
    net = duck.build('tiny_adm', seed=int(z['seed']))
    net.__class__ = type('EDMPrecond', (net.__class__,), {})
    hook.route_class(net.__class__)
    out = net(x, sig, class_labels=lab, step_condition=4, skip_tuning=False)
    torch.cuda.synchronize()
    assert _report('routed tiny_adm out_step4', rel(out.cpu(), z['out_step4'])) < TOL
    assert rel(net(x, sig, class_labels=lab).cpu(), z['out_none']) < TOL
    with pytest.raises(NotImplementedError, match='not routed'):          # the duck's own forward: where skip_tuning=True goes
        net(x, sig, class_labels=lab, step_condition=4, skip_tuning=True)
    ref = EDMDenoiser.from_config('tiny_adm', seed=int(z['seed']), step_condition=True)
    assert torch.equal(out, ref(x, sig, class_labels=lab, step_condition=4))


def _pngs(root):
    import PIL.Image
    found = {}
    for d, _, files in os.walk(root):
        for f in files:
            if f.endswith('.png'):
                found[f] = np.asarray(PIL.Image.open(os.path.join(d, f)))
    return found


def _direct_images(net, seeds, dev, **kw):
    """What sample.run computes for these seeds, called directly: seeded latents, the Euler sampler, the uint8 conversion."""
    from diff_sampler_amd import sample, solvers
    rnd = sample.StackedRandomGenerator(dev, seeds)
    lat = rnd.randn([len(seeds), 3, 16, 16], device=dev)
    img = solvers.euler_sampler(net, lat, sigma_min=net.sigma_min, sigma_max=net.sigma_max, **kw)
    from diff_sampler_amd import ops
    B, C, H, W = img.shape
    u8 = torch.empty(B, H, W, C, dtype=torch.uint8, device=img.device)
    ops.quantize_u8_nhwc(img.contiguous(), u8, B, C, H, W)          # the conversion sample.save_images makes (sample.py:311 of the reference)
    return u8.cpu().numpy()


def test_cli_random_sfd_net(dev, tmp_path, monkeypatch):
    from diff_sampler_amd import sample
    from diff_sampler_amd.engine import EDMDenoiser
    monkeypatch.chdir(tmp_path)          # the default output tree is relative: ./samples/<dataset>/euler_step<N>_nfe<nfe>
    out, n = sample.run(sfd_path='random:3', dataset_name='tiny_song', num_steps=4, afs=True, seeds='0-3', max_batch_size=4)
    assert n == 4 and os.path.normpath(out) == os.path.join('samples', 'tiny_song', 'euler_step4_nfe2')
    got = _pngs(out)
    assert sorted(got) == [f'{i:06d}.png' for i in range(4)]
    net = EDMDenoiser.from_config('tiny_song', seed=3, step_condition=True)
    want = _direct_images(net, [0, 1, 2, 3], dev, num_steps=4, afs=True, step_condition=4)
    for i in range(4):
        assert np.array_equal(got[f'{i:06d}.png'], want[i]), i
    plain = _direct_images(net, [0, 1, 2, 3], dev, num_steps=4, afs=True)
    assert not np.array_equal(plain, want)


def test_cli_pickled_sfd_net_training_kwargs_override_the_cli(dev, tmp_path, monkeypatch):
    import pickle
    from diff_sampler_amd import sample
    from diff_sampler_amd.engine import EDMDenoiser
    tk = dict(dataset_name='tiny_song', guidance_type=None, guidance_rate=None, afs=True, schedule_type='polynomial', schedule_rho=5, model_source='edm',
              sigma_min=0.01, sigma_max=40.0, use_step_condition=True, num_steps=9)
    pkl = tmp_path / 'sfd.pkl'
    with open(pkl, 'wb') as f:
        pickle.dump({'model': duck.build('tiny_song', seed=3, training_kwargs=tk)}, f)
    # the CLI says afs False, rho 7: the snapshot wins; num_steps is the CLI's because the net is step-conditioned
    monkeypatch.chdir(tmp_path)
    out, n = sample.run(sfd_path=str(pkl), dataset_name='tiny_song', num_steps=4, afs=False, schedule_rho=7, seeds='0-3', max_batch_size=4)
    assert n == 4 and os.path.normpath(out) == os.path.join('samples', 'tiny_song', 'euler_step4_nfe2')
    got = _pngs(out)
    net = EDMDenoiser.from_config('tiny_song', seed=3, step_condition=True)
    net.sigma_min, net.sigma_max = 0.01, 40.0
    want = _direct_images(net, [0, 1, 2, 3], dev, num_steps=4, afs=True, schedule_rho=5, step_condition=4)
    for i in range(4):
        assert np.array_equal(got[f'{i:06d}.png'], want[i]), i
    with pytest.raises(ValueError, match='distilled on'):
        sample.run(sfd_path=str(pkl), dataset_name='cifar10', num_steps=4, seeds='0-3', outdir=str(tmp_path / 'x'))
    # a snapshot distilled for one step count without the condition: num_steps is the snapshot's, no step value is passed
    tk2 = dict(tk, use_step_condition=False, num_steps=3, afs=False)
    with open(pkl, 'wb') as f:
        pickle.dump({'model': duck.build('tiny_song', seed=3, training_kwargs=tk2)}, f)
    out2, _ = sample.run(sfd_path=str(pkl), dataset_name='tiny_song', num_steps=4, seeds='0-1')
    assert os.path.normpath(out2) == os.path.join('samples', 'tiny_song', 'euler_step3_nfe2')
    want2 = _direct_images(net, [0, 1], dev, num_steps=3, afs=False, schedule_rho=5)
    got2 = _pngs(out2)
    assert np.array_equal(got2['000000.png'], want2[0]) and np.array_equal(got2['000001.png'], want2[1])


# ---- the latent-diffusion U-Net under classifier-free guidance ---------------------------------------------------------------------------------
def test_ldm_cfg_denoiser_and_euler_trajectory_match_the_reference(dev):
    """tiny_ldm_1res, B = 3, guidance 7.5 (one step row serves both halves of the doubled evaluation): the bounds of tests/test_hip_ldm.py --
    2e-4 of the output scale per evaluation, 1e-3 for the trajectory."""
    from diff_sampler_amd import solvers
    from diff_sampler_amd.ldm_engine import CFGDenoiser
    z = np.load(os.path.join(G, 'sfd_ldm_tiny.npz'))
    net = CFGDenoiser.from_config('tiny_ldm_1res', seed=int(z['seed']), guidance_rate=7.5, step_condition=True)
    x, sig, cond, uncond, lat = (torch.from_numpy(z[k]).to(dev) for k in ('x', 'sigma', 'cond', 'uncond', 'latents'))
    outs = {}
    for key, step in (('out_none', None), ('out_step4', 4), ('out_step6', torch.tensor([6.0, 6.0, 6.0]))):
        outs[key] = net(x, sig, condition=cond, unconditional_condition=uncond, step_condition=step).clone()
        torch.cuda.synchronize()
        assert _report(f'ldm tiny_ldm_1res {key}', rel(outs[key].cpu(), z[key])) < TOL, key
    assert rel(outs['out_step4'], outs['out_none']) > 1e-2 and rel(outs['out_step4'], outs['out_step6']) > 2e-3
    kw = dict(condition=cond, unconditional_condition=uncond, num_steps=4, sigma_min=net.sigma_min, sigma_max=net.sigma_max,
              schedule_type='discrete', schedule_rho=1, return_inters=True)
    tr = solvers.euler_sampler(net, lat, step_condition=4, **kw)
    torch.cuda.synchronize()
    assert tr.shape == z['traj_euler'].shape
    assert _report('ldm euler trajectory', rel(tr.cpu(), z['traj_euler']), 1e-3) < 1e-3
    assert rel(solvers.euler_sampler(net, lat, **kw)[-1].cpu(), z['traj_euler'][-1]) > 1e-2
    # None on the step-capable engine == an engine built from the same weights without the step keys, bit for bit
    import diff_sampler_amd.ldm_arch as la
    plain_spec = la.ldm_unet_spec(**la.NAMED_LDM_CONFIGS['tiny_ldm_1res'])
    params = la.init_ldm_params(net.spec, seed=int(z['seed']))
    plain = CFGDenoiser(plain_spec, {k: params[k] for k, _, _ in la.ldm_param_table(plain_spec)}, guidance_rate=7.5)
    assert torch.equal(plain(x, sig, condition=cond, unconditional_condition=uncond), outs['out_none'])
    with pytest.raises(ValueError, match='step'):
        plain(x, sig, condition=cond, unconditional_condition=uncond, step_condition=4)


def test_cli_pickled_ms_coco_snapshot_feeds_the_cfg_denoiser(dev, tmp_path, monkeypatch):
    """sfd-main/sample.py on an ms_coco snapshot: `{'model': CFGPrecond}` whose LatentDiffusion state dict (`model.diffusion_model.*`) builds the
    CFGDenoiser, guidance / afs / schedule / sigma range from training_kwargs, NFE doubled by the guidance: (4 - 2) * 2 = 4.  One latent file
    per seed, equal to the direct sampler call on the same seeded latents and conditions."""
    import pickle
    from diff_sampler_amd import sample, solvers
    from diff_sampler_amd.ldm_engine import CFGDenoiser
    tk = dict(dataset_name='ms_coco', guidance_type='cfg', guidance_rate=5.0, afs=True, schedule_type='discrete', schedule_rho=1, model_source='ldm',
              sigma_min=0.1, sigma_max=10.0, use_step_condition=True, num_steps=9)
    pkl = tmp_path / 'sfd_ldm.pkl'
    with open(pkl, 'wb') as f:
        pickle.dump({'model': duck.build_ldm('tiny_ldm_1res', seed=7, training_kwargs=tk)}, f)
    monkeypatch.chdir(tmp_path)
    out, n = sample.run(sfd_path=str(pkl), dataset_name='ms_coco', num_steps=4, afs=False, guidance_rate=7.5, schedule_type='polynomial', seeds='0-2',
                        max_batch_size=3)
    assert n == 3 and os.path.normpath(out) == os.path.join('samples', 'ms_coco', 'euler_step4_nfe4')
    got = {f: np.load(os.path.join(d, f)) for d, _, files in os.walk(out) for f in files if f.endswith('.npy')}
    assert sorted(got) == ['000000.npy', '000001.npy', '000002.npy']
    net = CFGDenoiser.from_config('tiny_ldm_1res', seed=7, guidance_rate=5.0, step_condition=True)
    net.sigma_min, net.sigma_max = 0.1, 10.0
    rnd = sample.StackedRandomGenerator(dev, [0, 1, 2])
    lat = rnd.randn([3, 4, 16, 16], device=dev)
    c = rnd.randn([3, 77, 64], device=dev)
    uc = torch.randn(1, 77, 64, generator=torch.Generator().manual_seed(0)).to(dev).expand(3, -1, -1)
    kw = dict(condition=c, unconditional_condition=uc, num_steps=4, afs=True, sigma_min=0.1, sigma_max=10.0, schedule_type='discrete', schedule_rho=1)
    want = solvers.euler_sampler(net, lat, step_condition=4, **kw).cpu().numpy()
    for i in range(3):
        assert np.array_equal(got[f'{i:06d}.npy'], want[i]), i
    assert not np.array_equal(solvers.euler_sampler(net, lat, **kw).cpu().numpy(), want)           # the step value reached the evaluations
    with pytest.raises(ValueError, match='distilled on'):
        sample.run(sfd_path=str(pkl), dataset_name='cifar10', num_steps=4, seeds='0-2')
