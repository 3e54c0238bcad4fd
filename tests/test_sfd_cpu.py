"""CPU-only: SFD's step-conditioned EDM networks (``UNetSpec.step_condition``) as data model, launch plan and host-side library surface.

  * tests/_sfd_ref.py -- the functional restatement -- equals the goldens recorded from the reference classes (tools/gen_sfd_golden.py) at the fp32
    bound of the NCSN++ restatement (1e-6), with no step, step 4 (both sigma forms) and step 6, and for the Euler trajectories.
  * ``param_table`` lists the reference's state-dict keys and shapes in its order; a spec without the flag keeps its keys and its bits.
  * ``spec_from_module`` recovers the flag from a module tree, ``from_reference_module`` leaves no state-dict entry over, and a step value on a
    net without step weights raises -- the three things that were silently wrong before.
  * plans: ``step=False`` on a step-capable engine hashes as the plans recorded before the feature; ``step=True`` adds 4 launches (SongUNet) or 5
    (DhariwalUNet); the dtype lint of tests/test_plan_cpu.py holds.
  * the latent-diffusion U-Net (``nfe_embed``, ``emb_nfe_layers``): restatement against the CFGPrecond golden, key list, plan hashes (sd15 B = 1), + 4 launches.
  * ``DS_OP_AFFINE_COMPOSE``: refusals by return code on the host, and its arithmetic (fp32 emulation) inside the derived rounding bound, alone and
    through the consumers' ``(1 + scale') n + shift'`` against the reference's two-stage expression in fp64.
"""
import ctypes as C
import hashlib
import json
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
from diff_sampler_amd import _lib  # noqa: E402
import _sfd_ref as R  # noqa: E402
import _ref_like_sfd as duck  # noqa: E402

G = os.path.join(ROOT, 'tests', 'golden')
CONFIGS = ['tiny_song', 'tiny_song_cond', 'tiny_adm', 'tiny_ncsnpp', 'cifar10', 'imagenet64']
DS_E_ARG, DS_E_ALIGN, DS_E_SHAPE = -1, -2, -3


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


def _spec(name, step=True):
    return arch.edm_precond_spec(**arch.NAMED_CONFIGS[name], step_condition=step)


@pytest.mark.parametrize('name', CONFIGS)
def test_restatement_equals_the_reference_golden(name):
    z = np.load(os.path.join(G, f'sfd_net_{name}.npz'))
    spec = _spec(name)
    params = arch.init_params(spec, seed=int(z['seed']))
    x, sig = torch.from_numpy(z['x']), torch.from_numpy(z['sigma'])
    lab = torch.from_numpy(z['labels']) if z['labels'].size else None
    got = {'out_none': R.edm_sfd(params, spec, x, sig, lab), 'out_step4': R.edm_sfd(params, spec, x, sig, lab, step=4),
           'out_step4_scalar': R.edm_sfd(params, spec, x, torch.tensor(0.6), lab, step=4), 'out_step6': R.edm_sfd(params, spec, x, sig, lab, step=6)}
    e = {k: _rel(v, torch.from_numpy(z[k])) for k, v in got.items()}
    print(f'{name}: restatement vs golden rel = {e}')
    assert max(e.values()) <= 1e-6, e
    # what the generator asserted: the goldens separate none / 4 / 6
    assert _rel(torch.from_numpy(z['out_step4']), torch.from_numpy(z['out_none'])) > 1e-2
    assert _rel(torch.from_numpy(z['out_step4']), torch.from_numpy(z['out_step6'])) > 2e-3


@pytest.mark.parametrize('name', ['tiny_song', 'tiny_adm'])
def test_restated_euler_equals_the_reference_trajectories(name):
    from diff_sampler_amd.solver_utils import get_schedule
    z = np.load(os.path.join(G, 'sfd_sampler_tiny.npz'))
    spec = _spec(name)
    params = arch.init_params(spec, seed=int(z[f'{name}_seed']))
    lat = torch.from_numpy(z[f'{name}_latents'])
    lab = torch.from_numpy(z[f'{name}_labels']) if z[f'{name}_labels'].size else None
    for tag, afs, n in (('afs4', True, 4), ('plain3', False, 3)):
        ts = get_schedule(n, 0.002, 80., device='cpu', schedule_type='polynomial', schedule_rho=7)
        tr = R.euler(params, spec, lat, ts, step=4, afs=afs, labels=lab)
        gold = torch.from_numpy(z[f'{name}_{tag}'])
        assert tuple(tr.shape) == tuple(gold.shape) == (n, 2, 3, 16, 16)
        errs = [_rel(tr[i], gold[i]) for i in range(n)]
        print(f'{name} {tag}: {errs}')
        assert max(errs) <= 1e-6, errs


@pytest.mark.parametrize('name', CONFIGS)
def test_param_table_is_the_reference_state_dict(name):
    z = np.load(os.path.join(G, f'sfd_net_{name}.npz'))
    want = [(k, tuple(s)) for k, s in json.loads(str(z['state_dict']))]
    spec, plain = _spec(name), _spec(name, False)
    got = [(k, tuple(s)) for k, s, _ in arch.param_table(spec)]
    assert got == want
    new = [k for k, _ in got if '.map_step' in k or '.affine_step.' in k]
    nblocks = sum(b.kind == 'block' for b in spec.blocks)
    assert len(new) == 4 + 2 * nblocks + (1 if spec.embedding_type == 'fourier' else 0) >= 24
    # without the flag: the key list of before, and with it every shared tensor keeps its bits
    before = [(k, tuple(s)) for k, s, _ in arch.param_table(plain)]
    assert before == [kv for kv in got if kv[0] not in new]
    if not name.startswith('imagenet'):
        a, b = arch.init_params(plain, seed=3), arch.init_params(spec, seed=3)
        assert list(b) == [k for k, _ in got] and all(torch.equal(a[k], b[k]) for k in a)
        assert all(float(b[k].abs().max()) > 0 for k in new)


# sha256 over (key, bytes) of all tensors of init_params(spec, seed=3), as tests/test_ncsnpp_cpu.py pins them
PINNED = {'cifar10': ('412903fd48f9436b0784ee2617ad304381ac18637f83476b4402db14d5293114', 417),
          'tiny_song': ('7406a0abbb5b7cf578278593a7631e7163c1ee72b77d6b5827819d9efb7d6883', 143)}


@pytest.mark.parametrize('name', sorted(PINNED))
def test_init_params_without_the_flag_keep_their_bits(name):
    sha_all, nkeys = PINNED[name]
    p = arch.init_params(arch.edm_precond_spec(**arch.NAMED_CONFIGS[name]), seed=3)
    h = hashlib.sha256()
    for k in p:
        h.update(k.encode())
        h.update(p[k].numpy().tobytes())
    assert len(p) == nkeys and h.hexdigest() == sha_all


@pytest.mark.parametrize('name', ['tiny_song', 'tiny_song_cond', 'tiny_adm', 'tiny_ncsnpp', 'cifar10'])
def test_spec_from_module_recovers_the_step_condition(name):
    """Fails before the feature: a plain spec came back from such a tree and 24+ state-dict entries were dropped without a word."""
    from diff_sampler_amd.engine import spec_from_module
    net = duck.build(name, seed=2)
    spec = spec_from_module(net)
    assert spec.step_condition is True and spec == _spec(name)
    keys = [k for k in net.state_dict() if 'resample_filter' not in k]
    assert keys == [k for k, _, _ in arch.param_table(spec)]
    assert sum('.affine_step.' in k or '.map_step' in k for k in keys) >= 24


def test_from_reference_module_consumes_every_key_and_refuses_leftovers():
    from diff_sampler_amd.engine import EDMDenoiser, spec_from_module
    net = duck.build('tiny_adm', seed=2)
    den = EDMDenoiser.from_reference_module(net, device='cpu')
    assert den.spec.step_condition and 'affs.w' in den.engine.w and 'step.pairs' in den.engine.w and den.engine.step_adaptive
    song = EDMDenoiser.from_reference_module(duck.build('tiny_song', seed=2), device='cpu')
    assert 'step.pairs' not in song.engine.w and not song.engine.step_adaptive
    # the bias of the step projection carries both layers' (non-adaptive) / its own (adaptive)
    p = arch.init_params(_spec('tiny_song'), seed=2)
    b0 = 'model.enc.16x16_block0'
    assert torch.equal(song.engine.w['affs.b'][:32], p[f'{b0}.affine.bias'] + p[f'{b0}.affine_step.bias'])
    pa = arch.init_params(_spec('tiny_adm'), seed=2)
    assert torch.equal(den.engine.w['affs.b'][:128], pa[f'{b0}.affine_step.bias'])
    # a tree with one group of layers and not the other raises
    for drop in ('map', 'affine'):
        with pytest.raises(ValueError, match='step'):
            spec_from_module(duck.build('tiny_song', seed=2, drop=drop))
    # an entry the spec has no place for is not dropped silently
    net.model.extra_layer = torch.nn.Linear(2, 2)
    with pytest.raises(NotImplementedError, match='extra_layer'):
        EDMDenoiser.from_reference_module(net, device='cpu')


def test_step_condition_on_a_plain_net_raises():
    """Fails before the feature: the keyword disappeared in **kwargs."""
    from diff_sampler_amd.engine import EDMDenoiser
    plain = EDMDenoiser.from_config('tiny_song', device='cpu')
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(ValueError, match='step'):
        plain(x, 1.0, step_condition=4)
    with pytest.raises(ValueError, match='step'):
        plain.raw(x, 1.0, step_condition=torch.tensor([4.0]))
    with pytest.raises(ValueError, match='step'):
        plain.head_update_ok(1, 1.0, step_condition=4)
    with pytest.raises(ValueError, match='step'):
        plain.engine.plan(1, 1, step=True)
    capable = EDMDenoiser.from_config('tiny_song', device='cpu', step_condition=True)
    assert capable._step_value(None) is None and capable._step_value(4) == 4.0 and capable._step_value(torch.tensor([5, 5])) == 5.0
    assert capable._step_value(np.float32(2.5)) == 2.5
    with pytest.raises(ValueError, match='one value'):
        capable._step_value(torch.tensor([4.0, 5.0]))
    with pytest.raises(NotImplementedError, match='skip_tuning'):
        capable(x, 1.0, step_condition=4, skip_tuning=True)
    with pytest.raises(NotImplementedError, match='skip_tuning'):
        plain(x, 1.0, skip_tuning=True)


# launch-list hashes recorded on the commit before the NCSN++ options (tests/test_hip_ncsnpp.py::test_existing_plans_hash_as_before)
PARENT_PLANS = {('cifar10', 4): {'/rows=4': (178, 'be6e8ed302cc5e59371ecb0e094cb523'), '/rows=1': (178, '85e40ac6578a44d0062ba83f8dbc4234')},
                ('ffhq', 2): {'/rows=2': (226, 'd82222054be0ea45e617b7d1e5b72acb'), '/rows=1': (226, 'e94891334fb2e8c8c06d3f681c05e62b')},
                ('imagenet64', 2): {'/rows=2': (275, '848694acb987887e46d7a352267f9948')}}


@pytest.mark.parametrize('key', sorted(PARENT_PLANS), ids=lambda k: '-'.join(map(str, k)))
def test_step_false_plans_hash_as_before_and_step_true_adds_the_stated_launches(key):
    """On an engine WITH step weights: plan(step=False) is launch for launch, argument for argument, the plan of a plain engine; step=True adds
    4 launches (SongUNet: embed, two Linear, one projection) or 5 (DhariwalUNet: + the compose launch) in front of / behind the affine launch."""
    import plan_dump as pd
    from diff_sampler_amd.engine import UNetEngine
    name, B = key
    spec = _spec(name)
    eng = UNetEngine(spec, arch.init_params(spec, seed=1), device='cpu')
    lib = _lib.load()
    for suffix, (nrows, sha) in PARENT_PLANS[key].items():
        r = int(suffix.split('=')[1])
        P = eng.plan(B, r)
        rows = [pd.row_record(*row) for row in pd.dump(eng, P)]
        assert (len(rows), hashlib.sha256('\n'.join(rows).encode()).hexdigest()[:32]) == (nrows, sha), (key, suffix)
        S = eng.plan(B, r, step=True)
        assert S is not P and eng.plan(B, r, step=True) is S and eng.plan(B, r) is P
        extra = 5 if spec.model_type == 'DhariwalUNet' else 4
        names, base = [op.name for op in S.ops], [op.name for op in P.ops]
        assert len(names) == nrows + extra
        assert names[:4] == ['step_embed', 'map_step_layer0', 'map_step_layer1', 'affine_step_all']
        assert [n for n in names if n not in ('step_embed', 'map_step_layer0', 'map_step_layer1', 'affine_step_all', 'affine_compose')] == base
        assert tuple(S.bufs['step'].shape) == (1,) and 'step' not in P.bufs
        i = names.index('affine_all')
        aff = S.ops[i].keep[0]
        if extra == 5:
            assert names[i + 1] == 'affine_compose' and S.ops[i + 1].fn is _lib.affine_compose
            c = S.ops[i + 1].keep[0]
            assert (c.aff, c.ld, c.rows, c.width, c.step) == (aff.out, eng.aff_total, r, eng.aff_total, S.bufs['aff_step'].data_ptr())
            assert c.groups == sum(b.cout for b in spec.blocks if b.kind == 'block') // 4 and aff.bias == eng.w['aff.b'].data_ptr()
        else:
            assert 'affine_compose' not in names and aff.bias == S.bufs['aff_step'].data_ptr()       # the step row IS the affine launch's bias
        assert not S.foreign and lib.ds_plan_size(S.native()) == len(names)                             # every launch has an op code
        pd.dump(eng, S)                                                                                 # and every pointer is classified


@pytest.mark.parametrize('name,B,kw', [('cifar10', 4, dict(use_fp16=True)), ('imagenet64', 4, dict(use_fp16=True)), ('imagenet64', 2, dict()),
                                       ('cifar10', 8, dict(split_fp16=True)), ('tiny_ncsnpp', 2, dict()), ('cifar10', 3, dict(batch_invariant=True))])
def test_step_plans_pass_the_dtype_lint(name, B, kw):
    from test_plan_cpu import _dtype_lint
    from diff_sampler_amd.engine import UNetEngine
    spec = _spec(name)
    eng = UNetEngine(spec, arch.init_params(spec, seed=1), device='cpu', **kw)
    assert _dtype_lint(eng.plan(B, B, step=True), _lib.load()) > 50


def test_ncsnpp_step_embedding_has_its_own_frequencies():
    from diff_sampler_amd.engine import UNetEngine
    spec = _spec('tiny_ncsnpp')
    p = arch.init_params(spec, seed=1)
    eng = UNetEngine(spec, p, device='cpu')
    assert torch.equal(eng.w['freqs_step'], (2 * np.pi * p['model.map_step.freqs']).float()) and not torch.equal(eng.w['freqs_step'], eng.w['freqs'])
    song = UNetEngine(_spec('tiny_song'), arch.init_params(_spec('tiny_song'), seed=1), device='cpu')
    assert song.w['freqs_step'] is song.w['freqs']
    P = eng.plan(2, 2, step=True)
    emb = P.ops[0].args
    assert emb[1] == 1 and emb[4] == 3 and emb[2].value == eng.w['freqs_step'].data_ptr()      # one row, [sin | cos], the value as given


def test_samplers_hand_the_step_condition_to_every_evaluation_but_denoise_to_zero():
    """solvers._Run on a recording denoiser of the plain protocol (no GPU: the run stops at the CUDA check, so the keyword plumbing is read
    from the signatures and from get_denoised)."""
    import inspect
    from diff_sampler_amd import solvers
    for fn in (getattr(solvers, n) for n in solvers.__all__ if n.endswith('_sampler')):
        assert inspect.signature(fn).parameters['step_condition'].default is None, fn.__name__
    seen = []

    def net(x, t, class_labels=None, **kw):
        seen.append(kw)
        return x
    solvers.get_denoised(net, torch.zeros(1), 1.0)
    solvers.get_denoised(net, torch.zeros(1), 1.0, step_condition=4)
    assert seen == [{}, {'step_condition': 4}]


# ---- DS_OP_AFFINE_COMPOSE -------------------------------------------------------------------------------------------------------------------
BLOCKS = [(0, 32), (64, 48), (160, 192)]          # (first column, cout): scale columns, then shift columns; 544 columns in all


def _compose_args(**over):
    buf = (C.c_float * 8192)()
    base = C.addressof(buf) + (-C.addressof(buf)) % 16
    p = lambda off: C.c_void_p(base + off)
    kw = dict(aff=p(0), ld=548, rows=3, width=544, step=p(8192), pairs=p(16384), groups=68)
    kw.update({k: (p(v) if k in ('aff', 'step', 'pairs') and isinstance(v, int) else v) for k, v in over.items()})
    a = _lib.AffineComposeArgs(**kw)
    a._keep = buf
    return a


COMPOSE_BAD = [('null aff', dict(aff=None), DS_E_ARG), ('null step', dict(step=None), DS_E_ARG), ('null pairs', dict(pairs=None), DS_E_ARG),
               ('rows = 0', dict(rows=0), DS_E_ARG), ('rows < 0', dict(rows=-1), DS_E_ARG), ('groups = 0', dict(groups=0), DS_E_ARG),
               ('width = 0', dict(width=0), DS_E_SHAPE), ('width % 4', dict(width=542), DS_E_SHAPE), ('width > ld', dict(width=552), DS_E_SHAPE),
               ('ld % 4', dict(ld=550), DS_E_ALIGN), ('aff off 16 bytes', dict(aff=4), DS_E_ALIGN), ('step off 16 bytes', dict(step=8200), DS_E_ALIGN),
               ('pairs off 8 bytes', dict(pairs=16388), DS_E_ALIGN), ('too many threads', dict(rows=1 << 30, groups=4), DS_E_SHAPE)]


@pytest.mark.parametrize('what,over,code', COMPOSE_BAD, ids=[b[0] for b in COMPOSE_BAD])
def test_affine_compose_refuses_on_the_host(what, over, code):
    """Every refusal comes before the launch: no GPU is needed (or touched)."""
    assert _lib.run_op_rc(_lib.DS_OP_AFFINE_COMPOSE, _compose_args(**over), None) == code


def test_affine_compose_is_a_plan_operation_like_its_two_predecessors():
    assert _lib.DS_OP_AFFINE_COMPOSE == 20 and 'ds_affine_compose' not in _lib.EXPORTS
    header = open(os.path.join(ROOT, 'include', 'ds_engine.h')).read()
    assert 'DS_OP_AFFINE_COMPOSE = 20' in header and 'ds_affine_compose_args' in header
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.ds_plan_create(C.byref(h)) == 0
    try:
        a = _lib.AffineComposeArgs()
        assert lib.ds_plan_add(h, _lib.DS_OP_AFFINE_COMPOSE, C.byref(a), C.sizeof(a)) == 0
        assert lib.ds_plan_add(h, _lib.DS_OP_AFFINE_COMPOSE, C.byref(a), C.sizeof(a) - 4) == DS_E_ARG
        assert lib.ds_plan_run(h, None) == DS_E_ARG and lib.ds_plan_last_failed(h) == 0      # all-NULL arguments: refused, nothing launched
    finally:
        lib.ds_plan_destroy(h)


def _compose_case(rows, seed):
    g = torch.Generator().manual_seed(seed)
    aff = torch.randn(rows, 548, generator=g) * 0.7
    step = torch.randn(544, generator=g) * 0.7
    aff[:, 5] = -1.0 + 2.0 ** -20          # 1 + s almost cancels: the product term of the bound is what covers it
    step[3] = -1.0 + 2.0 ** -18
    return aff, step


@pytest.mark.parametrize('rows', [1, 3])
def test_affine_compose_arithmetic_stays_inside_its_bound(rows):
    aff, step = _compose_case(rows, 40 + rows)
    got = R.compose_emulate(aff, step, BLOCKS)
    ref, bound = R.compose_ref64(aff, step, BLOCKS)
    err = (got.double() - ref).abs()
    assert bool((err <= bound).all()), float((err / bound.clamp_min(1e-300)).max())
    touched = torch.zeros(548, dtype=torch.bool)
    for off, c in BLOCKS:
        touched[off:off + 2 * c] = True
    assert int(touched.sum()) == 544 and torch.equal(got[:, ~touched], aff[:, ~touched]) and bool((bound[:, ~touched] == 0).all())
    pairs = R.compose_pairs(BLOCKS)
    assert tuple(pairs.shape) == (68, 2) and int(pairs.max()) == 544 - 4 and bool((pairs % 4 == 0).all())


def test_composed_affine_equals_the_two_stage_expression():
    """(1 + scale') n + shift' in fp32 on the composed pair against shift_step + (shift + n (scale + 1)) (scale_step + 1) in fp64."""
    aff, step = _compose_case(3, 50)
    comp = R.compose_emulate(aff, step, BLOCKS)
    g = torch.Generator().manual_seed(51)
    worst = 0.0
    for off, c in BLOCKS:
        n = torch.randn(3, c, generator=g) * 2
        y = ((1.0 + comp[:, off:off + c]) * n) + comp[:, off + c:off + 2 * c]
        ref, bound = R.two_stage64(n, aff, step, off, c)
        err = (y.double() - ref).abs()
        assert bool((err <= bound).all()), (off, float((err / bound).max()))
        worst = max(worst, float((err / bound).max()))
    print(f'composed affine vs two-stage fp64: worst err / bound = {worst:.3f}')
    assert worst > 1e-3          # the bound is not vacuous


# ---- the latent-diffusion U-Net (nfe_embed, emb_nfe_layers) --------------------------------------------------------------------------------------
def _ldm(name='tiny_ldm_1res', step=True):
    import diff_sampler_amd.ldm_arch as la
    kw = dict(la.NAMED_LDM_CONFIGS[name])
    return kw, la.ldm_unet_spec(**kw, step_condition=step)


def test_ldm_restatement_equals_the_reference_golden():
    """CFGPrecond + the step-conditioned UNetModel under guidance 7.5: evaluations without a step, at 4 and at 6, and the 4-step Euler
    trajectory on the discrete schedule, against the project's CPU restatement with the step row folded into the emb_layers biases."""
    import diff_sampler_amd.ldm_arch as la
    from diff_sampler_amd.solver_utils import get_schedule
    z = np.load(os.path.join(G, 'sfd_ldm_tiny.npz'))
    kw, spec = _ldm()
    params = la.init_ldm_params(spec, seed=int(z['seed']))
    x, sig, cond, uncond = (torch.from_numpy(z[k]) for k in ('x', 'sigma', 'cond', 'uncond'))
    e = {}
    with torch.no_grad():
        for key, step in (('out_none', None), ('out_step4', 4), ('out_step6', 6)):
            e[key] = _rel(R.cfg_sfd(params, kw, spec, step=step)(x, sig, condition=cond, unconditional_condition=uncond), torch.from_numpy(z[key]))
        net = R.cfg_sfd(params, kw, spec, step=4)
        ts = get_schedule(4, net.sigma_min, net.sigma_max, device='cpu', schedule_type='discrete', schedule_rho=1, net=net)
        xt = torch.from_numpy(z['latents']) * ts[0]
        tr = [xt]
        for t, tn in zip(ts[:-1], ts[1:]):
            d = (xt - net(xt, t, condition=cond, unconditional_condition=uncond)) / t
            xt = xt + (tn - t) * d
            tr.append(xt)
    gold = torch.from_numpy(z['traj_euler'])
    e['traj'] = max(_rel(a, b) for a, b in zip(tr, gold))
    print(f'ldm restatement vs golden rel = {e}')
    assert max(e.values()) <= 1e-6, e
    assert _rel(torch.from_numpy(z['out_step4']), torch.from_numpy(z['out_none'])) > 1e-2
    assert _rel(torch.from_numpy(z['out_step4']), torch.from_numpy(z['out_step6'])) > 2e-3


def test_ldm_param_table_is_the_reference_state_dict():
    import diff_sampler_amd.ldm_arch as la
    z = np.load(os.path.join(G, 'sfd_ldm_tiny.npz'))
    want = [(k, tuple(s)) for k, s in json.loads(str(z['state_dict']))]
    (kw, spec), (_, plain) = _ldm(), _ldm(step=False)
    got = [(k, tuple(s)) for k, s, _ in la.ldm_param_table(spec)]
    assert sorted(got) == sorted(want) and len(set(k for k, _ in got)) == len(got)       # (the table is keyed, not ordered, like the state dict)
    new = [k for k, _ in got if k.startswith('nfe_embed.') or '.emb_nfe_layers.' in k]
    assert len(new) == 4 + 2 * len(spec.res_layers())
    assert [(k, tuple(s)) for k, s, _ in la.ldm_param_table(plain)] == [kv for kv in got if kv[0] not in new]
    a, b = la.init_ldm_params(plain, seed=3), la.init_ldm_params(spec, seed=3)
    assert list(b) == [k for k, _ in got] and all(torch.equal(a[k], b[k]) for k in a) and all(float(b[k].abs().max()) > 0 for k in new)


LDM_PARENT_PLANS = {('tiny', 2): None, ('sd15', 1): {'/rows=2': (361, '1bce91e815afb2e5d9255daa8fd005f0'), '/rows=1': (361, '284b656dc531f38a641d9316c4f5b449')}}


@pytest.mark.parametrize('key', sorted(LDM_PARENT_PLANS), ids=lambda k: '-'.join(map(str, k)))
def test_ldm_step_false_plans_hash_as_before_and_step_true_adds_four_launches(key):
    """sd15 B = 1 against the hashes recorded before the feature; the tiny net against a plain engine built from the same weights."""
    import plan_dump as pd
    import diff_sampler_amd.ldm_arch as la
    from diff_sampler_amd.ldm_engine import LDMUNetEngine
    name, B = key
    kw, spec = _ldm('sd15' if name == 'sd15' else 'tiny_ldm_1res')
    params = la.init_ldm_params(spec, seed=1)
    eng = LDMUNetEngine(spec, params, device='cpu')
    def sha(e, P):          # (rows, digest) of a plan's dump: the context projections' launches lead the list
        rows = [pd.row_record(*r) for r in pd.dump(e, P)]
        return len(rows), hashlib.sha256('\n'.join(rows).encode()).hexdigest()[:32]
    n = 2 * B
    want = LDM_PARENT_PLANS[key]
    if want is None:
        plain_spec = _ldm('tiny_ldm_1res', step=False)[1]
        plain = LDMUNetEngine(plain_spec, {k: params[k] for k, _, _ in la.ldm_param_table(plain_spec)}, device='cpu')
        want = {f'/rows={r}': sha(plain, plain.plan(n, r, 77)) for r in (n, 1)}
    for suffix, (nrows, digest) in want.items():
        r = int(suffix.split('=')[1])
        P = eng.plan(n, r, 77)
        assert sha(eng, P) == (nrows, digest), (key, suffix)
        S = eng.plan(n, r, 77, step=True)
        names = [op.name for op in S.ops]
        assert len(names) == len(P.ops) + 4 and names[3:7] == ['step_embedding', 'nfe_embed.0', 'nfe_embed.2', 'emb_nfe_layers_all'], names[:8]
        assert [x for x in names if x not in ('step_embedding', 'nfe_embed.0', 'nfe_embed.2', 'emb_nfe_layers_all')] == [op.name for op in P.ops]
        aff = S.ops[names.index('emb_layers_all')].keep[0]
        assert aff.bias == S.bufs['aff_step'].data_ptr() and tuple(S.bufs['step'].shape) == (1,) and 'step' not in P.bufs
        assert S.ops[3].args[1] == 1 and S.ops[3].args[4] == 2            # ONE row for both halves of a classifier-free evaluation, the value as given
        pd.dump(eng, S)
    if name != 'sd15':
        from test_plan_cpu import _dtype_lint
        e16 = LDMUNetEngine(spec, params, device='cpu', use_fp16=True)
        assert _dtype_lint(e16.plan(n, n, 77, step=True), _lib.load()) > 20
        b0 = spec.res_layers()[0]
        assert torch.equal(eng.w['affs.b'][:b0.cout], params[f'{b0.key}.emb_layers.1.bias'] + params[f'{b0.key}.emb_nfe_layers.1.bias'])


def test_cfg_denoiser_step_condition_on_a_plain_net_raises():
    from diff_sampler_amd.ldm_engine import CFGDenoiser
    plain = CFGDenoiser.from_config('tiny_ldm_1res', device='cpu')
    x, c = torch.zeros(1, 4, 16, 16), torch.zeros(1, 77, 64)
    with pytest.raises(ValueError, match='step'):
        plain(x, 1.0, condition=c, step_condition=4)
    with pytest.raises(ValueError, match='step'):
        plain.engine.plan(2, 1, 77, step=True)
    with pytest.raises(NotImplementedError, match='skip_tuning'):
        plain(x, 1.0, condition=c, skip_tuning=True)
    capable = CFGDenoiser.from_config('tiny_ldm_1res', device='cpu', step_condition=True)
    assert capable.spec.step_condition and capable._step_value(torch.tensor([4, 4, 4])) == 4.0
    with pytest.raises(ValueError, match='one value'):
        capable._step_value(torch.tensor([4, 5]))


def test_ldm_spec_from_module_recovers_the_step_condition_and_refuses_half_a_tree():
    """The ms_coco route of sample.load_sfd: the snapshot's LatentDiffusion state dict is keyed like an SD checkpoint, and the U-Net's spec comes
    from the module's own attributes and tensors."""
    import diff_sampler_amd.ldm_arch as la
    from diff_sampler_amd.ldm_engine import ldm_spec_from_module
    from diff_sampler_amd.sample import split_sd_checkpoint
    net = duck.build_ldm('tiny_ldm_1res', seed=2)
    params, vae = split_sd_checkpoint(net.model.state_dict())
    kw, want = _ldm()
    assert not vae and sorted(params) == sorted(k for k, _, _ in la.ldm_param_table(want))
    unet = net.model.model.diffusion_model
    assert ldm_spec_from_module(unet, net.img_resolution, params) == want == ldm_spec_from_module(unet, net.img_resolution)
    for drop in ('nfe_embed', 'emb_nfe_layers'):
        with pytest.raises(ValueError, match='step'):
            ldm_spec_from_module(duck.build_ldm('tiny_ldm_1res', seed=2, drop=drop).model.model.diffusion_model, 16)
    plain = {k: v for k, v in params.items() if 'nfe' not in k}
    assert ldm_spec_from_module(unet, 16, plain) == _ldm(step=False)[1]
    with pytest.raises(NotImplementedError, match='state dict'):
        ldm_spec_from_module(unet, 16, dict(params, extra=torch.zeros(1)))
