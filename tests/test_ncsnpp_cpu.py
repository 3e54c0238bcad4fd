"""CPU-only: the NCSN++ side of the EDM SongUNet (Fourier embedding, residual encoder, [1,3,3,1] resampling, channel_mult_noise) as data
model, launch plan and host-side library surface.

  * tests/_ncsnpp_ref.py -- the functional restatement the GPU tests compare against -- equals the goldens recorded from the reference
    classes (tools/gen_ncsnpp_golden.py).  It makes the same ATen calls; bound 1e-6, OBSERVED 0.0 for all four configs and both sigma forms
    (printed by the test).
  * ``param_table`` lists the reference's state-dict keys and shapes in its order, ``init_params`` of the existing configs keeps its bits,
    ``spec_from_module`` recovers the three options from a module tree and refuses the ``skip`` variants.
  * the engine refuses the modes it has no NCSN++ form for, builds the two mixed configs, and libdsmetrics answers every bad argument of
    dsm_fir_resample / dsm_zero_border on the host.
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

import diff_sampler_amd.arch as arch  # noqa: E402
import _ncsnpp_ref as R  # noqa: E402
import _ref_like_ncsnpp as duck  # noqa: E402

G = os.path.join(ROOT, 'tests', 'golden')
CONFIGS = ['tiny_ncsnpp', 'tiny_ncsnpp_cond', 'cifar10_ve', 'ffhq_ve']
MIXED = {'positional_residual_fir': dict(arch.NAMED_CONFIGS['tiny_ncsnpp'], embedding_type='positional', channel_mult_noise=1),
         'fourier_standard_box': dict(arch.NAMED_CONFIGS['tiny_ncsnpp'], encoder_type='standard', resample_filter=[1, 1])}


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


@pytest.mark.parametrize('name', CONFIGS)
def test_restatement_equals_the_reference_golden(name):
    z = np.load(os.path.join(G, f'ncsnpp_net_{name}.npz'))
    spec = arch.edm_precond_spec(**arch.NAMED_CONFIGS[name])
    params = arch.init_params(spec, seed=int(z['seed']))
    x = torch.from_numpy(z['x'])
    lab = torch.from_numpy(z['labels']) if z['labels'].size else None
    taps = {}
    out_vec = R.edm_ncsnpp(params, spec, x, torch.from_numpy(z['sigma']), lab, taps=taps)
    out_sc = R.edm_ncsnpp(params, spec, x, torch.tensor(0.6), lab)
    e = (_rel(out_vec, torch.from_numpy(z['out_vec'])), _rel(out_sc, torch.from_numpy(z['out_scalar'])))
    print(f'{name}: restatement vs golden rel = {e[0]:.3g} (per-sample sigma), {e[1]:.3g} (scalar sigma)')
    assert max(e) <= 1e-6, e
    recorded = sorted(k[4:] for k in z.files if k.startswith('tap_'))
    if name.startswith('tiny'):
        assert recorded == sorted(taps) and any('aux_residual' in k for k in recorded)
    for k in recorded:
        assert _rel(taps[k], torch.from_numpy(z['tap_' + k])) <= 1e-6, k


@pytest.mark.parametrize('name', CONFIGS)
def test_param_table_is_the_reference_state_dict(name):
    z = np.load(os.path.join(G, f'ncsnpp_net_{name}.npz'))
    want = [(k, tuple(s)) for k, s in json.loads(str(z['state_dict']))]
    spec = arch.edm_precond_spec(**arch.NAMED_CONFIGS[name])
    got = [(k, tuple(s)) for k, s, _ in arch.param_table(spec)]
    assert got == want
    assert got[0][0] == 'model.map_noise.freqs' and sum('_aux_residual.' in k for k, _ in got) == 2 * sum(b.kind == 'aux' for b in spec.blocks) > 0
    p = arch.init_params(spec, seed=3)
    assert list(p) == [k for k, _ in got] and all(tuple(p[k].shape) == s for k, s in got)
    # freqs ~ N(0, 16^2) in both modes, the same draw
    f = p['model.map_noise.freqs']
    assert 8.0 < float(f.std()) < 32.0 and torch.equal(f, arch.init_params(spec, seed=3, mode='reference')['model.map_noise.freqs'])


# sha256 over (key, bytes) of a few tensors / of all tensors of init_params(spec, seed=3), computed on the commit before the NCSN++ options
PINNED = {'cifar10': (['model.map_augment.weight', 'model.dec.8x8_block0.affine.bias', 'model.dec.32x32_aux_conv.bias', 'model.map_layer0.weight'],
                      '4c0a7059d9131390229c08d55fdac9dfc47f8ae2470f89e8129bd58f3742eb5d',
                      '412903fd48f9436b0784ee2617ad304381ac18637f83476b4402db14d5293114', 417),
          'tiny_song': (['model.map_augment.weight', 'model.dec.8x8_in1.conv1.weight', 'model.dec.16x16_aux_conv.bias', 'model.map_layer0.weight'],
                        '9811205a584b3e542c06717889d2b737c13ff018af097b6ed6364068d4ef9432',
                        '7406a0abbb5b7cf578278593a7631e7163c1ee72b77d6b5827819d9efb7d6883', 143)}


@pytest.mark.parametrize('name', sorted(PINNED))
def test_init_params_of_existing_configs_keep_their_bits(name):
    pick, sha_pick, sha_all, nkeys = PINNED[name]
    p = arch.init_params(arch.edm_precond_spec(**arch.NAMED_CONFIGS[name]), seed=3)
    assert len(p) == nkeys

    def sha(keys):
        h = hashlib.sha256()
        for k in keys:
            h.update(k.encode())
            h.update(p[k].numpy().tobytes())
        return h.hexdigest()
    assert sha(pick) == sha_pick and sha(list(p)) == sha_all


def test_ncsnpp_tensors_come_from_their_own_generator():
    """Every tensor a network shares with its DDPM++ counterpart has the counterpart's bits."""
    a = arch.init_params(arch.edm_precond_spec(**MIXED['fourier_standard_box']), seed=5)
    kw = dict(MIXED['fourier_standard_box'], embedding_type='positional')
    b = arch.init_params(arch.edm_precond_spec(**kw), seed=5)
    assert set(a) - set(b) == {'model.map_noise.freqs'} and all(torch.equal(a[k], b[k]) for k in b)


@pytest.mark.parametrize('name', CONFIGS + sorted(MIXED))
def test_spec_from_module_recovers_the_ncsnpp_options(name):
    """Fails before the NCSN++ options existed: a DDPM++ spec came back from such a tree, and five state-dict entries were dropped."""
    from diff_sampler_amd.engine import spec_from_module
    kw = MIXED.get(name) or arch.NAMED_CONFIGS[name]
    net = duck.build(kw, seed=2)
    spec = spec_from_module(net)
    want = arch.edm_precond_spec(**kw)
    assert (spec.embedding_type, spec.encoder_type, list(spec.resample_filter)) == (
        kw.get('embedding_type', 'positional'), kw.get('encoder_type', 'standard'), list(kw.get('resample_filter', [1, 1])))
    assert spec == want
    if name in CONFIGS:
        assert (spec.embedding_type, spec.encoder_type, tuple(spec.resample_filter), spec.noise_channels) == (
            'fourier', 'residual', (1, 3, 3, 1), 2 * spec.model_channels)
    # nothing of the module's state is left over: the tree's keys are the parameter table's, in order
    keys = [k for k in net.state_dict() if 'resample_filter' not in k]
    assert keys == [k for k, _, _ in arch.param_table(spec)]


def test_spec_from_module_refuses_the_skip_encoder():
    from diff_sampler_amd.engine import spec_from_module
    kw = dict(arch.NAMED_CONFIGS['tiny_ncsnpp'], encoder_type='standard')
    with pytest.raises(NotImplementedError, match='skip'):
        spec_from_module(duck.build(kw, skip_variant=True))


def test_song_unet_spec_still_refuses_what_no_checkpoint_uses():
    base = dict(img_resolution=32, in_channels=3, out_channels=3)
    for bad in (dict(encoder_type='skip'), dict(decoder_type='skip'), dict(resample_filter=[1, 2, 1]), dict(resample_filter=[1, 4, 6, 4, 1])):
        with pytest.raises(NotImplementedError):
            arch.song_unet_spec(**base, **bad)
    # the four options are independent of each other
    for emb in ('positional', 'fourier'):
        for enc in ('standard', 'residual'):
            for f in ([1, 1], [1, 3, 3, 1]):
                for cmn in (1, 2, 3):
                    s = arch.song_unet_spec(**base, model_channels=32, channel_mult=[1, 2], num_blocks=1, embedding_type=emb, encoder_type=enc,
                                            resample_filter=f, channel_mult_noise=cmn)
                    assert s.noise_channels == 32 * cmn and sum(b.kind == 'aux' for b in s.blocks) == (1 if enc == 'residual' else 0)
                    assert s.ncsnpp == ((emb, enc, f) != ('positional', 'standard', [1, 1]))


@pytest.mark.parametrize('mode', ['use_fp16', 'split_fp16', 'batch_invariant'])
@pytest.mark.parametrize('name', ['tiny_ncsnpp'] + sorted(MIXED))
def test_modes_without_an_ncsnpp_form_are_refused_at_build_time(name, mode):
    from diff_sampler_amd.engine import UNetEngine
    spec = arch.edm_precond_spec(**(MIXED.get(name) or arch.NAMED_CONFIGS[name]))
    with pytest.raises(NotImplementedError, match='fp32'):
        UNetEngine(spec, arch.init_params(spec, seed=1), device='cpu', **{mode: True})


def _plan_names(kw, B=2):
    from diff_sampler_amd.engine import UNetEngine
    spec = arch.edm_precond_spec(**kw)
    eng = UNetEngine(spec, arch.init_params(spec, seed=1), device='cpu')
    return spec, eng, eng.plan(B, B)


@pytest.mark.parametrize('name', sorted(MIXED))
def test_mixed_configs_build_and_agree_with_the_restatement_shapes(name):
    kw = MIXED[name]
    spec, eng, P = _plan_names(kw)
    taps = {}
    x = torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(1))
    out = R.edm_ncsnpp(arch.init_params(spec, seed=1), spec, x, torch.tensor([2.0, 0.3]), taps=taps)
    assert tuple(out.shape) == tuple(P.bufs['out'].shape) == (2, 3, 32, 32) and bool(torch.isfinite(out).all())
    # every skip-stack tensor of the restatement has a plan buffer of its name and size
    for k, t in taps.items():
        assert tuple(P.bufs[k].shape) == (t.shape[0] * t.shape[2] * t.shape[3], t.shape[1]), k
    names = [op.name for op in P.ops]
    fir = [n for n in names if n.endswith('.fir')]
    if name == 'positional_residual_fir':
        assert P.foreign and len([n for n in fir if 'aux_residual' in n]) == 2 and len(fir) == 2 + 2 * 4       # 2 down + 2 up blocks: conv0 and skip each
        assert eng.w['freqs'].shape == (16,) and float(eng.w['freqs'][0]) == 1.0
    else:
        assert not fir and not P.foreign and eng.w['freqs'].shape == (32,)
        assert torch.equal(eng.w['freqs'], (2 * np.pi * arch.init_params(spec, seed=1)['model.map_noise.freqs']).float())


def test_fir_filter_blocks_take_no_box_filter_route():
    """With [1,3,3,1] no launch resamples inside ds_norm_act and no convolution reads through the x2 phase form."""
    from diff_sampler_amd import _lib
    spec, eng, P = _plan_names(arch.NAMED_CONFIGS['cifar10_ve'], B=4)
    lib = _lib.load()
    for op in P.ops:
        if op.fn is lib.ds_norm_act:
            assert op.keep[0].resample == _lib.DS_RESAMPLE_NONE, op.name
        if op.fn is lib.ds_conv2d_nhwc:
            assert not op.keep[0].in_up2, op.name
    order = [op.name for op in P.ops]
    i = order.index('enc.16x16_aux_residual.ring')
    assert order[i:i + 4] == ['enc.16x16_aux_residual.ring', 'enc.16x16_aux_residual.im2col', 'enc.16x16_aux_residual.conv', 'enc.16x16_aux_residual.fir']
    j = order.index('enc.8x8_aux_residual.ring')
    assert order[j:j + 3] == ['enc.8x8_aux_residual.ring', 'enc.8x8_aux_residual.conv', 'enc.8x8_aux_residual.fir']
    assert arch.flops_per_image(spec) > arch.flops_per_image(arch.edm_precond_spec(**dict(arch.NAMED_CONFIGS['cifar10_ve'], encoder_type='standard')))


def test_flops_count_the_aux_convolutions():
    kw = arch.NAMED_CONFIGS['cifar10_ve']
    a = arch.flops_per_image(arch.edm_precond_spec(**kw))
    b = arch.flops_per_image(arch.edm_precond_spec(**dict(kw, encoder_type='standard')))
    assert a - b == 2.0 * 9 * (34 ** 2 * 3 * 256 + 18 ** 2 * 256 * 256)


# ---- host-side refusals of the two entry points: no GPU is needed (or touched) -------------------------------------------------------------
@pytest.fixture(scope='module')
def mlib():
    from diff_sampler_amd import build, _metrics_lib
    build.build_metrics_lib(verbose=False)
    return _metrics_lib.load()


def _fir(**over):
    from diff_sampler_amd._metrics_lib import DsmFirArgs
    buf = (C.c_float * 4096)()
    base = C.addressof(buf) + (-C.addressof(buf)) % 16
    p = lambda off: C.c_void_p(base + off)
    kw = dict(x=p(0), ld_x=8, n=1, h=6, w=6, c=8, up=0, pad=1, taps=(C.c_float * 4)(1, 3, 3, 1), bias=None, res=None, res_ld=0, out_scale=1.0,
              out=p(4096), out_ld=8)
    kw.update({k: (p(v) if k in ('x', 'out', 'bias', 'res') and isinstance(v, int) else v) for k, v in over.items()})
    a = DsmFirArgs(**kw)
    a._keep = buf
    return a


FIR_BAD = [('null args', None, 'ARG'), ('null x', dict(x=None), 'ARG'), ('null out', dict(out=None), 'ARG'), ('x is out', dict(out=0), 'ARG'),
           ('n = 0', dict(n=0), 'ARG'), ('h = 0', dict(h=0), 'ARG'), ('w < 0', dict(w=-2), 'ARG'), ('c = 0', dict(c=0), 'ARG'),
           ('c % 4', dict(c=6), 'ALIGN'), ('ld_x < c', dict(ld_x=4), 'ARG'), ('out_ld < c', dict(out_ld=4), 'ARG'),
           ('res_ld < c', dict(res=8192, res_ld=4), 'ARG'), ('ld_x % 4', dict(ld_x=10), 'ALIGN'), ('out_ld % 4', dict(out_ld=9), 'ALIGN'),
           ('res_ld % 4', dict(res=8192, res_ld=10), 'ALIGN'), ('x misaligned', dict(x=4), 'ALIGN'), ('out misaligned', dict(out=4100), 'ALIGN'),
           ('bias misaligned', dict(bias=8196), 'ALIGN'), ('res misaligned', dict(res=8200, res_ld=8), 'ALIGN'),
           ('odd h does not fit', dict(h=7), 'SHAPE'), ('odd w does not fit', dict(w=5), 'SHAPE'), ('pad 0 too small', dict(pad=0, h=2, w=2), 'SHAPE'),
           ('pad = 2', dict(pad=2), 'ARG'), ('up with pad 0', dict(up=1, pad=0), 'ARG'), ('up = 2', dict(up=2), 'ARG'),
           ('taps sum to zero', dict(taps=(C.c_float * 4)(1, -1, 1, -1)), 'ARG'), ('reserved', 'reserved', 'ARG')]


@pytest.mark.parametrize('what,over,code', FIR_BAD, ids=[b[0] for b in FIR_BAD])
def test_fir_resample_refuses_on_the_host(mlib, what, over, code):
    from diff_sampler_amd import _metrics_lib as ML
    want = {'ARG': ML.DS_E_ARG, 'ALIGN': ML.DS_E_ALIGN, 'SHAPE': ML.DS_E_SHAPE}[code]
    if over is None:
        assert mlib.dsm_fir_resample(None, None) == want
        return
    a = _fir() if over == 'reserved' else _fir(**over)
    if over == 'reserved':
        a.reserved[1] = 1
    assert mlib.dsm_fir_resample(C.byref(a), None) == want


def test_fir_resample_supported_is_the_host_side_of_the_same_rules(mlib):
    ok = mlib.dsm_fir_resample_supported
    assert ok(0, 1, 8, 8, 4) and ok(0, 1, 2, 2, 8) and ok(0, 0, 34, 34, 32) and ok(0, 0, 10, 6, 8) and ok(1, 1, 1, 1, 8) and ok(1, 1, 3, 5, 36)
    assert not ok(0, 1, 7, 8, 4) and not ok(0, 0, 2, 4, 4) and not ok(0, 1, 8, 8, 6) and not ok(1, 0, 4, 4, 4) and not ok(0, 2, 8, 8, 4)
    assert not ok(0, 1, 0, 8, 4) and not ok(2, 1, 4, 4, 4)


ZB_BAD = [('null x', dict(x=None), 'ARG'), ('null out', dict(out=None), 'ARG'), ('x is out', dict(out=0), 'ARG'), ('outer = 0', dict(outer=0), 'ARG'),
          ('h = 0', dict(h=0), 'ARG'), ('w < 0', dict(w=-1), 'ARG'), ('inner = 0', dict(inner=0), 'ARG'), ('p < 0', dict(p=-1), 'ARG'),
          ('quads misaligned', dict(x=4), 'ALIGN'), ('quads out misaligned', dict(out=4104), 'ALIGN'), ('floats misaligned', dict(inner=1, x=2), 'ALIGN'),
          ('side too large', dict(h=40000), 'SHAPE'), ('too many pixels', dict(outer=1 << 40), 'SHAPE')]


@pytest.mark.parametrize('what,over,code', ZB_BAD, ids=[b[0] for b in ZB_BAD])
def test_zero_border_refuses_on_the_host(mlib, what, over, code):
    from diff_sampler_amd import _metrics_lib as ML
    buf = (C.c_float * 4096)()
    base = C.addressof(buf) + (-C.addressof(buf)) % 16
    kw = dict(x=0, out=4096, outer=2, h=4, w=4, inner=8, p=1)
    kw.update(over)
    ptr = lambda v: None if v is None else C.c_void_p(base + v)
    rc = mlib.dsm_zero_border(ptr(kw['x']), ptr(kw['out']), kw['outer'], kw['h'], kw['w'], kw['inner'], kw['p'], None)
    assert rc == {'ARG': ML.DS_E_ARG, 'ALIGN': ML.DS_E_ALIGN, 'SHAPE': ML.DS_E_SHAPE}[code]


def test_source_hashes_do_not_cover_the_new_translation_unit():
    """csrc/metrics/ is outside every hash of libdsamd's sources: tile tables and profile ties stay valid."""
    from diff_sampler_amd import build
    assert 'fir_resample.hip' not in build.source_hashes()
    assert os.path.join(build.METRICS_DIR, 'fir_resample.hip') in build.metrics_sources()
