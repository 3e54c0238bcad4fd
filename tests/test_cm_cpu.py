"""CPU: the consistency-model nets (cm_arch / cm_engine): parameter tables against the reference's recorded key and shape lists, the qkv
permutation, every refusal, create_model, the routing of the LSUN fp16 plan (wide fp16 block convolutions on, and off), the `wide16` flag on
plans that have no layer above 64 pixels, and the sub-batch logic."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from diff_sampler_amd import _lib, arch, cm_arch  # noqa: E402
from diff_sampler_amd.cm_engine import CMDenoiser, plan_elements_per_image, split_batch  # noqa: E402
import _routing  # noqa: E402

GOLD = os.path.join(ROOT, 'tests', 'golden')
WIDE_IDS = (2575, 2576)


@pytest.fixture(scope='module')
def keys():
    with open(os.path.join(GOLD, 'cm_keys.json')) as fh:
        return json.load(fh)


@pytest.mark.parametrize('name,rec', [('lsun_bedroom', 'lsun'), ('lsun_cat', 'lsun'), ('tiny_cm', 'tiny_cm'), ('tiny_cm_wide', 'tiny_cm_wide')])
def test_parameter_table_is_the_reference_state_dict(keys, name, rec):
    spec = cm_arch.cm_precond_spec(name)
    table = cm_arch.cm_param_table(spec)
    assert [(k, list(s)) for k, s, _ in table] == [(k, list(s)) for k, s in keys[rec]]
    assert sorted(e for _, _, e in table) == sorted(k for k, _, _ in arch.param_table(spec))


def test_lsun_setting_is_the_recorded_one(keys):
    for name in ('lsun_bedroom', 'lsun_cat'):
        assert cm_arch.NAMED_CM_CONFIGS[name] == keys['lsun_setting']
    spec = cm_arch.cm_precond_spec('lsun_bedroom')
    assert spec.use_fp16 and spec.cm_noise and not spec.swap_sincos and not spec.pos_endpoint and spec.sigma_data == 0.5
    blocks = [b for b in spec.blocks if b.kind == 'block']
    assert all(b.skip_scale == 1.0 and b.eps == 1e-5 and not b.adaptive_scale for b in blocks)
    assert all(b.adaptive_scale for b in cm_arch.cm_precond_spec('tiny_cm').blocks if b.kind == 'block')
    assert sum(torch.Size(s).numel() for _, s, _ in cm_arch.cm_param_table(spec)) == 526304771


def test_qkv_permutation_round_trips_and_is_the_stated_one():
    heads, d, c = 4, 64, 256
    w = torch.arange(3 * heads * d, dtype=torch.float32)[:, None].expand(-1, c).contiguous()      # row value = its index in (three, head, d) order
    e = cm_arch.qkv_to_engine(w, heads)
    for three, h, dd in ((0, 0, 0), (1, 2, 5), (2, 3, 63)):
        assert e[(h * d + dd) * 3 + three, 0] == (three * heads + h) * d + dd
    assert torch.equal(cm_arch.qkv_to_reference(e, heads), w)
    b = torch.randn(3 * heads * d)
    assert torch.equal(cm_arch.qkv_to_reference(cm_arch.qkv_to_engine(b, heads), heads), b)
    w4 = torch.randn(3 * heads * d, c, 1, 1)
    assert torch.equal(cm_arch.qkv_to_engine(w4, heads)[:, :, 0, 0], cm_arch.qkv_to_engine(w4[:, :, 0, 0], heads))


def test_state_dict_round_trip_and_entries_without_a_place_are_refused():
    spec = cm_arch.cm_precond_spec('tiny_cm')
    p = arch.init_params(spec, seed=3)
    sd = cm_arch.reference_state_dict(spec, p)
    back = cm_arch.engine_params(spec, sd)
    assert set(back) == set(p) and all(torch.equal(back[k], p[k]) for k in p)
    qkv = [k for k in sd if k.endswith('qkv.weight')][0]
    assert not torch.equal(sd[qkv], p[dict((r, e) for r, _, e in cm_arch.cm_param_table(spec))[qkv]])       # the rows really move
    with pytest.raises(NotImplementedError):
        cm_arch.engine_params(spec, dict(sd, **{'label_emb.weight': torch.zeros(10, 512)}))
    with pytest.raises(KeyError):
        cm_arch.engine_params(spec, {k: v for k, v in sd.items() if k != 'out.2.bias'})
    with pytest.raises(ValueError):
        cm_arch.engine_params(spec, dict(sd, **{'out.2.bias': torch.zeros(4)}))


@pytest.mark.parametrize('change', [dict(resblock_updown=False), dict(num_head_channels=-1), dict(use_new_attention_order=True),
                                    dict(class_cond=True), dict(num_channels=64), dict(num_channels=96), dict(learn_sigma=True),
                                    dict(num_head_channels=32)], ids=lambda c: ','.join(f'{k}={v}' for k, v in c.items()))
def test_refusals(change):
    kw = dict(cm_arch.NAMED_CM_CONFIGS['tiny_cm'], **change)
    with pytest.raises(NotImplementedError):
        cm_arch.cm_unet_spec(**kw)


@pytest.fixture(scope='module')
def lsun16():
    return CMDenoiser.from_config('lsun_bedroom', device='cpu', use_fp16=True)


def _convs(P):
    lib = _lib.load()
    return [(op.name, op.keep[0], P.kernel_ids[op.name]) for op in P.ops if op.fn is lib.ds_conv2d_nhwc]


@pytest.mark.parametrize('B', [1, 3])
def test_lsun_fp16_plan_runs_its_wide_block_convolutions_on_fp16_rows(lsun16, B):
    eng = lsun16.engine
    eng.wide16 = True
    P = eng.plan(B, 1)
    assert P.stream16
    convs = _convs(P)
    assert not [n for n, a, kid in convs if kid == 0]                                   # nothing on the generic gather kernel
    wide = [(n, a, kid) for n, a, kid in convs if a.taps == 9 and a.w >= 128 and a.cout >= 64]      # (the head, cout = 3, is the thin kernel's)
    assert len(wide) == 26 and {a.w for _, a, _ in wide} == {128, 256}
    assert all(a.in_f16 and kid in WIDE_IDS for _, a, kid in wide), [(n, kid) for n, a, kid in wide if kid not in WIDE_IDS]
    assert all((kid == 2576) == bool(a.ec0) for _, a, kid in wide) and any(a.ec0 for _, a, _ in wide)
    assert all(a.cbias for n, a, _ in wide if n.endswith('.conv0'))                      # the embedding row rides in conv0 (no scale / shift)
    assert all(a.out_f16 for _, a, _ in wide)
    # the routes at B = 1 and B = 3 are the same: no decision of the wide kernel depends on the batch
    other = eng.plan(4 - B, 1)
    wide_sig = lambda plan: [s for s in _routing.signature(plan) if dict(s[2:]).get('kernel') in WIDE_IDS]
    assert len(wide_sig(P)) == 26 and wide_sig(P) == wide_sig(other)


def test_lsun_fp16_plan_without_wide16_takes_the_fp32_routes_above_64_pixels(lsun16):
    eng = lsun16.engine
    try:
        eng.wide16 = False
        P = eng.plan(1, 1)
    finally:
        eng.wide16 = True
    assert not P.stream16
    wide = [(n, a, kid) for n, a, kid in _convs(P) if a.taps == 9 and a.w >= 128 and a.cout >= 64]
    assert len(wide) == 26 and all(not a.in_f16 and kid not in WIDE_IDS for _, a, kid in wide)
    narrow = [(n, a, kid) for n, a, kid in _convs(P) if a.taps == 9 and a.w <= 64 and a.cout >= 64 and (a.stride or 1) == 1]
    assert narrow and all(a.in_f16 and kid in (2566, 2572) for _, a, kid in narrow)


@pytest.mark.parametrize('config,B', [('tiny_song', 4), ('imagenet64', 2)])
def test_wide16_changes_no_plan_without_a_layer_above_64_pixels(config, B):
    from diff_sampler_amd.engine import EDMDenoiser
    sig = []
    for flag in (True, False):
        net = EDMDenoiser.from_config(config, device='cpu', use_fp16=True, wide16=flag)
        assert net.engine.wide16 == flag
        sig.append(_routing.signature(net.engine.plan(B, 1)))
    assert sig[0] == sig[1], _routing.diff(sig[0], sig[1])


def test_create_model_returns_a_cm_net():
    from diff_sampler_amd import sample
    net, source = sample.create_model('lsun_bedroom', random_init=True, device='cpu')
    assert source == 'cm' and isinstance(net, CMDenoiser) and not net.use_fp16
    assert (net.img_resolution, net.img_channels, net.label_dim, net.sigma_min, net.sigma_max, net.sigma_data) == (256, 3, 0, 0.002, 80.0, 0.5)
    assert float(net.round_sigma(1.5)) == 1.5 and net.bottleneck_name == 'dec.8x8_in1'
    assert net.max_plan_batch == 15


def test_batch_ceiling_and_sub_batches():
    spec = cm_arch.cm_precond_spec('lsun_bedroom')
    assert plan_elements_per_image(spec) == 256 * 256 * 512                # the concatenated level-0 input: 2**31 elements at 64 images
    assert (2 ** 31 - 1) // (4 * plan_elements_per_image(spec)) == 15
    assert split_batch(5, 2) == [(0, 2), (2, 4), (4, 5)]
    assert split_batch(64, 15) == [(0, 15), (15, 30), (30, 45), (45, 60), (60, 64)]
    assert split_batch(15, 15) == [(0, 15)] and split_batch(1, 15) == [(0, 1)]
    with pytest.raises(ValueError):
        split_batch(4, 0)
    tiny = cm_arch.cm_precond_spec('tiny_cm_wide')
    assert (2 ** 31 - 1) // (4 * plan_elements_per_image(tiny)) >= 64
