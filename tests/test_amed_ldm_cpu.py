"""CPU-only: the fixtures of the AMED-on-latent-diffusion route -- the golden file (tests/golden/amed_ldm_tiny.npz), the test-size U-Net whose
middle block is the 8x8 tap the AMED predictor needs, the two new plan operations of the C ABI, and (where the reference tree is present) that the
generator's own functions reproduce a stored trajectory."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, 'tests', 'golden', 'amed_ldm_tiny.npz')
TAGS = ('dpmpp2_eps_afs', 'dpmpp2_x0', 'amed', 'ipndm3', 'euler', 'dpm2')


def test_golden_keys_and_shapes():
    z = np.load(GOLD)
    assert os.path.getsize(GOLD) < 1 << 20
    assert str(z['config']) == 'tiny_ldm_amed' and int(z['seed']) == 61 and int(z['pred_seed']) == 900
    assert z['latents'].shape == (2, 4, 32, 32) and z['cond'].shape == z['uncond'].shape == (2, 7, 64)
    spec = json.loads(str(z['cases_json']))
    assert spec['common'] == dict(num_steps=4, schedule_type='discrete', schedule_rho=1, guidance_rate=7.5)
    assert tuple(spec['cases']) == TAGS
    recipe = spec['cases']['dpmpp2_eps_afs']           # the reference's Stable Diffusion recipe (amed-solver-main/launch.sh:55-62)
    assert recipe == dict(student='dpmpp', afs=True, scale_dir=0, scale_time=0.2, kwargs=dict(max_order=2, predict_x0=False, lower_order_final=True))
    assert {c['student'] for c in spec['cases'].values()} == {'amed', 'euler', 'ipndm', 'dpm', 'dpmpp'}
    for tag in TAGS:
        tr = z[f'{tag}_inters']
        assert tr.shape == (4, 2, 4, 32, 32) and tr.dtype == np.float32 and np.isfinite(tr).all()
        assert np.allclose(tr[0], z['latents'] * float(z['sigma_max']), rtol=1e-5)              # x_0 = latents * t_0
    assert z['tap_x'].shape == (2, 4, 32, 32) and z['tap_out'].shape == (4, 128, 8, 8) and z['tap_denoised'].shape == (2, 4, 32, 32)
    for pre in ('tap_', 'tap_afs_'):
        for k in ('r', 'scale_dir', 'scale_time'):
            assert z[pre + k].shape == (2, 1, 1, 1)
    assert np.ptp(z['tap_afs_r']) == 0 and np.ptp(z['tap_r']) > 0           # under AFS every sample sees the same zeros
    ps, pc = z['probe_sigma'], z['probe_c_noise']
    assert ps.shape == pc.shape == (64,) and ps.dtype == pc.dtype == np.float32 and (np.diff(ps) > 0).all()
    assert np.isclose(ps[0], float(z['sigma_min']) / 2) and np.isclose(ps[-1], 2 * float(z['sigma_max']))
    assert pc[0] < 0 and pc[-1] > 999 and (np.diff(pc) > 0).all()            # both linear extensions are hit


def test_tiny_ldm_amed_has_the_8x8_tap():
    import diff_sampler_amd.ldm_arch as la
    spec = la.ldm_unet_spec(**la.NAMED_LDM_CONFIGS['tiny_ldm_amed'])
    mid = [b for b in spec.blocks if b.name == 'middle_block'][0].layers
    assert [l.key for l in mid] == ['middle_block.0', 'middle_block.1', 'middle_block.2']
    assert (mid[-1].cout, mid[-1].res_out) == (128, 8)
    sd = la.ldm_unet_spec(**la.NAMED_LDM_CONFIGS['sd15'])
    assert [(l.cout, l.res_out) for b in sd.blocks for l in b.layers if l.key == 'middle_block.2'] == [(1280, 8)]


def test_new_plan_operations_are_bound():
    """The two launches are plan operations (DS_OP_CHANNEL_MEAN_F16, DS_OP_CFG_SIGMA_ROWS), not entry points of their own: the set of
    exported symbols is the parent's.  ds_plan_add is host bookkeeping, so the argument structs' sizes are checked here without a GPU."""
    import ctypes as C
    from diff_sampler_amd import _lib, ops
    assert (_lib.DS_OP_CHANNEL_MEAN_F16, _lib.DS_OP_CFG_SIGMA_ROWS) == (17, 18)
    assert 'ds_channel_mean_f16' not in _lib.EXPORTS and 'ds_cfg_sigma_rows' not in _lib.EXPORTS
    assert callable(ops.channel_mean_f16) and callable(ops.cfg_sigma_rows)
    header = open(os.path.join(ROOT, 'include', 'ds_engine.h')).read()
    assert 'DS_OP_CHANNEL_MEAN_F16 = 17' in header and 'DS_OP_CFG_SIGMA_ROWS = 18' in header
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.ds_plan_create(C.byref(h)) == 0
    try:
        for op, args in ((_lib.DS_OP_CHANNEL_MEAN_F16, _lib.ChannelMeanF16Args()), (_lib.DS_OP_CFG_SIGMA_ROWS, _lib.CfgSigmaRowsArgs())):
            assert lib.ds_plan_add(h, op, C.byref(args), C.sizeof(args)) == 0
            assert lib.ds_plan_add(h, op, C.byref(args), C.sizeof(args) - 4) != 0           # wrong struct size
        assert lib.ds_plan_size(h) == 2
        assert lib.ds_plan_add(h, 19, C.byref(args), C.sizeof(args)) != 0                   # no such operation
    finally:
        lib.ds_plan_destroy(h)


def test_generator_reproduces_a_stored_trajectory():
    """tools/gen_golden_amed_ldm.py, run on the real reference, gives the stored bits again (development machine only).  In an interpreter
    of its own: the generator imports the reference's top-level modules (solvers_amed, solver_utils, models, training)."""
    import subprocess
    from oracle import gen_golden
    if not os.path.isdir(os.path.join(gen_golden.REF, 'amed-solver-main')):
        pytest.skip('the reference tree is not on this machine')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'gen_golden_amed_ldm.py'), '--check', 'ipndm3'], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-1500:])
