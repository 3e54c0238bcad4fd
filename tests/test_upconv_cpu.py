"""CPU: the upsampled-input 3x3 convolution (ds_conv_args.in_up2) -- weight folding, the plans that use it, the arguments the route refuses.

conv3x3(nearest_x2(x), pad 1) collapses, per output phase (row & 1, col & 1), onto a 2x2 neighbourhood of the low-res image whose weights are
sums of the 3x3 kernel's (ops.fold_conv_weight_up2).  Plans and ds_conv_route are host logic: nothing here launches a kernel."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import diff_sampler_amd.arch as arch  # noqa: E402
from diff_sampler_amd import _lib, ops  # noqa: E402
from diff_sampler_amd._lib import DS_RESAMPLE_NONE  # noqa: E402
from diff_sampler_amd.engine import UNetEngine  # noqa: E402

DS_E_ARG, DS_E_SHAPE = -1, -3          # include/ds_engine.h


def phase_conv(x, folded):
    """The definition in ds_engine.h evaluated with torch: out[2y+py, 2x+px] = sum_{a,b} W[py][px][a][b] . x[y+py-1+a, x+px-1+b]."""
    n, _, h, w = x.shape
    out = x.new_zeros(n, folded.shape[1], 2 * h, 2 * w)
    xp = F.pad(x, (1, 1, 1, 1))
    for py in range(2):
        for px in range(2):
            out[:, :, py::2, px::2] = F.conv2d(xp[:, :, py:py + h + 1, px:px + w + 1], folded[py * 2 + px])
    return out


def test_folded_phase_kernels_reproduce_the_upsampled_convolution_in_fp64():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 5, 6, 6, generator=g, dtype=torch.float64)
    w = torch.randn(7, 5, 3, 3, generator=g, dtype=torch.float64)
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode='nearest'), w, padding=1)
    got = phase_conv(x, ops.fold_conv_weight_up2(w))
    assert float((got - ref).abs().max()) <= 1e-12


def test_pack_conv_weight_up2_k_order_and_row_padding():
    g = torch.Generator().manual_seed(4)
    cout, cin = 70, 64
    w = torch.randn(cout, cin, 3, 3, generator=g)
    f = ops.fold_conv_weight_up2(w)                       # [4, cout, cin, 2, 2]
    p = ops.pack_conv_weight_up2(w)
    assert p.shape == (4, 128, 4 * cin) and p.dtype == torch.float32 and p.is_contiguous()
    assert float(p[:, cout:].abs().max()) == 0.0          # rows padded with zeros to the 128-column tile
    for ph in range(4):
        for chunk in range(cin // 32):
            for a in range(2):
                for b in range(2):
                    k0 = (chunk * 4 + a * 2 + b) * 32
                    assert torch.equal(p[ph, :cout, k0:k0 + 32], f[ph, :, chunk * 32:chunk * 32 + 32, a, b])
    # one phase matrix is what pack_conv_weight would make of a 2x2 kernel: same chunk-major, tap-minor order
    assert torch.equal(p[3, :cout], ops.pack_conv_weight(f[3])[:cout])


def _engine(name, **kw):
    spec = arch.edm_precond_spec(**dict(arch.NAMED_CONFIGS[name]))
    return spec, UNetEngine(spec, arch.init_params(spec, seed=1), device='cpu', **kw)


@pytest.fixture(scope='module')
def cifar10():
    return _engine('cifar10')


def _convs(P, lib):
    return [(op.name, op.keep[0]) for op in P.ops if op.fn is lib.ds_conv2d_nhwc]


@pytest.mark.parametrize('B', [8, 64, 256])
def test_cifar10_fp32_plans_run_the_up_blocks_conv0_on_the_low_res_rows(cifar10, B):
    lib = _lib.load()
    spec, eng = cifar10
    P = eng.plan(B, 1)
    assert len(P.ops) == 178
    ups = {b.name: b for b in spec.blocks if b.kind == 'block' and b.up}
    assert len(ups) == 2
    got = {n: a for n, a in _convs(P, lib) if a.in_up2}
    assert set(got) == {n + '.conv0' for n in ups}            # exactly the up blocks' conv0, the 8 -> 16 layer included
    names = [op.name for op in P.ops]
    for n, b in ups.items():
        a = got[n + '.conv0']
        assert (a.taps, a.stride or 1, a.h, a.w, a.wgt_f16, a.in_f16) == (9, 1, b.res_out, b.res_out, 0, 0)
        assert not a.norm_coefs and not a.e0 and not a.res and a.stats_out
        i = names.index(n + '.conv0')
        assert names[i - 1] == n + '.norm0' and P.ops[i - 1].fn is lib.ds_norm_act
        na = P.ops[i - 1].keep[0]
        assert (na.resample, na.h, na.w) == (DS_RESAMPLE_NONE, b.res_in, b.res_in)     # the pass stays, at the input resolution
        assert na.out == a.x0
        if B == 256:
            assert lib.ds_conv_kernel_id(C.byref(a)) == 2565
        assert lib.ds_conv_kernel_id(C.byref(a)) in (2565, 256, 128, 1284)
    P.close()
    eng._plans.clear()


def test_up_phase_off_restores_the_upsampling_pass():
    lib = _lib.load()
    spec, eng = _engine('cifar10', up_phase=False)
    P = eng.plan(64, 1)
    assert len(P.ops) == 178 and not any(a.in_up2 for _, a in _convs(P, lib))
    assert not any(k.endswith('.wup') for k in eng.w)


@pytest.mark.parametrize('kw', [dict(split_fp16=True), dict(use_fp16=True)])
def test_reduced_operand_modes_do_not_use_the_mode(kw):
    lib = _lib.load()
    spec, eng = _engine('cifar10', **kw)
    assert not any(k.endswith('.wup') for k in eng.w)
    assert not any(a.in_up2 for _, a in _convs(eng.plan(8, 1), lib))


def test_latent_diffusion_and_vae_plans_do_not_use_the_mode():
    lib = _lib.load()
    import diff_sampler_amd.ldm_arch as la
    from diff_sampler_amd.ldm_engine import LDMUNetEngine
    from diff_sampler_amd.vae_engine import VAEDecoder
    lspec = la.ldm_unet_spec(**dict(la.NAMED_LDM_CONFIGS['tiny_ldm']))
    P = LDMUNetEngine(lspec, la.init_ldm_params(lspec, seed=1), device='cpu').plan(4, 4, 77)
    ops_ = list(P.ops) + list(P.ctx.ops if getattr(P, 'ctx', None) is not None else [])
    assert not any(op.keep[0].in_up2 for op in ops_ if op.fn is lib.ds_conv2d_nhwc)
    for fp16 in (False, True):
        P = VAEDecoder.from_config('tiny_vae', seed=0, device='cpu', use_fp16=fp16).plan(2)
        assert not any(op.keep[0].in_up2 for op in P.ops if op.fn is lib.ds_conv2d_nhwc)


def _args(n=4, h=32, cin=64, cout=256, **kw):
    """A valid in_up2 call (addresses are only looked at: non-null, 16-byte aligned)."""
    a = _lib.ConvArgs(0x10000, None, cin, 0, cin, 0, n, h, h, 9, 0x20000, cout, 0x30000, None, 0, 1, None, 0, 1.0, 0, 0x40000, cout)
    a.in_up2 = 1
    a.tune.mode = a.tune.variant = 0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _route(a):
    info = _lib.ConvRouteInfo()
    rc = _lib.load().ds_conv_route(C.byref(a), C.byref(info))
    assert _lib.load().ds_conv_kernel_id(C.byref(a)) == (rc if rc else info.kernel_id)
    return rc, info


def test_route_takes_the_mode_and_never_splits():
    for n in (1, 4, 256):
        rc, info = _route(_args(n=n, workspace=0x50000, workspace_floats=1 << 30))
        assert rc == 0 and info.splits == 1 and info.kernel_id in (2565, 256, 128, 1284)
    rc, info = _route(_args(n=256, stats_out=0x60000))
    assert rc == 0 and info.kernel_id == 2565
    rc, info = _route(_args(n=256, h=16, stats_out=0x60000))       # four 8x8 low-res images per 256-pixel tile
    assert rc == 0 and info.kernel_id == 2565


@pytest.mark.parametrize('kw,code', [
    (dict(taps=1), DS_E_ARG),
    (dict(stride=2), DS_E_ARG),
    (dict(h=31), DS_E_SHAPE),
    (dict(norm_coefs=0x70000), DS_E_ARG),
    (dict(e0=0x70000, ec0=64, eld0=64), DS_E_ARG),
    (dict(wgt_f16=1), DS_E_ARG),
    (dict(wgt_f16=2), DS_E_ARG),
    (dict(res=0x70000, res_ld=256), DS_E_ARG),
    (dict(in_up2=2), DS_E_ARG),
    (dict(cout=320), DS_E_SHAPE),                     # would leave a 64-column tail tile
    (dict(h=8, stats_out=0x60000), DS_E_SHAPE),       # 4x4 low-res image: no whole 64-row statistics block per phase
])
def test_route_refuses(kw, code):
    rc, _ = _route(_args(**kw))
    assert rc == code
    a = _args(**kw)
    a.in_up2 = 0
    if set(kw) <= {'h', 'cout', 'stats_out'}:
        assert _route(a)[0] == 0                      # the same call without the mode is an ordinary layer


def test_conv_args_struct_ends_with_the_new_field():
    fields = [f[0] for f in _lib.ConvArgs._fields_]
    assert fields[-2:] == ['update', 'in_up2']
    assert _lib.load().ds_version() == 7
