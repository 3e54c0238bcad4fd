"""CPU: the Winograd F(2x2, 3x3) weight packing (ops.pack_conv_weight_wino) and the routing of ds_conv_args.wino (host logic only).

The packing test applies the packed tensor in fp64 Winograd arithmetic and compares with F.conv2d at 1e-12 of the output absmax: it pins G,
the layout and the row padding.  The weights are multiples of 2**-10 below 1 in magnitude, so that U = G g G^T (sums of at most nine of them
times 1/4) has at most 16 significant bits and the packing's single rounding to fp32 is exact -- the bound then measures the transform, not
the storage format."""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

DS_E_ARG, DS_E_SHAPE = -1, -3


def _unpack(U, cout, cin):
    """[cout_pad / 64][cin / 8][16][2][64][4] -> [16][cout][cin]"""
    nt, ns = U.shape[:2]
    return U.permute(2, 0, 4, 1, 3, 5).reshape(16, nt * 64, ns * 8)[:, :cout, :cin]


def _wino_fp64(x, U, cout):
    """The kernel's arithmetic in fp64: pad, 4x4 patches at stride 2, V = B^T d B, per-position channel sums with U, Y = A^T M A."""
    from diff_sampler_amd.ops import WINO_AT, WINO_BT
    n, cin, H, W = x.shape
    BT, AT = torch.tensor(WINO_BT, dtype=torch.float64), torch.tensor(WINO_AT, dtype=torch.float64)
    d = F.pad(x, (1, 1, 1, 1)).unfold(2, 4, 2).unfold(3, 4, 2)                   # n, c, ty, tx, 4, 4
    V = torch.einsum('ik,nctxkl,jl->ijntxc', BT, d, BT)
    M = torch.einsum('ijntxc,ijoc->ijntxo', V, U.reshape(4, 4, cout, cin))
    return torch.einsum('ai,ijntxo,bj->notaxb', AT, M, AT).reshape(n, cout, H, W)


@pytest.mark.parametrize('cout', [64, 96])
def test_packing_reproduces_conv2d_in_fp64(cout):
    from diff_sampler_amd.ops import pack_conv_weight_wino
    g = torch.Generator().manual_seed(3)
    cin = 32
    w = torch.randint(-1023, 1024, (cout, cin, 3, 3), generator=g).double() / 1024
    x = torch.randn(2, cin, 8, 6, generator=g, dtype=torch.float64)
    U = pack_conv_weight_wino(w.float())
    assert U.dtype == torch.float32 and tuple(U.shape) == (-(-cout // 64), cin // 8, 16, 2, 64, 4)
    u = U.double().permute(2, 0, 4, 1, 3, 5).reshape(16, U.shape[0] * 64, cin)
    assert bool((u[:, cout:] == 0).all())                                       # rows zero-padded to the 64-column tile
    got = _wino_fp64(x, _unpack(U.double(), cout, cin), cout)
    ref = F.conv2d(x, w, padding=1)
    err = float((got - ref).abs().max() / ref.abs().max())
    print(f'wino packing cout {cout}: rel err {err:.3e}')
    assert err < 1e-12


def test_packing_appends_the_skip_columns_untransformed():
    from diff_sampler_amd.ops import pack_conv_weight_wino
    g = torch.Generator().manual_seed(4)
    w, ws = torch.randn(64, 32, 3, 3, generator=g), torch.randn(64, 96, 1, 1, generator=g)
    flat = pack_conv_weight_wino(w, extra=ws)
    U = pack_conv_weight_wino(w)
    assert flat.dim() == 1 and flat.numel() == U.numel() + 64 * 96
    assert torch.equal(flat[:U.numel()], U.reshape(-1))
    e = flat[U.numel():].reshape(1, 3, 4, 2, 64, 4).permute(0, 4, 1, 2, 3, 5).reshape(64, 96)      # (nt, row, slab, group, kh, e)
    assert torch.equal(e, ws.reshape(64, 96))


def test_wino_member_sits_in_the_tail_padding_of_the_args_struct():
    """`int wino` follows in_up2 in ds_conv_args and takes what was tail padding: the ctypes mirror keeps its field list and size, exposes the
    member as a property on those four bytes, and the library reads it there (the route answers wino = 1 only when it is set)."""
    import ctypes as C
    from diff_sampler_amd import _lib
    assert C.sizeof(_lib.ConvArgs) == _lib.ConvArgs.in_up2.offset + 8 and _lib.ConvArgs.in_up2.offset % 8 == 0
    a, keep = _conv_args()
    assert a.wino == 1 and a.in_up2 == 0
    raw = bytes(a)
    assert raw[-4:] == (1).to_bytes(4, sys.byteorder) and raw[-8:-4] == bytes(4)
    assert _route(a)[1].wino == 1
    a.wino = 0
    assert a.wino == 0 and bytes(a)[-8:] == bytes(8)
    rc, info = _route(a)
    assert rc == 0 and info.wino == 0 and info.kernel_id == 2565


def _plan_conv_ops(eng, B):
    from diff_sampler_amd import _lib
    lib = _lib.load()
    P = eng.plan(B, B)
    return P, [op for op in P.ops if op.fn is lib.ds_conv2d_nhwc]


def _route(a):
    from diff_sampler_amd import _lib
    info = _lib.ConvRouteInfo()
    rc = _lib.load().ds_conv_route(C.byref(a), C.byref(info))
    return rc, info


def _engine(**kw):
    import diff_sampler_amd.arch as arch
    from diff_sampler_amd.engine import UNetEngine
    spec = arch.edm_precond_spec(**dict(arch.NAMED_CONFIGS['cifar10']))
    return UNetEngine(spec, arch.init_params(spec, seed=1), device='cpu', **kw)


def test_routing_of_the_headline_plan():
    """cifar10 at B = 256: the library reports wino == 1 on exactly the launches the engine asked for, each of them is kernel id 2565 without
    split-K, and the (kernel id, split-K) of every launch is what it is with the flag off."""
    on, off = _engine(), _engine(winograd=False)
    P1, ops1 = _plan_conv_ops(on, 256)
    P0, ops0 = _plan_conv_ops(off, 256)
    assert [o.name for o in ops1] == [o.name for o in ops0] and len(P1.ops) == len(P0.ops)
    n_w = 0
    for o1, o0 in zip(ops1, ops0):
        rc1, r1 = _route(o1.keep[0])
        rc0, r0 = _route(o0.keep[0])
        assert rc1 == 0 and rc0 == 0, (o1.name, rc1, rc0)
        assert r1.wino == o1.keep[0].wino, o1.name
        assert r0.wino == 0 and o0.keep[0].wino == 0, o0.name
        assert (r1.kernel_id, r1.splits) == (r0.kernel_id, r0.splits), o1.name
        if r1.wino:
            assert o1.keep[0].taps == 9 and r1.kernel_id == 2565 and r1.splits == 1, o1.name
            n_w += 1
    # every non-up2 launch of kernel id 2565: 40 on the headline plan
    want = sum(1 for o in ops0 if _route(o.keep[0])[1].kernel_id == 2565 and not o.keep[0].in_up2)
    print(f'cifar10 B=256: {n_w} Winograd launches of {want} direct 2565 launches')
    assert want == 40 and n_w == want
    P1.close(); P0.close()


@pytest.mark.parametrize('kw,B', [(dict(winograd=False), 256), (dict(batch_invariant=True), 256), (dict(use_fp16=True), 256),
                                  (dict(split_fp16=True), 256), (dict(), 8)])
def test_no_winograd_launches(kw, B):
    eng = _engine(**kw)
    P, ops = _plan_conv_ops(eng, B)
    for o in ops:
        rc, r = _route(o.keep[0])
        assert rc == 0 and r.wino == 0 and o.keep[0].wino == 0, o.name
    assert not any(k.endswith('.wwino') for k in eng.w) or not kw
    P.close()


def _conv_args(B=2, H=16, W=16, c0=64, cout=256, **fields):
    from diff_sampler_amd import _lib
    from diff_sampler_amd.ops import pack_conv_weight_wino
    x = torch.zeros(B * H * W, c0)
    wp = pack_conv_weight_wino(torch.zeros(cout, c0, 3, 3))
    out = torch.zeros(B * H * W, cout)
    a = _lib.ConvArgs(x.data_ptr(), None, c0, 0, c0, 0, B, H, W, 9, wp.data_ptr(), cout, None, None, 0, 1, None, 0, 1.0, 0, out.data_ptr(), cout)
    a.wino = 1
    a.tune.mode, a.tune.variant = 256, 6
    for k, v in fields.items():
        if k.startswith('tune_'):
            setattr(a.tune, k[5:], v)
        else:
            setattr(a, k, v)
    return a, (x, wp, out)


@pytest.mark.parametrize('fields,shape,code', [
    (dict(), dict(), 2565),                                         # the accepted form of the same call
    (dict(), dict(H=15, W=15), DS_E_SHAPE),                         # odd H, W
    (dict(), dict(cout=320), DS_E_SHAPE),                           # a 64-column tail behind the 256-column tile
    (dict(in_up2=1), dict(), DS_E_ARG),
    (dict(tune_invariant=1), dict(), DS_E_ARG),
    (dict(stride=2), dict(), DS_E_ARG),
    (dict(wgt_f16=2), dict(), DS_E_ARG),
    (dict(tune_mode=1), dict(), DS_E_ARG),                          # forced generic route
    (dict(tune_mode=128), dict(), DS_E_ARG),                        # forced 128-pixel tiles
    (dict(tune_variant=7), dict(), DS_E_ARG),                       # forced 256 x 128 tiles
    (dict(tune_mode=0, tune_variant=0), dict(), DS_E_SHAPE),        # the default route of this small layer is not the 256 x 256 tile
])
def test_refusals_return_the_documented_code(fields, shape, code):
    from diff_sampler_amd import _lib
    lib = _lib.load()
    a, keep = _conv_args(**shape, **fields)
    assert lib.ds_conv_kernel_id(C.byref(a)) == code
    rc, info = _route(a)
    if code > 0:
        assert rc == 0 and info.kernel_id == code and info.wino == 1 and info.splits == 1
    else:
        assert rc == code
