"""CPU: the batch-invariant mode's routing (ds_conv_tune.invariant, ABI 6) over every configuration's full batch range and both sigma forms.

An invariant plan must route every launch the same way at every batch: same entry points, same kernel families, no split-K, the fp32 attention
on one work split, the GroupNorm statistics without the small-batch form.  Kernel ids whose outputs are bit-identical are mapped to one chain
class (the fp32 halo tiles 128 / 256 / 2565; the 1x1 GEMM kernels 0 / 2561), and these fields are ignored because the kernels' results
do not depend on them: the fp16-activation column-tile widths (each output is the same K-ordered fp32 sum under any width, and layers that
leave column sums through the staged epilogue get the widest tiles in this mode) and the thin head's rounds (not in the signature).
tests/test_hip_batch_invariant.py shows the chain classes bit-identical on the GPU."""
import ctypes as C
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import _routing  # noqa: E402
from diff_sampler_amd import _lib  # noqa: E402

CONFIGS = list(_routing.CONFIGS) + ['tiny_song']
# kernel ids the invariant route may pick interchangeably: shown bit-identical by tests/test_hip_batch_invariant.py
CHAIN_CLASS = {128: 'fp32_halo', 256: 'fp32_halo', 2565: 'fp32_halo', 0: 'fp32_gemm', 2561: 'fp32_gemm'}
IGNORED = ('f16_widths',)


def _engine(config, invariant):
    net, kind, kw, _, _ = _routing._cfg(config)
    kw = dict(kw, batch_invariant=invariant)
    if kind == 'edm':
        import diff_sampler_amd.arch as arch
        from diff_sampler_amd.engine import UNetEngine
        spec = arch.edm_precond_spec(**dict(arch.NAMED_CONFIGS[net]))
        return UNetEngine(spec, arch.init_params(spec, seed=1), device='cpu', **kw)
    import diff_sampler_amd.ldm_arch as la
    from diff_sampler_amd.ldm_engine import LDMUNetEngine
    spec = la.ldm_unet_spec(**dict(la.NAMED_LDM_CONFIGS[net]))
    return LDMUNetEngine(spec, la.init_ldm_params(spec, seed=1), device='cpu', **kw)


def _canonical(sig):
    out = []
    for launch in sig:
        fields = []
        for k, v in launch[2:]:
            if k in IGNORED:
                continue
            if k == 'kernel':
                v = CHAIN_CLASS.get(v, v)
            fields.append((k, v))
        out.append(launch[:2] + tuple(fields))
    return tuple(out)


def _plans(eng, config, B):
    for rows in _routing.sigma_forms(config, B):
        P = _routing.plan_of(eng, config, B, rows)
        yield rows, P
        P.close()
        eng._plans.clear()


@pytest.mark.parametrize('config', CONFIGS)
def test_invariant_plans_route_every_batch_and_sigma_form_the_same(config):
    eng = _engine(config, True)
    lib = _lib.load()
    ref, where = None, None
    for B in _routing._cfg(config)[3]:
        for rows, P in _plans(eng, config, B):
            for op in P.ops:
                if op.fn is lib.ds_conv2d_nhwc:
                    a = op.keep[0]
                    assert a.tune.invariant & 1, (config, B, op.name)
                    assert _routing.conv_route(a).splits == 1, (config, B, rows, op.name)
                elif op.fn is lib.ds_gn_stats:
                    assert not op.keep[0].partial, (config, B, op.name)
            sig = _canonical(_routing.signature(P))
            if ref is None:
                ref, where = sig, (B, rows)
            assert sig == ref, (config, where, (B, rows), _routing.diff(list(ref), list(sig)))


@pytest.mark.parametrize('config', CONFIGS)
def test_both_sigma_forms_route_the_embedding_path_identically(config):
    """The embedding projections run on the row kernel (2573) in both forms wherever it applies -- one row or one row per image."""
    eng = _engine(config, True)
    lib = _lib.load()
    for B in sorted({1, 5, _routing._cfg(config)[4]} & set(_routing._cfg(config)[3])):
        routes = []
        for rows, P in _plans(eng, config, B):
            emb = [(op.name, _routing.conv_route(op.keep[0]).kernel_id) for op in P.ops
                   if op.fn is lib.ds_conv2d_nhwc and op.keep[0].tune.invariant & 2]
            assert emb, (config, B)
            routes.append(emb)
        assert all(r == routes[0] for r in routes), (config, B, routes)
        assert any(k == 2573 for _, k in routes[0]), (config, B, routes[0])


@pytest.mark.parametrize('config', ['cifar10_fp32', 'sd15_fp16', 'tiny_song'])
def test_default_plans_carry_no_invariant_flag(config):
    """batch_invariant=False is the default: no launch of such a plan carries the flag, and an engine built with the keyword set to False
    routes like one built without it.  (That default routing equals the parent's is shown by tests/test_batch_routing_cpu.py, whose
    boundary map and sweep table are unchanged.)"""
    eng, eng_default = _engine(config, False), _routing.make_engine(config)
    lib = _lib.load()
    for B in sorted({1, 4, 5, _routing._cfg(config)[4]} & set(_routing._cfg(config)[3])):
        for rows in _routing.sigma_forms(config, B):
            P, Q = _routing.plan_of(eng, config, B, rows), _routing.plan_of(eng_default, config, B, rows)
            assert _routing.signature(P) == _routing.signature(Q), (config, B, rows)
            assert all(op.keep[0].tune.invariant == 0 for op in P.ops if op.fn is lib.ds_conv2d_nhwc)
            P.close(); Q.close()
            eng._plans.clear(); eng_default._plans.clear()


def test_abi_6_and_the_row_kernel_at_any_row_count():
    lib = _lib.load()
    assert lib.ds_version() == 7
    assert C.sizeof(_lib.ConvTune) == 7 * C.sizeof(C.c_int)
    from diff_sampler_amd.plan import Builder
    import torch
    for rows in (1, 4, 5, 256):
        bd = Builder('cpu', invariant=True, batch=rows)
        x, w = torch.zeros(rows, 512), torch.zeros(1024, 512)
        out = torch.zeros(rows, 1024)
        bd.linear(x, 512, rows, w, 1024, out, 'emb', bias=torch.zeros(1024), emb=True)
        bd.linear(x, 512, rows, w, 1024, out, 'rows')
        emb, plain = (_routing.conv_route(op.keep[0]) for op in bd.P.ops)
        assert emb.kernel_id == 2573 and emb.splits == 1, rows
        assert plain.kernel_id != 2573 and plain.splits == 1, rows
    # the default route keeps its <= 4-row rule
    for rows, want in ((4, True), (5, False)):
        bd = Builder('cpu')
        x, w, out = torch.zeros(rows, 512), torch.zeros(1024, 512), torch.zeros(rows, 1024)
        bd.linear(x, 512, rows, w, 1024, out, 'emb', emb=True)
        assert (_routing.conv_route(bd.P.ops[0].keep[0]).kernel_id == 2573) == want, rows


def test_cli_has_the_batch_invariant_option():
    from diff_sampler_amd import sample
    names = {p.name for p in sample.main.params}
    assert 'batch_invariant' in names
