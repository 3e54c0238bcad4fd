"""The five attention kernels (ds_attention in both work splits, ds_attention_f16, ds_attention_causal, dsm_attention) per element against
tests/_attn_refs.py: the exact family to the last bit the arithmetic allows (2 ulp), the generic family against fp64 softmax with the
bounds derived there.  Every operand buffer holds NaN in its padding columns and in the rows at and beyond sq / skv, every output is
NaN-prefilled with padding columns and spare rows that must still hold NaN afterwards.  tests/test_attn_refs_cpu.py proves the case
table's coverage and that the exact family bites."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _attn_refs as A  # noqa: E402

pytestmark = pytest.mark.gpu

IDS = [c.name for c in A.CASES]
NAMES = ('q', 'k', 'v', 'out')


def _libs():
    from diff_sampler_amd import _lib, _metrics_lib
    return _lib, _lib.load(), _metrics_lib, _metrics_lib.load()


def _launch(kernel, f):
    L, lib, M, mlib = _libs()
    if kernel == 'm88':
        f = dict(f)
        res = (C.c_int * 3)(f.pop('out_f16'), f.pop('in_f16'), f.pop('variant'))
        return mlib.dsm_attention(C.byref(M.DsmAttnArgs(reserved=res, **f)), L.stream_ptr())
    fn = {'f32': lib.ds_attention, 'f16': lib.ds_attention_f16, 'causal': lib.ds_attention_causal}[kernel]
    return fn(C.byref(L.AttnArgs(**f)), L.stream_ptr())


class Dev:
    """A case's operands on the device in the layout of _attn_refs.pack."""

    def __init__(self, case, q, k, v, fill='nan'):
        self.case = case
        self.t, self.ld, self.bs = {}, {}, {}
        for n, (name, x) in enumerate(zip(NAMES, A.as_operands(case, q, k, v))):
            buf, self.ld[name], self.bs[name] = A.pack(x, x.dtype, fill, seed=n)
            self.t[name] = torch.from_numpy(buf).cuda()

    def run(self, scale, variant=None):
        """One launch into a fresh NaN-prefilled output; the live block as fp64 [batch, sq, heads, d] (guards checked)."""
        case = self.case
        buf, self.ld['out'], self.bs['out'] = A.out_buffer(case)
        out = torch.from_numpy(buf).cuda()
        f = A.fields(case, {n: self.t[n].data_ptr() for n in NAMES[:3]} | {'out': out.data_ptr()}, self.ld, self.bs, scale)
        if variant is not None:
            f['variant'] = variant
        rc = _launch(case.kernel, f)
        torch.cuda.synchronize()
        assert rc == 0, (case.name, rc)
        return A.unpack_out(case, out.cpu().numpy())

    def run_rows(self, scale, b, h, rows, variant):
        """Image b, head h alone (batch = heads = 1 at a pointer offset): the queries `rows` one launch each with sq = 1 -- or, for the
        causal kernel, whose mask is the row index, the whole sequence in one launch.  Returns {row: [d] fp64}."""
        case = self.case
        es = {n: self.t[n].element_size() for n in NAMES[:3]}
        base = {n: self.t[n].data_ptr() + (b * self.bs[n] + h * case.d) * es[n] for n in NAMES[:3]}
        got = {}
        whole = case.kernel == 'causal'
        for row in ([None] if whole else rows):
            sub = case._replace(batch=1, heads=1, sq=case.sq if whole else 1)
            buf, ldo, bso = A.out_buffer(sub)
            out = torch.from_numpy(buf).cuda()
            ptr = dict(base, out=out.data_ptr())
            if not whole:
                ptr['q'] += row * self.ld['q'] * es['q']
            f = A.fields(sub, ptr, dict(self.ld, out=ldo), dict(self.bs, out=bso), scale)
            f['variant'] = variant
            rc = _launch(case.kernel, f)
            torch.cuda.synchronize()
            assert rc == 0, (case.name, rc)
            o = A.unpack_out(sub, out.cpu().numpy())[0, :, 0]
            got.update({r: o[r] for r in rows} if whole else {row: o[0]})
        return got


def _pinned(case):
    """A variant under which the kernel does not depend on the launch's size."""
    return A.named_split(case) if case.kernel == 'f32' and case.d % 128 == 0 else case.variant


# --------------------------------------------------------------------------------------------------------------------------------
# the hardware exp2: the exact family's one assumption and the generic bounds' one measured constant

def _exp2_through_attention(x):
    """out = p / (1 + p), p = exp2(x), for fp32 x <= 0: ds_attention at d = 8, skv = 2, scale = fl32(ln 2) (the folded factor is exactly 1),
    q = (x, 0, ..), k = (0 | e0), v = (0 | e0): the scores are 0 and x exactly, the maximum is 0, O = p exactly."""
    n = x.size
    case = A.Case('exp2', 'f32', 8, 1, 1, n, 2, 0, 0, 0, 0)
    q, k, v = np.zeros((1, n, 1, 8)), np.zeros((1, 2, 1, 8)), np.zeros((1, 2, 1, 8))
    q[0, :, 0, 0], k[0, 1, 0, 0], v[0, 1, 0, 0] = x, 1.0, 1.0
    got = Dev(case, q, k, v).run(A.LN2_32)
    assert np.array_equal(got[0, :, 0, 1:], np.zeros((n, 7)))
    return got[0, :, 0, 0]


def test_exp2_is_exact_on_integer_arguments():
    """The assumption of the exact family: for integer x in [-126, 0] the kernel's output is fl(2^x fl(1 / fl(1 + 2^x))) bit for bit."""
    x = -np.arange(127, dtype=np.float32)
    got = _exp2_through_attention(x).astype(np.float32)
    p = np.exp2(x.astype(np.float64)).astype(np.float32)
    want = (p * (np.float32(1) / (np.float32(1) + p))).astype(np.float64)
    excess = np.abs(got.astype(np.float64) - want) / (A.U * want)
    print(f'\nexp2 on integers: largest deviation {float(excess.max()):.3f} U (recorded EXP2_INT_EXCESS {A.EXP2_INT_EXCESS})')
    assert (excess <= A.EXP2_INT_EXCESS).all(), (x[excess > A.EXP2_INT_EXCESS], excess.max())


def test_exp2_constant_holds_on_a_dense_sweep():
    """Re-measures EXP2_MEASURED over ~1 M points of [-126, 0] and holds the maximum below K_EXP2, twice the recorded measurement."""
    lo, hi, n = A.EXP2_SWEEP
    x = np.linspace(lo, hi, n).astype(np.float32)
    got = _exp2_through_attention(x)
    p = np.exp2(x.astype(np.float64))
    small = x <= -25                                       # fl(1 + p) = 1: the output is exp2(x) itself
    ref = np.where(small, p, p / (1.0 + p))
    rel = np.abs(got - ref) / ref
    meas = np.where(small, rel, np.maximum(rel - 3 * A.U * A.SECOND, 0.0) * (1.0 + p)) / A.U
    i = int(np.argmax(meas))
    print(f'\nMEASURED exp2 {float(meas.max()):.3f} U at x = {float(x[i])!r} ({float(meas[small].max()):.3f} U on x <= -25 alone; '
          f'recorded {A.EXP2_MEASURED})')
    assert meas.max() <= A.K_EXP2, (float(meas.max()), float(x[i]))


# --------------------------------------------------------------------------------------------------------------------------------
# the exact family

@functools.lru_cache(maxsize=None)
def _exact(name):
    case = A.CASE_BY_NAME[name]
    q, k, v = A.exact_inputs(case)
    return q, k, v, A.exact_ref(case, q, k, v)


@pytest.mark.parametrize('name', IDS)
def test_exact_family_to_two_ulps(name):
    case = A.CASE_BY_NAME[name]
    q, k, v, ref = _exact(name)
    bound = A.exact_bound(ref)
    dev = Dev(case, q, k, v)
    got = dev.run(A.exact_scale(case))
    assert A.inside(got, ref, bound, case.out16).all(), A.worst(got, ref, bound, case.out16)
    if case.kernel == 'f16' and case.d <= 64:          # one kernel serves the three variants
        for variant in (0, 1, 2):
            assert np.array_equal(dev.run(A.exact_scale(case), variant), got), variant
    if case.kernel == 'f32' and case.d % 128 == 0 and case.d < 512:          # both splits meet the bound whatever the case names
        for variant in (1, 2):
            g = dev.run(A.exact_scale(case), variant)
            assert A.inside(g, ref, bound).all(), (variant, A.worst(g, ref, bound))


# --------------------------------------------------------------------------------------------------------------------------------
# the generic family

def _refused(case, kind):
    return kind == 'negscale' and case.kernel == 'f16' and bool(case.in16 & 1)


@pytest.mark.parametrize('name', IDS)
def test_generic_family_inside_the_derived_bound(name):
    case = A.CASE_BY_NAME[name]
    for kind in A.GENERIC_KINDS:
        q, k, v, scale = A.generic_inputs(case, kind)
        dev = Dev(case, q, k, v)
        if _refused(case, kind):          # fp16 q with a negative scale: refused, nothing written
            buf, dev.ld['out'], dev.bs['out'] = A.out_buffer(case)
            out = torch.from_numpy(buf).cuda()
            f = A.fields(case, {n: dev.t[n].data_ptr() for n in NAMES[:3]} | {'out': out.data_ptr()}, dev.ld, dev.bs, scale)
            assert _launch('f16', f) == -1
            torch.cuda.synchronize()
            assert bool(torch.isnan(out).all())
            continue
        ref, bound = A.generic_ref(case, *A.as_operands(case, q, k, v), scale)
        got = dev.run(scale)
        if not case.out16:          # (an fp16 output is held to the rounded interval, not to the fp32 bound)
            print(f'{name} {kind}: at most {float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max()):.3f} of the bound')
        assert A.inside(got, ref, bound, case.out16).all(), (kind, A.worst(got, ref, bound, case.out16))


@pytest.mark.parametrize('name', IDS)
def test_what_must_not_be_read_has_no_effect(name):
    """The same bits whether the padding columns and the rows at and beyond sq / skv hold NaN or numbers of the order of 1e3 (1e3 times
    the operands' scale)."""
    case = A.CASE_BY_NAME[name]
    q, k, v, scale = A.generic_inputs(case, 'randn')
    a = Dev(case, q, k, v, fill='nan').run(scale)
    b = Dev(case, q, k, v, fill='junk').run(scale)
    assert np.array_equal(a, b), int((a != b).sum())


@pytest.mark.parametrize('name', IDS)
def test_shift_invariance(name):
    """softmax does not see a constant row added to every key of a head.  The keys and the row are multiples of 2^-8 below 7 in absolute
    value, so the shifted keys are exact in fp32 and in fp16: the shifted launch is held to the UNSHIFTED reference, with the bound of
    the operands it was given."""
    case = A.CASE_BY_NAME[name]
    q, k, v, scale = A.generic_inputs(case, 'randn')
    k = np.clip(np.round(k * 256.0) / 256.0, -6.0, 6.0)
    c = np.round(np.random.default_rng(5).uniform(-1, 1, size=(1, 1, case.heads, case.d)) * 256.0) / 256.0
    ops = A.as_operands(case, q, k, v)
    ref, bound = A.generic_ref(case, *ops, scale)
    got = Dev(case, q, k, v).run(scale)
    assert A.inside(got, ref, bound, case.out16).all(), A.worst(got, ref, bound, case.out16)
    ks = k + c
    assert np.array_equal(A.as_operands(case, q, ks, v)[1].astype(np.float64), ks)
    _, bound_s = A.generic_ref(case, *A.as_operands(case, q, ks, v), scale)
    got_s = Dev(case, q, ks, v).run(scale)
    assert A.inside(got_s, ref, bound_s, case.out16).all(), A.worst(got_s, ref, bound_s, case.out16)


@pytest.mark.parametrize('name', IDS)
def test_a_query_does_not_depend_on_its_launch(name):
    """With the variant pinned a query's output bits depend neither on batch, nor on the heads beside it, nor on sq: a query is one lane,
    nothing is reduced across queries.  Rows {0, 31, 32, sq - 1} of the first and the last (image, head), alone and inside the launch."""
    case = A.CASE_BY_NAME[name]
    q, k, v, scale = A.generic_inputs(case, 'randn')
    dev = Dev(case, q, k, v)
    variant = _pinned(case)
    full = dev.run(scale, variant)
    rows = sorted({r for r in (0, 31, 32, case.sq - 1) if r < case.sq})
    for b, h in {(0, 0), (case.batch - 1, case.heads - 1)}:
        alone = dev.run_rows(scale, b, h, rows, variant)
        for r in rows:
            assert np.array_equal(alone[r], full[b, r, h]), (b, h, r, int((alone[r] != full[b, r, h]).sum()))


# --------------------------------------------------------------------------------------------------------------------------------
# refusals

def test_refusals_launch_nothing():
    """Every entry of the refusal table with real device buffers: its code, and the output keeps its prefill."""
    for kernel in ('f32', 'f16', 'causal', 'm88'):
        case = A.CASE_BY_NAME[A.BASE[kernel]]
        q, k, v, _ = A.generic_inputs(case, 'randn')
        dev = Dev(case, q, k, v)
        out = torch.from_numpy(A.out_buffer(case)[0]).cuda()
        ptr = {n: dev.t[n].data_ptr() for n in NAMES[:3]} | {'out': out.data_ptr()}
        for entry in A.REFUSALS:
            if entry[1] != kernel:
                continue
            kern, f = A.refusal_fields(entry, ptr)
            assert _launch(kern, f) == entry[4], entry[0]
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), kernel
