"""tests/_attn_refs.py checked without a GPU: the references against ATen's fp64 softmax, every bound against the fp32 emulation of its
kernel's operation order, the exact family against its 2-ulp bound and against mutants of the emulation (it must bite), the coverage of
the case table against the traits table and the library's own support / routing queries, and the refusal table against the entry points
(argument checks answer on the host: nothing is launched)."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _attn_refs as A  # noqa: E402

IDS = [c.name for c in A.CASES]


def _libs():
    from diff_sampler_amd import _lib, _metrics_lib
    return _lib, _lib.load(), _metrics_lib, _metrics_lib.load()


@functools.lru_cache(maxsize=None)
def _exact(name):
    case = A.CASE_BY_NAME[name]
    q, k, v = A.exact_inputs(case)
    ref = A.exact_ref(case, q, k, v)
    return q, k, v, ref


def test_the_exact_scales_fold_to_powers_of_two():
    """fl32(fl32(ln 2) 2^-k) fl32(log2 e) rounds to exactly 2^-k in fp32: the factor every kernel folds into q (or the scores) is exact."""
    assert A.LN2_32 == np.float32(np.log(2.0)) and A.LN2_32.view(np.uint32) == 0x3f317218
    for k in A.EXACT_K:
        sc = np.float32(A.LN2_32 * np.float32(2.0 ** -k)) * A.LOG2E32
        assert sc.dtype == np.float32 and sc == np.float32(2.0 ** -k), k
    assert {c.k for c in A.CASES} == set(A.EXACT_K)


@pytest.mark.parametrize('name', IDS)
def test_exact_family_is_exact_and_its_emulation_meets_the_two_ulp_bound(name):
    case = A.CASE_BY_NAME[name]
    q, k, v, ref = _exact(name)
    assert case.skv <= 256 and np.abs(k).max() <= 2 and np.abs(v).max() <= 7 and ((q != 0).sum(-1) <= 3).all()
    # the reference agrees with ATen's fp64 softmax at the scale the kernels' factor stands for, ln 2 * 2^-k
    scale = float(np.log(2.0)) * 2.0 ** -case.k
    assert abs(float(A.exact_scale(case)) / scale - 1) < 2.0 ** -24
    s = torch.einsum('bqhd,bkhd->bhqk', torch.from_numpy(q), torch.from_numpy(k)) * scale
    if case.kernel == 'causal':
        s = s.masked_fill(torch.triu(torch.ones(case.sq, case.skv, dtype=torch.bool), 1), float('-inf'))
    aten = torch.einsum('bhqk,bkhd->bqhd', s.softmax(-1), torch.from_numpy(v)).numpy()
    assert np.abs(aten - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max())
    ops = A.as_operands(case, q, k, v)
    assert all(np.array_equal(o.astype(np.float64), x) for o, x in zip(ops, (q, k, v)))          # exact in fp16 too
    got = A.emulate_case(case, *ops, A.exact_scale(case))
    assert A.inside(got, ref, A.exact_bound(ref), case.out16).all(), A.worst(got, ref, A.exact_bound(ref), case.out16)


@pytest.mark.parametrize('mutant', A.MUTANTS)
def test_the_exact_family_bites_on_mutants_of_the_emulation(mutant):
    """Each deliberate bug leaves the exact bound on the case MUTANT_CASES names (and the unmutated emulation of that case is inside)."""
    name = A.MUTANT_CASES[mutant]
    case = A.CASE_BY_NAME[name]
    q, k, v, ref = _exact(name)
    ops = A.as_operands(case, q, k, v)
    bound = A.exact_bound(ref)
    assert A.inside(A.emulate_case(case, *ops, A.exact_scale(case)), ref, bound, case.out16).all()
    bad = A.emulate_case(case, *ops, A.exact_scale(case), mutant=mutant)
    out = int((~A.inside(bad, ref, bound, case.out16)).sum())
    print(f'{mutant} on {name}: {out} of {ref.size} elements outside')
    assert out > 0


@pytest.mark.parametrize('name', IDS)
def test_generic_reference_is_aten_softmax_and_the_emulation_lies_inside_the_bound(name):
    case = A.CASE_BY_NAME[name]
    worst_frac = 0.0
    for kind in A.GENERIC_KINDS:
        if kind == 'negscale' and case.kernel == 'f16' and case.in16 & 1:
            continue          # refused by the entry point (REFUSALS)
        q, k, v, scale = A.generic_inputs(case, kind)
        ops = A.as_operands(case, q, k, v)
        ref, bound = A.generic_ref(case, *ops, scale)
        if case.kernel != 'f16':          # (the f16 reference is of the rounded operands: compared through the emulation below)
            s = torch.einsum('bqhd,bkhd->bhqk', *(torch.from_numpy(o.astype(np.float64)) for o in ops[:2])) * scale
            if case.kernel == 'causal':
                s = s.masked_fill(torch.triu(torch.ones(case.sq, case.skv, dtype=torch.bool), 1), float('-inf'))
            aten = torch.einsum('bhqk,bkhd->bqhd', s.softmax(-1), torch.from_numpy(ops[2].astype(np.float64))).numpy()
            assert np.abs(aten - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), kind
        if kind == 'spike':          # every other weight underflows in fp64 too: the reference IS that key's v
            j = 0 if case.kernel == 'causal' else case.skv // 2
            want = np.broadcast_to(ops[2][:, j][:, None].astype(np.float64), ref.shape)
            want = A.rne16(want) if case.kernel == 'f16' else want
            assert np.array_equal(ref, want)
        got = A.emulate_case(case, *ops, scale)
        assert A.inside(got, ref, bound, case.out16).all(), (kind, A.worst(got, ref, bound, case.out16))
        if not case.out16:
            worst_frac = max(worst_frac, float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max()))
    print(f'{name}: emulation at most {worst_frac:.3f} of the bound')


def test_the_case_table_reaches_every_trait_and_edge():
    by = lambda kern: [c for c in A.CASES if c.kernel == kern]
    f32c, f16c = by('f32'), by('f16')
    # head sizes: the table's equal the library's support queries over 1 .. 1024
    _lib, lib, _m, mlib = _libs()
    assert {c.d for c in f32c} == set(A.F32_SIZES) == {d for d in range(1, 1025) if lib.ds_attention_supported(d)}
    assert {c.d for c in f16c} == set(A.F16_SIZES) == {d for d in range(1, 1025) if lib.ds_attention_f16_supported(d)}
    assert {c.d for c in by('causal')} == {64} == {d for d in range(1, 1025) if lib.ds_attention_causal_supported(d, 77)}
    assert {c.d for c in by('m88')} == {88} == {d for d in range(1, 1025) if mlib.dsm_attention_supported(d)}
    # ds_attention: every trait combination of the traits table, with the split actually taken and the prefetch that follows
    combos = lambda ds, split_of: {(t['kt'], t['vrem'], t['alias'], s, A.prefetch_f32(d, s)) for d in ds for t in [A.traits_f32(d)] for s in split_of(d)}
    every = combos(A.F32_SIZES, lambda d: (2,) if d >= 512 else ((1, 2) if d % 128 == 0 else (1,)))
    reached = {(t['kt'], t['vrem'], t['alias'], A.named_split(c), A.prefetch_f32(c.d, A.named_split(c))) for c in f32c for t in [A.traits_f32(c.d)]}
    assert reached == every and (32, False, False, 1, False) in every and (32, False, True, 2, True) in every and (64, False, False, 1, True) in every
    for d in (128, 256):
        assert {c.variant for c in f32c if c.d == d} == {0, 1, 2}
    assert [(c.sq, c.skv) for c in f32c if c.d == 512] == [(33, 65)]
    for kt in (32, 64):
        assert {c.skv for c in f32c if A.case_kt(c) == kt} == {1, kt - 1, kt, kt + 1, 2 * kt + 1}
    for d in A.F32_SIZES:
        assert A.traits_f32(d)['kt'] == (64 if d in (8, 16, 32, 64) else 32) and A.traits_f32(d)['vrem'] == (d == 40)
    assert {c.sq for c in f32c if A.named_split(c) == 1} == {1, 31, 32, 33, 127, 128, 129}
    assert {c.sq for c in f32c if A.named_split(c) == 2} == {1, 31, 32, 33, 65}
    # ds_attention_f16
    assert {(c.d, c.in16) for c in f16c if c.d in (40, 64)} == {(d, m) for d in (40, 64) for m in range(4)}
    for d in A.F16_SIZES:
        assert len({c.in16 for c in f16c if c.d == d}) >= 2 and {c.out16 for c in f16c if c.d == d} == {0, 1}
    assert {c.sq for c in f16c} == {1, 33, 255, 256, 257} and {c.skv for c in f16c} == {1, 63, 64, 65, 129}
    assert {c.batch * c.heads for c in f16c} >= {1, 7, 8, 9}
    key = lambda d: tuple(sorted(A.traits_f16(d).items()))
    assert {key(c.d) for c in f16c} == {key(d) for d in A.F16_SIZES}
    assert {d for d in A.F16_SIZES if A.traits_f16(d)['ones']} == {40, 80} and {d for d in A.F16_SIZES if A.traits_f16(d)['zero_pad']} == {40}
    assert any(A.traits_f16(c.d)['ones'] and c.in16 != 3 and c.skv % 64 for c in f16c)          # matrix-pipe denominator, not mode 3, ragged tile
    # the two younger kernels
    assert [c.sq for c in by('causal')] == [1, 31, 32, 33, 77, 128] and all(c.sq == c.skv for c in by('causal'))
    assert {c.sq for c in by('m88') if c.sq == c.skv} == {1, 31, 32, 33, 129} and any(c.sq != c.skv for c in by('m88'))
    assert all(1 <= c.batch <= 3 or c.kernel == 'f16' for c in A.CASES) and all(c.skv <= 256 for c in A.CASES)
    assert len(IDS) == len(set(IDS)) and set(A.MUTANT_CASES) == set(A.MUTANTS) and set(A.MUTANT_CASES.values()) <= set(IDS)


def test_the_library_takes_the_split_each_case_names():
    _lib, lib, _, _ = _libs()
    for case in A.CASES:
        if case.kernel != 'f32':
            continue
        _, ld, bs = A.out_buffer(case)
        f = A.fields(case, A.fake_ptrs(), dict.fromkeys('q k v out'.split(), ld), dict.fromkeys('q k v out'.split(), bs), 0.125)
        assert lib.ds_attention_variant(C.byref(_lib.AttnArgs(**f))) == A.named_split(case), case.name
    assert lib.ds_attention_variant(None) == -1


def _call(entry, ptr=None, stream=None):
    _lib, lib, _m, mlib = _libs()
    kernel, f = A.refusal_fields(entry, ptr)
    if kernel == 'm88':
        f = dict(f)
        res = (C.c_int * 3)(f.pop('out_f16'), f.pop('in_f16'), f.pop('variant'))
        return mlib.dsm_attention(C.byref(_m.DsmAttnArgs(reserved=res, **f)), stream)
    fn = {'f32': lib.ds_attention, 'f16': lib.ds_attention_f16, 'causal': lib.ds_attention_causal}[kernel]
    return fn(C.byref(_lib.AttnArgs(**f)), stream)


@pytest.mark.parametrize('entry', A.REFUSALS, ids=[e[0] for e in A.REFUSALS])
def test_refusals_return_their_codes_without_a_gpu(entry):
    assert _call(entry) == entry[4]


def test_null_argument_structs_are_refused():
    _lib, lib, _m, mlib = _libs()
    assert lib.ds_attention(None, None) == -1 and lib.ds_attention_f16(None, None) == -1
    assert lib.ds_attention_causal(None, None) == -1 and mlib.dsm_attention(None, None) == -1
    names = [e[0] for e in A.REFUSALS]
    assert len(names) == len(set(names))


def test_the_design_document_carries_the_measured_constants():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'DESIGN.md'), encoding='utf-8').read()
    assert f'{A.EXP2_MEASURED:.3f} U' in text and f'`K_EXP2` = {A.K_EXP2:.3f}' in text and '`EXP2_INT_EXCESS` = 0' in text
    assert A.K_EXP2 == 2 * A.EXP2_MEASURED and A.EXP2_INT_EXCESS == 0.0
