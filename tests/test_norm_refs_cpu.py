"""The references, bounds and case tables of tests/_norm_refs.py, checked without a GPU: the fp64 restatements against ATen in fp64, every
bound against an fp32 emulation of the kernel's operation order, and -- through ds_norm_route, the library's own routing -- that the
tables reach every kernel, resampling instantiation and loop they claim."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _norm_refs as R  # noqa: E402


def _route(fields):
    from diff_sampler_amd import build, _lib
    build.build_lib(verbose=False)
    lib = _lib.load()
    info = _lib.NormRouteInfo()
    assert lib.ds_norm_route(C.byref(_lib.NormArgs(**fields)), C.byref(info)) == 0
    return info


def _nchw(v):
    return torch.from_numpy(np.ascontiguousarray(v)).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).numpy()


def _aten_pass(case, d):
    x = _nchw(d['x'].astype(np.float64))
    n, c = x.shape[:2]
    if case.form in ('stats', 'full', 'ada', 'planes', 'fin'):
        x = F.group_norm(x, case.groups, None, None, float(np.float32(R.EPS)))
    if d['gamma'] is not None:
        x = x * torch.from_numpy(d['gamma']).double().reshape(1, c, 1, 1)
    if d['beta'] is not None:
        x = x + torch.from_numpy(d['beta']).double().reshape(1, c, 1, 1)
    if d['scale'] is not None:
        x = x * (1 + torch.from_numpy(d['scale']).double().reshape(n, c, 1, 1)) + torch.from_numpy(d['shift']).double().reshape(n, c, 1, 1)
    if case.act:
        x = F.silu(x)
    if case.resample == R.DOWN:
        x = F.avg_pool2d(x, 2)
    elif case.resample == R.UP:
        x = F.interpolate(x, scale_factor=2, mode='nearest')
    return _nhwc(x)


SMALL_PASS = [c for c in R.PASS_CASES if c.n * c.h * c.w * (c.c0 + c.c1) < (1 << 22)]


@pytest.mark.parametrize('case', SMALL_PASS, ids=lambda c: c.name)
def test_pass_reference_is_group_norm_silu_and_resampling_in_fp64(case):
    d = R.pass_inputs(case)
    y, b, raw, rawb, extra = R.pass_reference(case, d)
    ref = _aten_pass(case, d)
    assert y.shape == ref.shape and b.shape == y.shape and np.all(b >= 0) and np.all(np.isfinite(b))
    # 'fin' takes its statistics from block sums rounded to fp32: the same operation to 1e-6, not to fp64's 1e-12
    tol = 1e-5 if case.form == 'fin' else 1e-11
    assert np.abs(y - ref).max() <= tol * max(1.0, np.abs(ref).max())
    if case.raw:
        x = _nchw(d['x'].astype(np.float64))
        rr = F.avg_pool2d(x, 2) if case.resample == R.DOWN else (F.interpolate(x, scale_factor=2, mode='nearest') if case.resample == R.UP else x)
        assert np.array_equal(raw, _nhwc(rr)) or np.abs(raw - _nhwc(rr)).max() < 1e-14


@pytest.mark.parametrize('case', R.PASS_CASES, ids=lambda c: c.name)
def test_pass_bound_holds_for_an_fp32_emulation_of_the_kernel(case):
    d = R.pass_inputs(case)
    y, b, raw, rawb, extra = R.pass_reference(case, d)
    c = case.c0 + case.c1
    if case.form == 'identity':
        got = R.emulate_pass(d['x'], None, case.act, case.resample, identity=True, out16=case.out16)
    else:
        if case.form == 'planes':
            p32 = extra['planes32']
        else:
            n = case.n
            if case.form == 'fin':
                mean, rstd = R.gn_from_sums_ref(extra['stats'], n, case.h * case.w, case.groups)
            elif 'mean32' in extra:
                mean, rstd = extra['mean32'], extra['rstd32']
            else:
                mean, rstd = np.zeros((n, 1)), np.ones((n, 1))
            p32 = R.emulate_planes(mean, rstd, d['gamma'], d['beta'], d['scale'], d['shift'], c)
        got = R.emulate_pass(d['x'], p32, case.act, case.resample, out16=case.out16)
    ok = R.inside(got, y, b, case.out16)
    assert ok.all(), R.worst(got, y, b, case.out16)
    if case.raw:
        got = R.emulate_pass(d['x'], None, 0, case.resample, identity=True, out16=True)
        assert R.inside(got, raw, rawb, True).all(), R.worst(got, raw, rawb, True)
    # the reference itself satisfies every condition the GPU test sets, and a value two bounds away does not
    assert R.inside(y, y, b, False).all()
    far = y + 2.5 * np.maximum(b, np.abs(y) * 2.0 ** -10 if case.out16 else 0) + (1e-3 if case.out16 else 0)
    assert not R.inside(far, y, b, case.out16).any()


@pytest.mark.parametrize('case', R.STATS_CASES, ids=lambda c: c.name)
def test_statistics_reference_and_plane_bounds(case):
    d = R.stats_inputs(case)
    c = case.c0 + case.c1
    mean, rstd = R.gn_stats_ref(d['x'], case.groups)
    x = torch.from_numpy(d['x']).double().permute(0, 2, 1).reshape(case.n, c, case.h, case.w)
    xg = x.reshape(case.n, case.groups, -1)
    assert np.allclose(mean, xg.mean(-1).numpy(), rtol=1e-13, atol=0)
    assert np.allclose(rstd, 1 / np.sqrt(xg.var(-1, unbiased=False).numpy() + float(np.float32(R.EPS))), rtol=1e-12, atol=0)
    ex2 = (xg * xg).mean(-1).numpy()
    var = xg.var(-1, unbiased=False).numpy()
    live = var > 0
    assert (ex2[live] / var[live]).max() <= 1e4          # the domain the one-ulp statement is made for
    if case.const:
        assert var[0, 0] == 0 and rstd[0, 0] == 1 / np.sqrt(float(np.float32(R.EPS))) and mean[0, 0] == R.CONST_VALUE
    for rows in (1, case.n):
        sc, sh = d['scale'][:rows, :c], d['shift'][:rows, :c]
        planes, pb = R.planes_ref(mean, rstd, d['gamma'], d['beta'], sc, sh, c)
        ref = F.group_norm(x, case.groups, torch.from_numpy(d['gamma']).double(), torch.from_numpy(d['beta']).double(), float(np.float32(R.EPS)))
        ref = ref * (1 + torch.from_numpy(sc).double().reshape(rows, c, 1, 1)) + torch.from_numpy(sh).double().reshape(rows, c, 1, 1)
        mine = (x - torch.from_numpy(planes[:, 0]).reshape(case.n, c, 1, 1)) * torch.from_numpy(planes[:, 1]).reshape(case.n, c, 1, 1) + \
            torch.from_numpy(planes[:, 2]).reshape(case.n, c, 1, 1)
        assert float((mine - ref).abs().max()) <= 1e-9 * float(ref.abs().max())
        got = R.emulate_planes(mean, rstd, d['gamma'], d['beta'], sc, sh, c)
        assert R.inside(got, planes, pb).all(), R.worst(got, planes, pb)


@pytest.mark.parametrize('case', R.FINALIZE_CASES, ids=lambda c: c.name)
def test_statistics_from_block_sums_reference(case):
    d = R.finalize_inputs(case)
    c = case.c0 + case.c1
    nrb = case.hw // 64
    assert d['stats'].shape == (case.n * nrb, 2, c) and d['stats'].dtype == np.float32
    mean, rstd = R.gn_from_sums_ref(d['stats'], case.n, case.hw, case.groups)
    assert np.all(np.isfinite(mean)) and np.all(np.isfinite(rstd))
    # independent evaluation: python floats (fp64), channel by channel
    s = d['stats'].astype(np.float64).reshape(case.n, nrb, 2, c)
    cpg = c // case.groups
    for n_, g_ in ((0, 0), (case.n - 1, case.groups - 1)):
        S = sum(float(s[n_, rb, 0, ch]) for rb in range(nrb) for ch in range(g_ * cpg, (g_ + 1) * cpg))
        Q = sum(float(s[n_, rb, 1, ch]) for rb in range(nrb) for ch in range(g_ * cpg, (g_ + 1) * cpg))
        m = S / (cpg * case.hw)
        v = max(Q / (cpg * case.hw) - m * m, 0.0)
        assert abs(mean[n_, g_] - m) <= 1e-13 * abs(m) and abs(rstd[n_, g_] - (v + float(np.float32(R.EPS))) ** -0.5) <= 1e-9 * rstd[n_, g_]
    if case.neg:
        assert np.all(rstd[0] == 1 / np.sqrt(float(np.float32(R.EPS)))) and np.all(rstd[1] < 2)
    gpb = R.finalize_gpb(case.n, case.groups)
    assert 1 <= gpb <= case.groups


def test_finalize_cases_cover_what_they_name():
    by = {c.name: c for c in R.FINALIZE_CASES}
    assert {c.hw // 64 for c in R.FINALIZE_CASES} >= {1, 2, 3, 5, 16, 17}
    assert [R.finalize_gpb(by[k].n, 32) for k in ('gpb1_n2', 'gpb2_n17', 'gpb3_n33')] == [1, 2, 3]
    assert 32 % 3 != 0                                                                  # gpb 3: the last workgroup holds 2 groups
    c = by['c512_per_block']
    assert (c.c0 // c.groups) * R.finalize_gpb(c.n, c.groups) == 512                      # > 256: the coefficient loop's second trip
    for k in ('group_across_sources', 'gpb3_across_sources'):
        c = by[k]
        cpg = (c.c0 + c.c1) // c.groups
        assert c.c0 % cpg != 0                                                          # a group holds channels of both sources
    assert {c.hw // 64 % 4 for c in R.FINALIZE_CASES} == {0, 1, 2, 3}                   # row blocks not a multiple of the 4 row-block lanes
    assert {c.null for c in R.FINALIZE_CASES} == {None, 'gamma', 'beta', 'scale', 'coefs'}


@pytest.mark.parametrize('f16in', [False, True])
def test_layernorm_reference_and_bound(f16in):
    for cols in R.LN_COLS:
        for rows in R.ln_rows(cols) + (40,):
            x, g, b = R.ln_inputs(rows, cols, f16in)
            y, bound = R.layernorm_ref(x, g, b)
            ref = F.layer_norm(torch.from_numpy(x).double(), (cols,), torch.from_numpy(g).double(), torch.from_numpy(b).double(),
                               float(np.float32(R.EPS))).numpy()
            assert np.abs(y - ref).max() <= 1e-9 * np.abs(ref).max()
            got = R.emulate_layernorm(x, g, b)
            assert np.all(np.isfinite(got))
            assert R.inside(got, y, bound).all(), (cols, rows, R.worst(got, y, bound))
            assert R.inside(got.astype(np.float16), y, bound, True).all()
            assert np.array_equal(y[rows // 2], np.broadcast_to(b.astype(np.float64), (cols,)))      # the constant row: exactly beta
    assert [R.layernorm_lanes(c) for c in R.LN_COLS] == [16, 16, 16, 16, 32, 32, 32, 64, 64, 64]
    assert (R.LN_SECOND_TRIP[0] - 1) // (256 // R.layernorm_lanes(R.LN_SECOND_TRIP[1])) >= 4096


def test_geglu_reference_and_bound():
    for inner in R.GEGLU_INNER:
        for rows in (1, 5):
            x = R.geglu_inputs(rows, inner, 2 * inner + 4)
            y, bound = R.geglu_ref(x, inner)
            xt = torch.from_numpy(x).double()
            ref = (xt[:, :inner] * F.gelu(xt[:, inner:2 * inner])).numpy()
            assert np.abs(y - ref).max() <= 1e-14 * max(1.0, np.abs(ref).max())
            got = R.emulate_geglu(x, inner)
            assert R.inside(got, y, bound).all(), R.worst(got, y, bound)
    x = R.geglu_inputs(5, 4, 12)
    assert {float(np.float32(v)) for v in R.GEGLU_GATES} <= set(x[:, 4:8].reshape(-1).tolist())
    rows, inner = R.GEGLU_SECOND_TRIP
    assert rows * (inner // 4) > 16384 * 256


def test_noise_embedding_reference_and_bound():
    for swap in (0, 1, 2, 3):
        for bs, nch, _ in R.NOISE_SHAPES:
            sigma, freqs = R.noise_inputs(bs, nch, swap)
            y, bound = R.noise_embed_ref(sigma, freqs, swap)
            s, f = torch.from_numpy(sigma).double(), torch.from_numpy(freqs).double()
            ang = (s if swap & 2 else s.log() / 4)[:, None] * f[None]
            ref = torch.cat([ang.sin(), ang.cos()] if swap & 1 else [ang.cos(), ang.sin()], 1).numpy()
            assert np.abs(y - ref).max() <= 1e-12
            got = R.emulate_noise_embed(sigma, freqs, swap)
            assert R.inside(got, y, bound).all(), R.worst(got, y, bound)
            assert (bs * nch // 2) % 256 != 0
    assert not (sigma.min() < 0) and any(bs * nch // 2 > 256 for bs, nch, _ in R.NOISE_SHAPES)


def test_fp16_interval_check_is_no_looser_than_one_rounding():
    ref = np.array([1.0, 1.0 + 2.0 ** -11, 1000.3, -3.1e-6])
    b = np.abs(ref) * R.U
    assert R.inside(R.rne16(ref), ref, b, True).all()
    up = np.nextafter(R.rne16(ref).astype(np.float16), np.float16(np.inf)).astype(np.float64)
    dn = np.nextafter(R.rne16(ref).astype(np.float16), np.float16(-np.inf)).astype(np.float64)
    ok_up, ok_dn = R.inside(up, ref, b, True), R.inside(dn, ref, b, True)
    assert not (ok_up & ok_dn).any()                                    # never both neighbours
    assert not ok_up[0] and not ok_dn[0]                                # an exactly representable reference admits only itself
    assert not R.inside(np.array([np.nan]), ref[:1], b[:1], True).any() and not R.inside(np.array([np.nan]), ref[:1], b[:1]).any()


# --------------------------------------------------------------------------------------------------------------------------------
# coverage, by the library's own routing

def test_pass_cases_take_the_kernels_and_loops_they_name():
    seen, loops = set(), {}
    for case in R.PASS_CASES:
        ptr = R.fake_ptrs()
        if case.mis == 'gamma':
            ptr['gamma'] += 4
        info = _route(R.pass_fields(case, ptr))
        assert info.act_rc == 0, case.name
        assert (info.kernel, info.resampling) == (case.kernel, int(case.resample != R.NONE)), (case.name, info.kernel, info.resampling)
        oh, ow = R.out_hw(case)
        assert info.chunk % info.lanes == 0 and (info.chunks - 1) * info.chunk < oh * ow <= info.chunks * info.chunk, case.name
        octets = (case.c0 + case.c1) // (8 if case.kernel else 4)
        assert info.threads >= octets * info.lanes and info.threads % 64 == 0 and info.lanes <= oh * ow
        found = R.pass_loops(case, info.lanes, info.chunk, info.chunks)
        assert set(case.loops) <= found, (case.name, sorted(found), info.lanes, info.chunk, info.chunks)
        seen.add((info.kernel, info.resampling))
        loops.setdefault(info.kernel, set()).update(found)
    # every kernel id x resampling instantiation (the self-finalising form does not resample)
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (3, 0), (3, 1)}
    assert loops[0] >= {'four', 'tail', 'four+tail', 'ragged'}
    for k in (1, 3):
        assert loops[k] >= {'four', 'tail', 'four+tail', 'ragged', 'down2', 'down1', 'down2+down1'}, (k, loops[k])
    assert loops[2] >= {'four', 'tail'}
    by = {c.name: c for c in R.PASS_CASES}
    # the fp32 case is the only fp32 one above 16 MB; idle threads where the names say so
    big = [c.name for c in R.PASS_CASES if not c.out16 and c.n * c.h * c.w * (c.c0 + c.c1) * 4 > (16 << 20)]
    assert big == ['k0_f32_four_then_tail']
    info = _route(R.pass_fields(by['k1_c2056_idle_threads'], R.fake_ptrs()))
    assert (info.threads, info.lanes) == (512, 1)
    # tune_variant 1 sends every twin to the 8-byte kernel
    for name in R.TUNE1_TWINS:
        f = R.pass_fields(by[name], R.fake_ptrs())
        f['tune_variant'] = 1
        info = _route(f)
        assert (info.act_rc, info.kernel) == (0, 0), name


def test_stats_cases_take_the_geometry_they_name():
    for case in R.STATS_CASES:
        info = _route(R.stats_fields(case, R.fake_ptrs()))
        assert info.stats_rc == 0, case.name
        assert info.stats_chunks == case.P, (case.name, info.stats_chunks)
        assert case.h != case.w or case.h * case.w == 1
    by = {c.name: c for c in R.STATS_CASES}
    i = _route(R.stats_fields(by['cpg125_idle_threads'], R.fake_ptrs()))
    assert (i.stats_threads, i.stats_lanes) == (1024, 4)                  # 250 quads x 4 lanes = 1000 live threads
    i = _route(R.stats_fields(by['c4096_one_lane'], R.fake_ptrs()))
    assert (i.stats_threads, i.stats_lanes) == (1024, 1)
    i = _route(R.stats_fields(by['split_ragged'], R.fake_ptrs()))
    assert (by['split_ragged'].h * by['split_ragged'].w) % (i.stats_lanes * i.stats_chunks) != 0
    assert {(c.c0 + c.c1) // c.groups for c in R.STATS_CASES} >= {1, 2, 3, 5, 125}
    c = by['two_sources']
    assert c.c0 % ((c.c0 + c.c1) // c.groups) != 0 and c.ld0 > c.c0
    assert {c.in16 for c in R.STATS_CASES} == {0, 1, 2, 3}


def test_refusals_are_refused_by_the_routing():
    for entry in R.REFUSALS:
        info = _route(R.refusal_fields(entry, R.fake_ptrs()))
        if entry[4] is not None:
            assert info.act_rc == entry[4], (entry[0], info.act_rc)
        if entry[5] is not None:
            assert info.stats_rc == entry[5], (entry[0], info.stats_rc)
    from diff_sampler_amd import _lib
    assert _lib.load().ds_norm_route(None, None) == -1
