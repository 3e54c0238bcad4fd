"""The normalisation family of csrc/norm_act.hip (GroupNorm statistics, ds_gn_finalize, both pass kernels in every instantiation), LayerNorm
rows, GEGLU and the noise embedding off the networks' own geometry: every element against the fp64 references of tests/_norm_refs.py with
the bounds derived there.  Outputs are NaN-prefilled with padding columns and 64 guard rows that must still hold NaN afterwards; the
padding columns of the sources hold NaN, so a read past a source poisons the result.  Which kernel and loop a case runs is asked of the
library (ds_norm_route); tests/test_norm_refs_cpu.py proves the tables' coverage with the same query."""
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
import _norm_refs as R  # noqa: E402

pytestmark = pytest.mark.gpu

NAN = float('nan')
GUARD = 64
SLACK = 8          # elements in front of / behind every allocation's view: room for the misaligned views


def _lib():
    from diff_sampler_amd import _lib as L
    return L, L.load()


def _place(flat, off_bytes=0):
    """A CPU tensor's values in a device view that starts off_bytes into a NaN-filled allocation."""
    flat = flat.reshape(-1)
    k = off_bytes // flat.element_size()
    big = torch.full((flat.numel() + SLACK,), NAN, dtype=flat.dtype, device='cuda')
    view = big[k:k + flat.numel()]
    view.copy_(flat)
    return view


def _src(vals, ld, half, off=0):
    """[rows, c] values as rows of ld elements, the padding columns NaN."""
    vals = np.ascontiguousarray(vals)
    rows, c = vals.shape
    if ld == c:
        t = torch.from_numpy(vals).float()
    else:
        t = torch.full((rows, ld), NAN, dtype=torch.float32)
        t[:, :c] = torch.from_numpy(vals)
    return _place(t.half() if half else t, off)


def _vec(v, off=0):
    return None if v is None else _place(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)), off)


def _out(rows, ld, dtype=torch.float32, off=0):
    """NaN-prefilled output of `rows` rows of ld elements with GUARD rows behind."""
    return _place(torch.full(((rows + GUARD) * ld,), NAN, dtype=dtype), off)


def _check_out(view, rows, ld, c, what):
    """The output's live block [rows, c] as fp64 numpy; padding columns and guard rows must still hold NaN."""
    t = view.cpu().reshape(rows + GUARD, ld)
    assert bool(torch.isnan(t[rows:]).all()), f'{what}: a guard row was written'
    assert ld == c or bool(torch.isnan(t[:rows, c:]).all()), f'{what}: a padding column was written'
    return t[:rows, :c].double().numpy()


def _untouched(view):
    return bool(torch.isnan(view).all())


def _ptr(t):
    return None if t is None else t.data_ptr()


def _route(L, lib, a):
    info = L.NormRouteInfo()
    assert lib.ds_norm_route(C.byref(a), C.byref(info)) == 0
    return info


# --------------------------------------------------------------------------------------------------------------------------------
# device functions: the measured constants

def test_device_function_constants_hold_on_a_dense_sweep():
    """Re-measures what _norm_refs.py records (SILU_MEASURED, ERF_MEASURED, TRIG_MEASURED, LOG_MEASURED; printed with -s) on ~1 M points each
    and holds every maximum below the constant the bounds use, twice the recorded measurement."""
    L, lib = _lib()
    st = L.stream_ptr()
    npts = 1 << 20
    t = np.linspace(-100.0, 100.0, npts).astype(np.float32)
    # ds_silu: the pass in identity + SiLU form, fp32 -> fp32, one image of 2^18 pixels x 4 channels
    x, out = _place(torch.from_numpy(t)), _out(npts // 4, 4)
    a = L.NormArgs(x0=_ptr(x), c0=4, ld0=4, n=1, h=1, w=npts // 4, act=L.DS_ACT_SILU, out=_ptr(out), out_ld=4)
    assert lib.ds_norm_act(C.byref(a), st) == 0
    got = _check_out(out, npts // 4, 4, 4, 'silu').reshape(-1)
    ref = R.silu64(t.astype(np.float64))
    scale = R.U * np.maximum(np.abs(ref), 1e-300)
    m_silu = float((np.maximum(np.abs(got - ref) - R.SILU_ABS - R.silu_exp_term(t) * scale, 0) / scale).max())
    raw = np.maximum(np.abs(got - ref) - R.SILU_ABS, 0) / scale
    print(f'\nsilu without the derived exponent term: {float(raw.max()):.3f} U overall, {float(raw[t >= -10].max()):.3f} U on t >= -10')
    # erff: ds_geglu with a = 1
    rows, inner = 1024, 1024
    xg = torch.ones(rows, 2 * inner)
    xg[:, inner:] = torch.from_numpy(t).reshape(rows, inner)
    xd, yd = _place(xg), _out(rows, inner)
    assert lib.ds_geglu(_ptr(xd), 2 * inner, _ptr(yd), inner, rows, inner, st) == 0
    got = _check_out(yd, rows, inner, inner, 'geglu')
    g = t.astype(np.float64).reshape(rows, inner)
    ref = 0.5 * g * (1.0 + torch.erf(torch.from_numpy(g) * 0.5 ** 0.5).numpy())
    live = g != 0
    m_erf = float((np.maximum(np.abs(got - ref) - 3 * R.U * np.abs(ref), 0)[live] / (R.U * np.abs(0.5 * g[live]))).max())
    # cosf / sinf: the argument given directly, frequency 1
    arg = np.linspace(-1000.0, 1000.0, npts).astype(np.float32)
    sg, fr, emb = _place(torch.from_numpy(arg)), _place(torch.ones(1)), _out(npts, 2)
    assert lib.ds_noise_embed(_ptr(sg), npts, _ptr(fr), 2, 2, _ptr(emb), 2, st) == 0
    got = _check_out(emb, npts, 2, 2, 'noise_embed')
    ref = np.stack([np.cos(arg.astype(np.float64)), np.sin(arg.astype(np.float64))], 1)
    m_trig = float((np.abs(got - ref) / (R.U * np.maximum(np.abs(ref), 1e-300))).max())
    # logf: sigma log-uniform, frequency 2^-20 (exact product; sin(a) = a to 4e-13 for |a| < 1.6e-6)
    sig = np.exp(np.linspace(np.log(0.002), np.log(80.0), npts)).astype(np.float32)
    sg, fr, emb = _place(torch.from_numpy(sig)), _place(torch.full((1,), 2.0 ** -20)), _out(npts, 2)
    assert lib.ds_noise_embed(_ptr(sg), npts, _ptr(fr), 2, 0, _ptr(emb), 2, st) == 0
    got = _check_out(emb, npts, 2, 2, 'noise_embed')[:, 1]
    ref = np.log(sig.astype(np.float64)) / 4.0 * 2.0 ** -20
    live = ref != 0
    m_log = float((np.abs(got - ref)[live] / (R.U * np.abs(ref[live]))).max())
    print(f'\nMEASURED silu {m_silu:.3f} erf {m_erf:.3f} trig {m_trig:.3f} log {m_log:.3f} (units of U)')
    assert m_silu <= R.K_SILU and m_erf <= R.K_ERF and m_trig <= R.K_TRIG and m_log <= R.K_LOG, (m_silu, m_erf, m_trig, m_log)


# --------------------------------------------------------------------------------------------------------------------------------
# ds_gn_stats

def _stats_operands(case, d, ss_rows):
    c = case.c0 + case.c1
    x = d['x'].reshape(-1, c)
    t = dict(x0=_src(x[:, :case.c0], case.ld0, case.in16 & 1), x1=_src(x[:, case.c0:], case.ld1, case.in16 & 2) if case.c1 else None,
             mean=_out(case.n, case.groups), rstd=_out(case.n, case.groups), coefs=_out(case.n * 3, c),
             gamma=_vec(d['gamma']), beta=_vec(d['beta']), scale=_vec(d['scale'][:ss_rows]), shift=_vec(d['shift'][:ss_rows]),
             partial=torch.full((case.n * 32 * 128,), NAN, dtype=torch.float64, device='cuda') if case.partial else None)
    return t


@pytest.mark.parametrize('case', R.STATS_CASES, ids=lambda c: c.name)
def test_gn_stats_mean_rstd_and_planes(case):
    L, lib = _lib()
    d = R.stats_inputs(case)
    c = case.c0 + case.c1
    mean, rstd = R.gn_stats_ref(d['x'], case.groups)
    for ss_rows in (1, case.n):
        t = _stats_operands(case, d, ss_rows)
        a = L.NormArgs(**R.stats_fields(case, {k: _ptr(v) for k, v in t.items()}, ss_rows))
        info = _route(L, lib, a)
        assert (info.stats_rc, info.stats_chunks) == (0, case.P)
        assert lib.ds_gn_stats(C.byref(a), L.stream_ptr()) == 0
        torch.cuda.synchronize()
        gm = _check_out(t['mean'], case.n, case.groups, case.groups, 'mean').astype(np.float32)
        gr = _check_out(t['rstd'], case.n, case.groups, case.groups, 'rstd').astype(np.float32)
        assert R.within_ulps32(gm, mean).all(), (gm, mean)
        assert R.within_ulps32(gr, rstd).all(), (gr, rstd)
        planes, pb = R.planes_ref(mean, rstd, d['gamma'], d['beta'], d['scale'][:ss_rows, :c], d['shift'][:ss_rows, :c], c)
        got = _check_out(t['coefs'], case.n * 3, c, c, 'planes').reshape(case.n, 3, c)
        assert R.inside(got, planes, pb).all(), R.worst(got, planes, pb)
        assert np.array_equal(got[:, 0].astype(np.float32), np.repeat(gm, c // case.groups, axis=1))          # mu IS the stored mean
    if case.const:
        # a group of constant channels: rstd = 1 / sqrt(eps), never NaN, and the pass returns exactly B there (x - mu = 0)
        assert gm[0, 0] == np.float32(R.CONST_VALUE) and np.isfinite(gr[0, 0])
        assert R.within_ulps32(gr[0, :1], np.array([1 / np.sqrt(float(np.float32(R.EPS)))])).all()
        rows = case.n * case.h * case.w
        out = _out(rows, c)
        f = R.stats_fields(case, {k: _ptr(v) for k, v in t.items()}, 1)
        f.update(scale=None, shift=None, coefs=None, partial=None, out=_ptr(out), out_ld=c, act=0)
        assert lib.ds_norm_act(C.byref(L.NormArgs(**f)), L.stream_ptr()) == 0
        got = _check_out(out, rows, c, c, 'pass on a constant group')
        cpg = c // case.groups
        assert np.array_equal(got[:case.h * case.w, :cpg], np.broadcast_to(d['beta'][:cpg].astype(np.float64), (case.h * case.w, cpg)))


# --------------------------------------------------------------------------------------------------------------------------------
# ds_gn_finalize

@pytest.mark.parametrize('case', R.FINALIZE_CASES, ids=lambda c: c.name)
def test_gn_finalize_from_block_sums(case):
    L, lib = _lib()
    d = R.finalize_inputs(case)
    c = case.c0 + case.c1
    s0 = _place(torch.from_numpy(np.ascontiguousarray(d['stats'][:, :, :case.c0])))
    s1 = _place(torch.from_numpy(np.ascontiguousarray(d['stats'][:, :, case.c0:]))) if case.c1 else None
    for ss_rows in (1, case.n):
        ops = dict(gamma=d['gamma'], beta=d['beta'], scale=d['scale'][:ss_rows], shift=d['shift'][:ss_rows])
        if case.null in ('gamma', 'beta'):
            ops[case.null] = None
        if case.null == 'scale':
            ops['scale'] = ops['shift'] = None
        t = {k: _vec(v) for k, v in ops.items()}
        mean_o, rstd_o = _out(case.n, case.groups), _out(case.n, case.groups)
        coefs = None if case.null == 'coefs' else _out(case.n * 3, c)
        f = L.GnFinalizeArgs(_ptr(s0), _ptr(s1), case.c0, case.c1, case.n, case.hw, case.groups, R.EPS, _ptr(t['gamma']), _ptr(t['beta']),
                             _ptr(t['scale']), _ptr(t['shift']), 2 * c, ss_rows, _ptr(mean_o), _ptr(rstd_o), _ptr(coefs))
        assert lib.ds_gn_finalize(C.byref(f), L.stream_ptr()) == 0
        torch.cuda.synchronize()
        mean, rstd = R.gn_from_sums_ref(d['stats'], case.n, case.hw, case.groups)
        gm = _check_out(mean_o, case.n, case.groups, case.groups, 'mean').astype(np.float32)
        gr = _check_out(rstd_o, case.n, case.groups, case.groups, 'rstd').astype(np.float32)
        assert R.within_ulps32(gm, mean).all() and R.within_ulps32(gr, rstd).all(), (gm, mean, gr, rstd)
        if case.neg:
            assert np.isfinite(gr).all() and R.within_ulps32(gr[0], np.full(case.groups, 1 / np.sqrt(float(np.float32(R.EPS))))).all()
        if coefs is not None:
            planes, pb = R.planes_ref(mean, rstd, ops['gamma'], ops['beta'], None if ops['scale'] is None else ops['scale'][:, :c],
                                      None if ops['shift'] is None else ops['shift'][:, :c], c)
            got = _check_out(coefs, case.n * 3, c, c, 'planes').reshape(case.n, 3, c)
            assert R.inside(got, planes, pb).all(), R.worst(got, planes, pb)


# --------------------------------------------------------------------------------------------------------------------------------
# ds_norm_act

@functools.lru_cache(maxsize=2)
def _pass_reference(name):
    case = R.pass_case(name)
    d = R.pass_inputs(case)
    return d, R.pass_reference(case, d)


BIG = 1 << 25          # elements above which the reference is taken slab by slab (forms without statistics only)


def _launch_pass(case, d, extra, tune=None, offs=None):
    """Builds the operands of a case, launches ds_norm_act and returns (route info, out view, raw view)."""
    L, lib = _lib()
    offs = offs or {}
    c = case.c0 + case.c1
    x = d['x'].reshape(-1, c)
    oh, ow = R.out_hw(case)
    rows = case.n * oh * ow
    ld = c + case.out_pad
    dt = torch.float16 if case.out16 else torch.float32
    t = dict(x0=_src(x[:, :case.c0], case.ld0, case.in16 & 1, offs.get('x0', 0)),
             x1=_src(x[:, case.c0:], case.ld1, case.in16 & 2, offs.get('x1', 0)) if case.c1 else None,
             gamma=_vec(d['gamma'], 4 if case.mis == 'gamma' else offs.get('gamma', 0)), beta=_vec(d['beta']),
             scale=_vec(d['scale']), shift=_vec(d['shift'], offs.get('shift', 0)),
             mean=_vec(extra.get('mean32')), rstd=_vec(extra.get('rstd32')), coefs=_vec(extra.get('planes32')),
             out=_out(rows, ld, dt, offs.get('out', 0)), raw_out=_out(rows, ld, torch.float16) if case.raw else None)
    if 'stats' in extra:
        t['stats0'] = _place(torch.from_numpy(np.ascontiguousarray(extra['stats'][:, :, :case.c0])))
        t['stats1'] = _place(torch.from_numpy(np.ascontiguousarray(extra['stats'][:, :, case.c0:]))) if case.c1 else None
    ptr = {k: _ptr(v) for k, v in t.items()}
    for k in ('mean', 'rstd', 'coefs', 'stats0', 'stats1', 'partial'):
        ptr.setdefault(k, None)
    f = R.pass_fields(case, ptr)
    if tune is not None:
        f['tune_variant'] = tune
    a = L.NormArgs(**f)
    info = _route(L, lib, a)
    rc = lib.ds_norm_act(C.byref(a), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == info.act_rc
    return info, t, rc


@pytest.mark.parametrize('case', R.PASS_CASES, ids=lambda c: c.name)
def test_norm_act_every_element(case):
    c = case.c0 + case.c1
    oh, ow = R.out_hw(case)
    rows, ld = case.n * oh * ow, c + case.out_pad
    big = case.n * case.h * case.w * c > BIG
    if big:
        assert case.form in ('identity', 'beta', 'gb') and not case.raw
        d, extra = R.pass_inputs(case), {}
    else:
        d, (y, b, raw, rawb, extra) = _pass_reference(case.name)
    info, t, rc = _launch_pass(case, d, extra)
    assert rc == 0 and (info.kernel, info.resampling) == (case.kernel, int(case.resample != R.NONE))
    assert set(case.loops) <= R.pass_loops(case, info.lanes, info.chunk, info.chunks)
    got = _check_out(t['out'], rows, ld, c, 'out').reshape(case.n, oh, ow, c)
    if big:
        step = max(1, BIG // (4 * case.h * case.w * c))
        for i in range(0, case.n, step):
            sub = case._replace(n=min(step, case.n - i))
            y, b, _, _, _ = R.pass_reference(sub, dict(d, x=d['x'][i:i + step]))
            ok = R.inside(got[i:i + step], y, b, case.out16)
            assert ok.all(), (i, R.worst(got[i:i + step], y, b, case.out16))
    else:
        assert R.inside(got, y, b, case.out16).all(), R.worst(got, y, b, case.out16)
        if case.raw:
            got = _check_out(t['raw_out'], rows, ld, c, 'raw_out').reshape(case.n, oh, ow, c)
            assert R.inside(got, raw, rawb, True).all(), R.worst(got, raw, rawb, True)


@pytest.mark.parametrize('name', R.TUNE1_TWINS)
def test_norm_act_16_byte_and_8_byte_kernels_write_equal_bits(name):
    case = R.pass_case(name)
    d, (y, b, raw, rawb, extra) = _pass_reference(name)
    i16, t16, rc16 = _launch_pass(case, d, extra)
    i8, t8, rc8 = _launch_pass(case, d, extra, tune=1)
    assert (rc16, rc8) == (0, 0) and i16.kernel == case.kernel and i8.kernel == 0
    assert torch.equal(t16['out'].view(torch.int16), t8['out'].view(torch.int16))
    if case.raw:
        assert torch.equal(t16['raw_out'].view(torch.int16), t8['raw_out'].view(torch.int16))


@pytest.mark.parametrize('entry', R.REFUSALS, ids=lambda e: e[0])
def test_norm_refusals_launch_nothing(entry):
    L, lib = _lib()
    name, base, changes, offs, act_rc, stats_rc = entry
    case = R.pass_case(base)
    d, (y, b, raw, rawb, extra) = _pass_reference(base)
    c = case.c0 + case.c1
    x = d['x'].reshape(-1, c)
    oh, ow = R.out_hw(case)
    rows, ld = case.n * oh * ow, c + case.out_pad
    mean, rstd = R.gn_stats_ref(d['x'].reshape(case.n, -1, c), 1)
    t = dict(x0=_src(x[:, :case.c0], case.ld0, case.in16 & 1, offs.get('x0', 0)),
             x1=_src(x[:, case.c0:], case.ld1, case.in16 & 2, offs.get('x1', 0)) if case.c1 else None,
             gamma=_vec(d['gamma'], offs.get('gamma', 0)), beta=_vec(d['beta']), scale=_vec(d['scale']), shift=_vec(d['shift'], offs.get('shift', 0)),
             mean=_vec(np.repeat(mean, 64, 1)), rstd=_vec(np.repeat(rstd, 64, 1)), coefs=_vec(extra.get('planes32')),
             out=_out(rows, ld, torch.float16 if case.out16 else torch.float32, offs.get('out', 0)),
             raw_out=_out(rows, ld, torch.float16) if case.raw else None, partial=None)
    if 'stats' in extra:
        t['stats0'] = _place(torch.from_numpy(np.ascontiguousarray(extra['stats'][:, :, :case.c0])))
        t['stats1'] = _place(torch.from_numpy(np.ascontiguousarray(extra['stats'][:, :, case.c0:]))) if case.c1 else None
    ptr = {k: _ptr(v) for k, v in t.items()}
    for k in ('stats0', 'stats1'):
        ptr.setdefault(k, None)
    f = R.pass_fields(case, ptr)
    f.setdefault('mean', ptr['mean'])
    f.setdefault('rstd', ptr['rstd'])
    f.update(changes)
    a = L.NormArgs(**f)
    info = _route(L, lib, a)
    if act_rc is not None:
        assert info.act_rc == act_rc and lib.ds_norm_act(C.byref(a), L.stream_ptr()) == act_rc
        torch.cuda.synchronize()
        assert _untouched(t['out']) and (t['raw_out'] is None or _untouched(t['raw_out']))
    if stats_rc is not None:
        mo, ro, co = _out(case.n, 64), _out(case.n, 64), _out(case.n * 3, c)
        f.update(mean=_ptr(mo), rstd=_ptr(ro), coefs=_ptr(co), out=None, raw_out=None, stats0=None, stats1=None)
        a = L.NormArgs(**f)
        assert _route(L, lib, a).stats_rc == stats_rc and lib.ds_gn_stats(C.byref(a), L.stream_ptr()) == stats_rc
        torch.cuda.synchronize()
        assert _untouched(mo) and _untouched(ro) and _untouched(co)


# --------------------------------------------------------------------------------------------------------------------------------
# LayerNorm rows, GEGLU, noise embedding

def _layernorm(entry, rows, cols, ldx, ldy):
    L, lib = _lib()
    f16in, f16out = entry == 'f16io', entry != 'f32'
    x, g, b = R.ln_inputs(rows, cols, f16in, const_row=rows < 1000)
    xd, gd, bd = _src(x, ldx, f16in), _vec(g), _vec(b)
    yd = _out(rows, ldy, torch.float16 if f16out else torch.float32)
    fn = {'f32': lib.ds_layernorm_rows, 'f16out': lib.ds_layernorm_rows_f16, 'f16io': lib.ds_layernorm_rows_f16io}[entry]
    assert fn(_ptr(xd), ldx, _ptr(gd), _ptr(bd), R.EPS, _ptr(yd), ldy, rows, cols, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    got = _check_out(yd, rows, ldy, cols, 'layernorm')
    y, bound = R.layernorm_ref(x, g, b)
    assert np.isfinite(got).all()
    assert R.inside(got, y, bound, f16out).all(), (entry, rows, cols, R.worst(got, y, bound, f16out))


@pytest.mark.parametrize('entry', R.LN_ENTRIES)
def test_layernorm_rows_every_element(entry):
    for cols in R.LN_COLS:
        for rows in R.ln_rows(cols):
            _layernorm(entry, rows, cols, cols + 4, cols + 8)
    _layernorm(entry, 5, 1024, 1024, 1024)


@pytest.mark.parametrize('entry', R.LN_ENTRIES)
def test_layernorm_rows_second_trip_of_the_grid_stride(entry):
    rows, cols = R.LN_SECOND_TRIP
    _layernorm(entry, rows, cols, cols + 4, cols)


def _geglu(rows, inner, ldx, ldy):
    L, lib = _lib()
    x = R.geglu_inputs(rows, inner, ldx)
    xd, yd = _place(torch.from_numpy(x)), _out(rows, ldy)
    assert lib.ds_geglu(_ptr(xd), ldx, _ptr(yd), ldy, rows, inner, L.stream_ptr()) == 0
    torch.cuda.synchronize()
    got = _check_out(yd, rows, ldy, inner, 'geglu')
    y, bound = R.geglu_ref(x, inner)
    assert R.inside(got, y, bound).all(), (rows, inner, R.worst(got, y, bound))


def test_geglu_every_element():
    for inner in R.GEGLU_INNER:
        for rows in (1, 5):
            _geglu(rows, inner, 2 * inner + 4, inner + 4)


def test_geglu_second_trip_of_the_grid_stride():
    rows, inner = R.GEGLU_SECOND_TRIP
    _geglu(rows, inner, 2 * inner, inner)


@pytest.mark.parametrize('swap', [0, 1, 2, 3])
def test_noise_embedding_every_element(swap):
    L, lib = _lib()
    for bs, nch, out_ld in R.NOISE_SHAPES:
        sigma, freqs = R.noise_inputs(bs, nch, swap)
        sd, fd, od = _vec(sigma), _vec(freqs), _out(bs, out_ld)
        assert lib.ds_noise_embed(_ptr(sd), bs, _ptr(fd), nch, swap, _ptr(od), out_ld, L.stream_ptr()) == 0
        torch.cuda.synchronize()
        got = _check_out(od, bs, out_ld, nch, 'noise_embed')
        y, bound = R.noise_embed_ref(sigma, freqs, swap)
        assert R.inside(got, y, bound).all(), (swap, bs, nch, R.worst(got, y, bound))
