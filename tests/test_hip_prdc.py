"""Precision / recall / density / coverage on the GPU (csrc/metrics/prdc.hip through libdsmetrics.so; reference sfd-main/prdc.py).

The reference of every case is the direct restatement  sum_c (x_ic - y_jc)^2  in numpy fp64 (tests/_prdc_cases.py), computed once per
case before anything runs on the device.  Tolerances:
  * squared radii and row minima: 1e-12 of the LARGEST squared distance of the case -- the bound tests/test_hip_fid.py uses for an fp64
    contraction summed in another order (the expansion's terms |x|^2, |y|^2, 2 x.y are of that size, fp64 carries 2^-53);
  * realism_sq = r^2 / d^2: 1e-12 RELATIVE -- the separation condition (d^2 >= 1e-2 (|x|^2 + |y|^2)) bounds the relative error of d^2 by a
    hundred times that of the expansion's terms, about 1e-14 for these lengths;
  * counts, hits, and the four metrics: EXACT, legitimate because the decision-gap condition holds on these inputs (asserted in
    _prdc_cases.conditions; a seed that fails it is replaced there, not skipped);
  * the integer lattice: everything exact, radii and realism included."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diff_sampler_amd import prdc as P  # noqa: E402
from tests import _prdc_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

METRICS = ('precision', 'recall', 'density', 'coverage')
GUARD = 777.0


def _lib():
    from diff_sampler_amd import _metrics_lib
    return _metrics_lib.load()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    from diff_sampler_amd import _lib as engine_lib
    return engine_lib.stream_ptr()


def _knn(x, ld, n, dim, k):
    """dsm_knn_radii_sq through the C ABI on a device tensor [n][ld]; one guard element behind the output."""
    lib = _lib()
    out = torch.full((n + 1,), GUARD, dtype=torch.float64, device='cuda')
    ws = torch.empty(lib.dsm_prdc_workspace_bytes(n, n, k), dtype=torch.uint8, device='cuda')
    rc = lib.dsm_knn_radii_sq(_ptr(x), int(x.dtype == torch.float64), ld, n, dim, k, _ptr(out), _ptr(ws), ws.numel(), _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.dsm_error_string(rc)
    got = out.cpu().numpy()
    assert got[-1] == GUARD
    return got[:-1]


def _cross(real, ld_r, n_real, fake, ld_f, n_fake, dim, rr, rf, mask):
    """dsm_prdc_cross through the C ABI; guard elements behind all four outputs."""
    lib = _lib()
    dev = dict(device='cuda')
    count = torch.full((n_fake + 1,), 777, dtype=torch.int32, **dev)
    hit = torch.full((n_real + 1,), 777, dtype=torch.int32, **dev)
    mn = torch.full((n_real + 1,), GUARD, dtype=torch.float64, **dev)
    rls = torch.full((n_fake + 1,), GUARD, dtype=torch.float64, **dev) if mask is not None else None
    m8 = torch.from_numpy(mask.astype(np.uint8)).cuda() if mask is not None else None
    rr_d, rf_d = torch.from_numpy(np.array(rr)).cuda(), torch.from_numpy(np.array(rf)).cuda()
    ws = torch.empty(lib.dsm_prdc_workspace_bytes(n_real, n_fake, 1), dtype=torch.uint8, **dev)
    rc = lib.dsm_prdc_cross(_ptr(real), int(real.dtype == torch.float64), ld_r, n_real, _ptr(fake), int(fake.dtype == torch.float64), ld_f, n_fake,
                            dim, _ptr(rr_d), _ptr(rf_d), _ptr(count), _ptr(hit), _ptr(mn), _ptr(m8), _ptr(rls), _ptr(ws), ws.numel(), _stream())
    torch.cuda.synchronize()
    assert rc == 0, lib.dsm_error_string(rc)
    outs = [t.cpu().numpy() if t is not None else None for t in (count, hit, mn, rls)]
    assert all(o is None or o[-1] == 777 for o in outs), 'a guard element was overwritten'
    return [o[:-1] if o is not None else None for o in outs]


@pytest.mark.parametrize('f64', [False, True], ids=['fp32', 'fp64'])
@pytest.mark.parametrize('n,dim,k', [(6, 16, 5), (37, 7, 5), (130, 50, 1), (300, 64, 5), (513, 200, 3), (1000, 96, 5)])
def test_knn_radii_sq_matches_direct_distances(n, dim, k, f64):
    """Ragged n and dim against every tile size (128 rows, 16 features, 4 per MFMA), k + 1 == n, k = 1, ld = dim + 8; the (k + 1)-th smallest
    with the diagonal at exactly 0; two runs give equal bits."""
    ld = dim + 8
    x = cases.features(n, ld, seed=n * 1000 + dim, dtype=np.float64 if f64 else np.float32)
    d = cases.direct_sq(x[:, :dim], x[:, :dim])
    want = cases.radii_sq_of(d, k)
    lib = _lib()
    if n == 1000:                                               # several row bands AND several column splits, merged from partial lists
        splits = lib.dsm_prdc_splits(n, n)
        assert -(-n // 128) > 1 and splits > 1
        assert lib.dsm_prdc_workspace_bytes(n, n, k) >= splits * n * (k + 1) * 8
    xd = torch.from_numpy(x).cuda()
    got = _knn(xd, ld, n, dim, k)
    print(f'knn n={n} dim={dim} k={k} f64={f64}: max |err| / max d2 = {np.abs(got - want).max() / d.max():.2e}')
    assert np.abs(got - want).max() <= 1e-12 * d.max()
    assert np.array_equal(got, _knn(xd, ld, n, dim, k))


CROSS_CASES = [(37, 41, 7, False, False), (37, 41, 7, True, True), (130, 333, 50, False, False), (130, 333, 50, True, False),
               (130, 333, 50, False, True), (300, 257, 64, False, False), (300, 257, 64, True, True), (1000, 777, 96, False, False),
               (1000, 777, 96, True, True)]


@pytest.mark.parametrize('n_real,n_fake,dim,real_f64,fake_f64', CROSS_CASES)
def test_prdc_cross_matches_direct_distances(n_real, n_fake, dim, real_f64, fake_f64):
    """Radii handed in from numpy: the three integer / boolean outputs equal numpy EXACTLY, real_min_sq and realism_sq to 1e-12, with and
    without the realism pair, guards intact."""
    c = cases.gauss_case(n_real, n_fake, dim, f64=real_f64 and fake_f64)         # gap and separation asserted inside, on the CPU
    ld = dim + 8
    real = torch.tensor(c['real']).cuda().to(torch.float64 if real_f64 else torch.float32)   # mixed: the fp32 case, one set widened exactly
    fake = torch.tensor(c['fake']).cuda().to(torch.float64 if fake_f64 else torch.float32)
    count, hit, mn, rls = _cross(real, ld, n_real, fake, ld, n_fake, dim, c['rr'], c['rf'], c['mask'])
    print(f'cross {n_real}x{n_fake}x{dim}: min err {np.abs(mn - c["mn"]).max() / c["d"].max():.2e} realism rel err {np.abs(rls / c["rls"] - 1).max():.2e}')
    assert np.array_equal(count, c['count']) and np.array_equal(hit, c['hit'])
    assert np.array_equal(mn < c['rr'], c['mn'] < c['rr'])                      # coverage's booleans
    assert np.abs(mn - c['mn']).max() <= 1e-12 * c['d'].max()
    assert np.abs(rls / c['rls'] - 1).max() <= 1e-12
    count2, hit2, mn2, none = _cross(real, ld, n_real, fake, ld, n_fake, dim, c['rr'], c['rf'], None)
    assert none is None and np.array_equal(count2, count) and np.array_equal(hit2, hit) and np.array_equal(mn2, mn)


def _tiles(n):
    return -(-n // 128)


def test_knn_radii_sq_when_a_workgroup_walks_several_column_tiles():
    """Every shape above has as many column splits as column tiles: each workgroup sees ONE tile.  Here 32 tiles meet 16 splits, so the
    per-row lists and thresholds in LDS live on into a second tile (finite thresholds: the wave-uniform skip, inserts into a full list)
    under the next tile's staging -- what the metric's own size (10 000 rows: 6 splits of 13 - 14 tiles) runs."""
    c = cases.walk_case()
    n, dim, k, lib = cases.WALK_N_REAL, cases.WALK_DIM, cases.GAUSS_K, _lib()
    assert _tiles(n) >= 2 * lib.dsm_prdc_splits(n, n) > 2
    xd = torch.tensor(c['real']).cuda()
    got = _knn(xd, dim + 8, n, dim, k)
    print(f'knn walk n={n}: max |err| / max d2 = {np.abs(got - c["rr"]).max() / c["dmax_rr"]:.2e}')
    assert np.abs(got - c['rr']).max() <= 1e-12 * c['dmax_rr']
    assert np.array_equal(got, _knn(xd, dim + 8, n, dim, k))


def test_prdc_cross_when_a_workgroup_walks_several_column_tiles():
    """32 fake tiles over 16 splits: row minima and hit counts accumulate in registers over two tiles, the column counters are zeroed
    again and the column maxima rewritten behind the previous tile's read-out.  Same bounds as the one-tile cases."""
    c = cases.walk_case()
    nr, nf, dim, lib = cases.WALK_N_REAL, cases.WALK_N_FAKE, cases.WALK_DIM, _lib()
    assert _tiles(nf) >= 2 * lib.dsm_prdc_splits(nr, nf) > 2
    real, fake = torch.tensor(c['real']).cuda(), torch.tensor(c['fake']).cuda()
    count, hit, mn, rls = _cross(real, dim + 8, nr, fake, dim + 8, nf, dim, c['rr'], c['rf'], c['mask'])
    print(f'cross walk {nr}x{nf}: min err {np.abs(mn - c["mn"]).max() / c["dmax"]:.2e} realism rel err {np.abs(rls / c["rls"] - 1).max():.2e}')
    assert np.array_equal(count, c['count']) and np.array_equal(hit, c['hit'])
    assert np.array_equal(mn < c['rr'], c['mn'] < c['rr'])
    assert np.abs(mn - c['mn']).max() <= 1e-12 * c['dmax']
    assert np.abs(rls / c['rls'] - 1).max() <= 1e-12
    count2, hit2, mn2, none = _cross(real, dim + 8, nr, fake, dim + 8, nf, dim, c['rr'], c['rf'], None)
    assert none is None and np.array_equal(count2, count) and np.array_equal(hit2, hit) and np.array_equal(mn2, mn)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['fp32', 'fp64'])
def test_integer_lattice_on_the_device_is_exact(dtype):
    c = cases.lattice_case()
    k = cases.LATTICE_K
    real, fake = torch.tensor(c['real']).to(dtype).cuda(), torch.tensor(c['fake']).to(dtype).cuda()
    assert np.array_equal(_knn(real, 6, 200, 6, k), c['rr']) and np.array_equal(_knn(fake, 6, 180, 6, k), c['rf'])
    count, hit, mn, rls = _cross(real, 6, 200, fake, 6, 180, 6, c['rr'], c['rf'], c['mask'])
    assert np.array_equal(count, c['count']) and np.array_equal(hit, c['hit']) and np.array_equal(mn, c['mn'])
    assert np.array_equal(rls, c['rls'], equal_nan=True)
    got = P.compute_prdc(real, fake, k, realism=True)
    for m in METRICS:
        assert got[m] == c['metrics'][m], m
    assert np.array_equal(got['realism'], np.sqrt(c['rls']), equal_nan=True)
    assert np.array_equal(P.compute_nearest_neighbour_distances(real, k).cpu().numpy(), np.sqrt(c['rr']))


@pytest.mark.parametrize('case', ['a', 'b', 'c'])
def test_compute_prdc_on_the_device_equals_the_reference_golden_and_the_host_path(golden_dir, case):
    z = np.load(os.path.join(golden_dir, 'prdc_small.npz'))
    p = case + '_'
    k = int(z[p + 'k'])
    host = P.compute_prdc(z[p + 'real'], z[p + 'fake'], k, realism=True)
    for dtype in (np.float32, np.float64):
        real, fake = z[p + 'real'].astype(dtype), z[p + 'fake'].astype(dtype)
        got = P.compute_prdc(real, fake, k, realism=True, device='cuda')          # numpy in, computed on the engine
        for m in METRICS:
            assert got[m] == z[p + m] == host[m], (m, got[m], z[p + m], host[m])
        assert np.abs(got['realism'] / z[p + 'realism'] - 1).max() <= 1e-12
        r = P.compute_nearest_neighbour_distances(torch.from_numpy(real).cuda(), k)                  # a CUDA tensor selects the device by itself
        assert r.is_cuda and np.abs(r.cpu().numpy() / z[p + 'radii_real'] - 1).max() <= 1e-12
