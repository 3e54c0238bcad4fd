"""CPU-only: precision / recall / density / coverage (diff_sampler_amd/prdc.py; reference sfd-main/prdc.py).

The second library (csrc/metrics/libdsmetrics.so) cross-compiles, exports exactly its header and answers argument errors on the host; the
sampling engine's build inputs and ABI are untouched by it; the host path of `compute_prdc` equals the golden recorded from the reference
implementation (tools/gen_prdc_golden.py) and, on an integer lattice with planted duplicates, a direct restatement EXACTLY; the command
line on image folders equals `compute_prdc` on the same features, under one process and under two gloo ranks."""
import ctypes as C
import multiprocessing as mp
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diff_sampler_amd import prdc as P  # noqa: E402
from tests import _prdc_cases as cases  # noqa: E402

METRICS = ('precision', 'recall', 'density', 'coverage')


# ------------------------------------------------------------------------------------------------------------------ library surface
@pytest.fixture(scope='module')
def lib():
    from diff_sampler_amd import build, _metrics_lib
    build.build_metrics_lib(verbose=False)
    return _metrics_lib.load()


def test_metrics_library_builds_and_exports_exactly_its_header(lib):
    from diff_sampler_amd import _metrics_lib
    header = open(os.path.join(ROOT, 'diff_sampler_amd', 'csrc', 'metrics', 'ds_metrics.h')).read()
    declared = set(re.findall(r'^DSM_API\s+(?:int|long long|const char\*|void)\s+(dsm_\w+)\s*\(', header, flags=re.M))
    assert declared and not re.findall(r'^(?:int|long long|const char\*|void)\s+dsm_\w+\s*\(', header, flags=re.M), 'an entry point without DSM_API'
    assert set(_metrics_lib.EXPORTS) == declared
    nm = subprocess.run(['nm', '-D', '--defined-only', _metrics_lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    text = {ln.split()[2] for ln in nm.splitlines() if len(ln.split()) == 3 and ln.split()[1] in 'TtWw'}
    assert text == declared, (sorted(text - declared), sorted(declared - text))
    assert lib.dsm_version() == _metrics_lib.DSM_VERSION == int(re.search(r'#define DSM_VERSION (\d+)', header).group(1))
    assert _metrics_lib.DSM_MAX_K == int(re.search(r'#define DSM_MAX_K (\d+)', header).group(1)) >= 8
    assert lib.dsm_error_string(-3) == b'unsupported shape' and lib.dsm_error_string(-1) == b'invalid argument'


def test_missing_or_mismatched_metrics_library_fails_loudly(lib, monkeypatch, tmp_path):
    from diff_sampler_amd import _metrics_lib
    monkeypatch.setattr(_metrics_lib, '_lib', None)
    monkeypatch.setattr(_metrics_lib, 'LIB_PATH', str(tmp_path / 'nope.so'))
    with pytest.raises(_metrics_lib.DsMetricsError, match='no CPU fallback'):
        _metrics_lib.load()
    monkeypatch.setattr(_metrics_lib, 'LIB_PATH', os.path.join(ROOT, 'diff_sampler_amd', 'csrc', 'metrics', 'libdsmetrics.so'))
    monkeypatch.setattr(_metrics_lib, 'DSM_VERSION', 99)
    with pytest.raises(_metrics_lib.DsMetricsError, match='ABI version'):
        _metrics_lib.load()


def test_argument_errors_are_answered_on_the_host(lib):
    """Every rejection comes back before any launch -- no GPU is needed (or touched) for them."""
    from diff_sampler_amd._metrics_lib import DS_E_ARG, DS_E_SHAPE
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    big = 1 << 30

    def knn(x=p, ld=8, n=20, dim=8, k=5, out=p, ws=p, nbytes=big):
        return lib.dsm_knn_radii_sq(x, 0, ld, n, dim, k, out, ws, nbytes, None)

    assert knn(x=None) == knn(out=None) == knn(ws=None) == DS_E_ARG                  # null pointers
    assert knn(ld=7) == DS_E_ARG                                                     # ld < dim
    assert knn(k=0) == DS_E_ARG and knn(k=-1) == DS_E_ARG                            # k < 1
    assert knn(n=5, k=5) == DS_E_ARG                                                 # k + 1 > n
    assert knn(n=6, k=5, nbytes=0) == DS_E_ARG                                       # (k + 1 == n is fine; the workspace is not)
    assert knn(k=9) == DS_E_SHAPE                                                    # beyond the instantiated list size
    assert knn(n=65535 * 128 + 1, nbytes=1 << 62) == DS_E_SHAPE                      # more bands than a grid dimension holds
    need = lib.dsm_prdc_workspace_bytes(20, 20, 5)
    assert need > 0 and knn(nbytes=need - 1) == DS_E_ARG                             # workspace too small
    assert lib.dsm_prdc_workspace_bytes(0, 20, 5) < 0 and lib.dsm_prdc_workspace_bytes(20, 20, 0) < 0

    def cross(real=p, ld_r=8, n_real=20, fake=p, ld_f=8, n_fake=30, dim=8, rr=p, rf=p, cnt=p, hit=p, mn=p, mask=None, rls=None, ws=p, nbytes=big):
        return lib.dsm_prdc_cross(real, 0, ld_r, n_real, fake, 1, ld_f, n_fake, dim, rr, rf, cnt, hit, mn, mask, rls, ws, nbytes, None)

    for name in ('real', 'fake', 'rr', 'rf', 'cnt', 'hit', 'mn', 'ws'):
        assert cross(**{name: None}) == DS_E_ARG, name
    assert cross(mask=p) == DS_E_ARG and cross(rls=p) == DS_E_ARG                    # the realism pair comes together or not at all
    assert cross(ld_r=7) == DS_E_ARG and cross(ld_f=7) == DS_E_ARG
    assert cross(n_real=0) == DS_E_ARG and cross(n_fake=0) == DS_E_ARG and cross(dim=0) == DS_E_ARG
    assert cross(nbytes=0) == DS_E_ARG
    # the column split is a function of the sizes alone: 10 000 rows = 79 bands get several workgroups each, one tile cannot be split
    assert lib.dsm_prdc_splits(10000, 10000) > 1 and lib.dsm_prdc_splits(100, 100) == 1 and lib.dsm_prdc_splits(0, 5) < 0


def test_the_engine_library_does_not_see_the_metrics_sources():
    """The tile table and the profile ties hang on build.source_sha256: nothing under csrc/metrics/ may enter the engine's sources, headers
    or hashes, and libdsamd.so gets no new entry point."""
    from diff_sampler_amd import build, _lib
    assert build.metrics_sources() and all(os.sep + 'metrics' + os.sep in s for s in build.metrics_sources())
    assert not [f for f in build.sources() + build.headers() if 'metrics' in f]
    assert len(_lib.EXPORTS) == 61 and not [e for e in _lib.EXPORTS if e.startswith('dsm_')]


# ------------------------------------------------------------------------------------------------------------------ host path
@pytest.fixture(scope='module')
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, 'prdc_small.npz'))


@pytest.mark.parametrize('case', ['a', 'b', 'c'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_host_path_equals_the_reference_golden(golden, case, dtype):
    """The four metrics EXACTLY (the golden's generator checked the decision gap of every case); radii and realism to 1e-12 relative: the
    same fp64 expansion as sklearn's with another BLAS summation order."""
    p = case + '_'
    real, fake, k = golden[p + 'real'].astype(dtype), golden[p + 'fake'].astype(dtype), int(golden[p + 'k'])
    got = P.compute_prdc(real, fake, k, realism=True)
    for m in METRICS:
        assert got[m] == golden[p + m], (m, got[m], golden[p + m])
    assert np.abs(got['realism'] / golden[p + 'realism'] - 1).max() <= 1e-12
    for which, feats in (('radii_real', real), ('radii_fake', fake)):
        r = P.compute_nearest_neighbour_distances(feats, k)
        assert r.dtype == np.float64 and np.abs(r / golden[p + which] - 1).max() <= 1e-12
    assert set(P.compute_prdc(torch.from_numpy(real), torch.from_numpy(fake), k)) == set(METRICS)      # torch in, no realism key


def test_parity_functions_follow_the_reference(golden):
    real, k = golden['b_real'].astype(np.float64), int(golden['b_k'])
    d = P.compute_pairwise_distance(real)
    assert d.shape == (37, 37) and np.all(np.diag(d) == 0) and np.allclose(d, np.sqrt(cases.direct_sq(real, real)), rtol=1e-12, atol=1e-12)
    assert np.abs(P.get_kth_value(d, k=k + 1, axis=-1) / golden['b_radii_real'] - 1).max() <= 1e-12
    assert torch.equal(P.get_kth_value(torch.from_numpy(d), k + 1), torch.from_numpy(P.get_kth_value(d, k + 1)))
    dxy = P.compute_pairwise_distance(real, golden['b_fake'])
    assert dxy.shape == (37, 41) and np.allclose(dxy, np.sqrt(cases.direct_sq(real, golden['b_fake'])), rtol=1e-12, atol=1e-12)
    with pytest.raises(ValueError):
        P.compute_prdc(real[:5], real, 5)                                           # nearest_k + 1 > n
    lines = []
    np.random.seed(0)
    fake = golden['b_fake'].astype(np.float64)[:37]
    s = P.compute_scores(['prdc'], [real, fake], log=lines.append)
    assert [ln.split(':')[0] for ln in lines[1:]] == list(METRICS) and lines[1] == f'precision: {s["precision"]:.5f}'
    # equal set sizes below 10 000: the random subsampling keeps every row, so the scores are those of the two sets in another row order
    want = P.compute_prdc(real, fake, 5)
    assert all(s[m] == want[m] for m in METRICS)


def test_host_path_in_several_row_blocks(monkeypatch):
    """The host path works in blocks of `_BLOCK` rows: counts and the realism maximum accumulate over blocks and the zeroed diagonal moves
    with the block.  With 64-row blocks the lattice (200 x 180) takes four: still exact, and the Gaussian golden still matches."""
    monkeypatch.setattr(P, '_BLOCK', 64)
    c = cases.lattice_case()
    assert np.array_equal(P.compute_nearest_neighbour_distances(c['real'], cases.LATTICE_K), np.sqrt(c['rr']))
    got = P.compute_prdc(c['real'], c['fake'], cases.LATTICE_K, realism=True)
    assert all(got[m] == c['metrics'][m] for m in METRICS)
    assert np.array_equal(got['realism'], np.sqrt(c['rls']), equal_nan=True)
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'prdc_small.npz'))
    got = P.compute_prdc(z['a_real'], z['a_fake'], int(z['a_k']), realism=True)
    assert all(got[m] == z['a_' + m] for m in METRICS) and np.abs(got['realism'] / z['a_realism'] - 1).max() <= 1e-12


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_integer_lattice_equals_the_direct_restatement_exactly(dtype):
    """Features in {0, 1, 2}: every squared distance is an exact integer whatever the order of summation, so strict <, multiplicity
    (six identical rows: a radius of exactly 0) and the zeroed diagonal are pinned by equality -- radii and realism included."""
    c = cases.lattice_case()
    real, fake, k = c['real'].astype(dtype), c['fake'].astype(dtype), cases.LATTICE_K
    assert np.array_equal(P.compute_nearest_neighbour_distances(real, k), np.sqrt(c['rr']))
    assert np.array_equal(P.compute_nearest_neighbour_distances(fake, k), np.sqrt(c['rf']))
    got = P.compute_prdc(real, fake, k, realism=True)
    for m in METRICS:
        assert got[m] == c['metrics'][m], m
    assert np.array_equal(got['realism'], np.sqrt(c['rls']), equal_nan=True)


# ------------------------------------------------------------------------------------------------------------------ command line, ranks
def _toy_detector(device):
    """module:factory detector: 8 fixed random projections of the 4 x 4 mean-pooled image (deterministic)."""
    g = torch.Generator().manual_seed(0)
    w = torch.randn(3 * 4 * 4, 8, generator=g).to(device)

    def f(images):
        x = torch.nn.functional.adaptive_avg_pool2d(images.to(torch.float32) / 255.0, 4).reshape(images.shape[0], -1)
        return x @ w
    return f


DETECTOR = 'tests.test_prdc_cpu:_toy_detector'


def _write_folders(tmp_path):
    import PIL.Image
    rng = np.random.RandomState(3)
    sets = {}
    for name, n, lo in (('ref', 31, 0), ('gen', 26, 40)):
        d = tmp_path / name / '000000'
        d.mkdir(parents=True)
        imgs = rng.randint(lo, 256, size=(n, 8, 8, 3), dtype=np.uint8)
        for i, a in enumerate(imgs):
            PIL.Image.fromarray(a, 'RGB').save(d / f'{i:06d}.png')
        sets[name] = imgs
    return sets


def _cli_args(tmp_path, *extra):
    return ['calc', '--images', str(tmp_path / 'gen'), '--images_ref', str(tmp_path / 'ref'), '--detector', DETECTOR, '--device', 'cpu',
            '--nearest_k', '3', *extra]


def _parse(output):
    return {ln.split(':')[0]: ln.split(':')[1].strip() for ln in output.splitlines() if ln.split(':')[0] in METRICS}


def _rank_cli(rank, world, port, args, q):
    import torch.distributed as dist
    from click.testing import CliRunner
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    r = CliRunner().invoke(P.main, args)
    q.put((rank, r.exit_code, r.output))
    dist.destroy_process_group()


def test_cli_equals_compute_prdc_on_one_process_and_on_two_gloo_ranks(tmp_path):
    from click.testing import CliRunner
    sets = _write_folders(tmp_path)
    det = _toy_detector('cpu')
    feats = {k: det(torch.from_numpy(v).permute(0, 3, 1, 2)) for k, v in sets.items()}
    want = P.compute_prdc(feats['ref'], feats['gen'], 3)
    assert 0 < want['precision'] and 0 < want['coverage']                           # not a degenerate pair of folders
    r = CliRunner().invoke(P.main, _cli_args(tmp_path, '--batch', '7'))
    assert r.exit_code == 0, r.output
    one = _parse(r.output)
    assert one == {m: f'{want[m]:.5f}' for m in METRICS}
    assert [ln.split(':')[0] for ln in r.output.splitlines()[-4:]] == list(METRICS)  # the reference's `key: value` lines, its order
    # --num: the dataset's subset rule on both folders; more than there are is an error, not a silent smaller set
    from diff_sampler_amd import fid
    r = CliRunner().invoke(P.main, _cli_args(tmp_path, '--num', '20', '--seed', '5'))
    assert r.exit_code == 0, r.output
    sub = {k: feats[k][torch.from_numpy(fid.ImageFolder(str(tmp_path / k), max_size=20, random_seed=5).idx)] for k in feats}
    w20 = P.compute_prdc(sub['ref'], sub['gen'], 3)
    assert _parse(r.output) == {m: f'{w20[m]:.5f}' for m in METRICS}
    assert CliRunner().invoke(P.main, _cli_args(tmp_path, '--num', '30')).exit_code != 0
    # two ranks: the batches are sharded, the features combined, rank 0 prints the same numbers and rank 1 nothing
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    procs = [ctx.Process(target=_rank_cli, args=(rk, 2, port, _cli_args(tmp_path, '--batch', '4'), q)) for rk in range(2)]
    [p.start() for p in procs]
    got = dict((rk, (code, out)) for rk, code, out in (q.get(timeout=120) for _ in range(2)))
    [p.join(60) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    assert got[0][0] == 0 and got[1][0] == 0, got
    assert _parse(got[0][1]) == one and got[1][1].strip() == ''
