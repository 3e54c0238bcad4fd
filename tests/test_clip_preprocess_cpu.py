"""CPU-only: the device resize and crop of the CLIP score (diff_sampler_amd/clip_preprocess.py, csrc/metrics/image_prep.hip).

The numpy restatement of the two integer passes equals PIL's resize + crop byte for byte; the crop geometry is ``preprocess``'s, halves
rounded to even included; the entry point is declared, bound and refuses bad arguments on the host; the kernel needs no scratch;
``calc_clip_score(device_resize=True)`` resizes once per image size and keeps every image with its caption."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diff_sampler_amd import clip_preprocess as P, clip_score as CS  # noqa: E402

# (h, w, size): square, both orientations with a crop, one pass skipped, the copy, upscaling (ksize 5), deep and flagship downscaling
GEOMETRIES = [(33, 33, 28), (53, 37, 28), (37, 53, 28), (29, 28, 28), (28, 28, 28), (20, 20, 28), (512, 512, 28), (512, 512, 224),
              (480, 640, 224), (64, 64, 224)]


def make_image(kind, h, w, seed=0):
    rng = np.random.default_rng(seed + 1000 * h + w)
    if kind == 'noise':
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == 'ramp':
        y, x = np.mgrid[0:h, 0:w]
        return np.stack([255 * x // max(w - 1, 1), 255 * y // max(h - 1, 1), 255 * (x + y) // max(h + w - 2, 1)], axis=2).astype(np.uint8)
    return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)            # 0 / 255 only: overshoot on both sides, both clamps


def pil_preprocess(a, size):
    import PIL.Image
    return CS.preprocess(PIL.Image.fromarray(a), size).numpy()


@pytest.mark.parametrize('kind', ['noise', 'ramp', 'binary'])
@pytest.mark.parametrize('h,w,size', GEOMETRIES)
def test_reference_equals_pil_byte_for_byte(h, w, size, kind):
    a = make_image(kind, h, w)
    got, want = P.resize_reference(a, size), pil_preprocess(a, size)
    assert got.shape == want.shape == (3, size, size) and got.dtype == np.uint8
    mismatches = int((got != want).sum())
    print(f'{h}x{w} -> {size} {kind}: {mismatches} mismatching bytes')
    assert mismatches == 0


def test_binary_image_reaches_both_clamps():
    """The 0 / 255 image drives accumulators below 0 and above 255 << 22: without the clamp the bytes would wrap."""
    a = make_image('binary', 33, 33)
    b, c = P.resample_coeffs(33, 28)
    lo = hi = 0
    for j in range(28):
        xmin, n = b[j]
        s = (1 << 21) + (a[:, xmin:xmin + n, 0].astype(np.int64) * c[j, :n]).sum(axis=1)
        lo, hi = min(lo, int(s.min()) >> 22), max(hi, int(s.max()) >> 22)
    assert lo < 0 and hi > 255


def test_coefficient_tables():
    b, c = P.resample_coeffs(512, 224)
    assert b.shape == (224, 2) and c.shape == (224, 11) and b.dtype == c.dtype == np.int32           # support 2 * 512 / 224 = 4.57: ksize 2 * 5 + 1
    assert P.resample_coeffs(20, 28)[1].shape == (28, 5) and P.resample_coeffs(2048, 224)[1].shape[1] == 39
    for n_in, n_out in ((512, 224), (20, 28), (37, 28), (2048, 224), (64, 224)):
        b, c = P.resample_coeffs(n_in, n_out)
        assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= n_in).all() and (b[:, 1] >= 1).all() and (b[:, 1] <= c.shape[1]).all()
        assert (np.diff(b[:, 0]) >= 0).all() and (np.diff(b[:, 0] + b[:, 1]) >= 0).all()             # the band's rows: first row's first tap ... last row's last
        assert (np.abs(c.sum(axis=1) - (1 << 22)) <= c.shape[1]).all()                               # weights sum to 1 up to one rounding each
        assert int(np.abs(c).max()) < P.COEFF_LIMIT                                                  # the 24-bit multiplier is exact
        assert all((c[i, b[i, 1]:] == 0).all() for i in range(n_out))
    assert b[0, 0] == 0 and b[-1, 0] + b[-1, 1] == 64                        # upscaling: clipped at both edges
    assert P.resample_coeffs(512, 224)[0] is P.resample_coeffs(512, 224)[0]  # cached
    with pytest.raises(ValueError):
        P.resample_coeffs(0, 5)


@pytest.mark.parametrize('h,w,size', GEOMETRIES + [(33, 30, 28), (30, 33, 28), (31, 28, 28), (28, 35, 28), (224, 224, 224), (225, 224, 224), (100, 37, 28)])
def test_crop_geometry_is_preprocess(h, w, size):
    """``preprocess`` run on a stand-in image that records the resize and the crop it is asked for."""
    calls = {}

    class Img:
        def __init__(self, s):
            self.size = s

        def convert(self, mode):
            return self

        def resize(self, s, resample):
            calls['resize'] = s
            return Img(s)

        def crop(self, box):
            calls['crop'] = box
            return np.zeros((size, size, 3), np.uint8)

        def __array__(self, dtype=None, copy=None):
            return np.zeros((size, size, 3), np.uint8)

    CS.preprocess(Img((w, h)), size)
    nh, nw, top, left = P.crop_geometry(h, w, size)
    assert calls.get('resize', (w, h)) == (nw, nh)
    assert calls.get('crop', (0, 0, size, size)) == (left, top, left + size, top + size)
    assert 0 <= top <= nh - size and 0 <= left <= nw - size


def test_crop_offset_halves_round_to_even():
    assert P.crop_geometry(33, 28, 28) == (33, 28, 2, 0)              # (33 - 28) / 2 = 2.5 -> 2
    assert P.crop_geometry(35, 28, 28) == (35, 28, 4, 0)              # 3.5 -> 4
    assert P.crop_geometry(28, 31, 28) == (28, 31, 0, 2)              # 1.5 -> 2
    assert P.crop_geometry(37, 53, 28) == (28, 40, 0, 6) and P.crop_geometry(53, 37, 28) == (40, 28, 6, 0)


# ------------------------------------------------------------------------------------------------------------------ library surface
@pytest.fixture(scope='module')
def mlib():
    from diff_sampler_amd import build, _metrics_lib
    build.build_metrics_lib(verbose=False)
    return _metrics_lib.load()


def test_entry_point_is_declared_and_bound(mlib):
    from diff_sampler_amd import _metrics_lib
    header = open(os.path.join(ROOT, 'diff_sampler_amd', 'csrc', 'metrics', 'ds_metrics.h')).read()
    assert re.search(r'^DSM_API\s+int\s+dsm_resize_crop_u8\s*\(', header, flags=re.M)
    assert 'dsm_resize_crop_u8' in _metrics_lib.EXPORTS and hasattr(mlib, 'dsm_resize_crop_u8')
    assert mlib.dsm_version() == _metrics_lib.DSM_VERSION == 2
    assert len(_metrics_lib._SIGNATURES['dsm_resize_crop_u8'][1]) == 19


def test_stale_library_is_reported_as_such(monkeypatch, tmp_path):
    """A library built before the entry point existed: DsMetricsError with the rebuild advice, not a bare AttributeError."""
    import shutil
    import subprocess
    from diff_sampler_amd import _metrics_lib
    cc = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang') or '/opt/rocm/llvm/bin/clang'
    src = tmp_path / 'old.c'
    src.write_text('int dsm_version(void) { return 2; }\n')
    subprocess.run([cc, '-shared', '-fPIC', '-o', str(tmp_path / 'libold.so'), str(src)], check=True)
    monkeypatch.setattr(_metrics_lib, '_lib', None)
    monkeypatch.setattr(_metrics_lib, 'LIB_PATH', str(tmp_path / 'libold.so'))
    with pytest.raises(_metrics_lib.DsMetricsError, match='rebuild it'):
        _metrics_lib.load()


def test_entry_point_rejects_bad_arguments_on_the_host(mlib):
    from diff_sampler_amd._metrics_lib import DS_E_ALIGN, DS_E_ARG, DS_E_SHAPE
    buf = (C.c_int * 4096)()
    base = (C.addressof(buf) + 63) & ~63
    p = C.c_void_p(base)

    def call(**kw):
        a = dict(src=p, stride=512 * 1536, pitch=1536, n=1, h=512, w=512, nh=224, nw=224, top=0, left=0, size=224, hb=p, hc=p, hk=11, vb=p, vc=p,
                 vk=11, out=p)
        a.update(kw)
        return mlib.dsm_resize_crop_u8(a['src'], a['stride'], a['pitch'], a['n'], a['h'], a['w'], a['nh'], a['nw'], a['top'], a['left'], a['size'],
                                       a['hb'], a['hc'], a['hk'], a['vb'], a['vc'], a['vk'], a['out'], None)

    assert call(src=None) == call(out=None) == call(hb=None) == call(hc=None) == call(vb=None) == call(vc=None) == DS_E_ARG
    assert call(n=0) == call(h=0) == call(w=0) == call(nh=0) == call(nw=0) == call(size=0) == call(stride=-1) == DS_E_ARG
    assert call(pitch=1535) == DS_E_ARG                                   # pitch < 3 w
    assert call(hk=10) == call(vk=10) == call(hk=0) == DS_E_ARG           # 512 -> 224 needs ksize 11
    assert call(top=1) == call(left=1) == call(top=-1) == call(size=225) == DS_E_ARG      # the window leaves the resized image
    assert call(out=C.c_void_p(base + 4)) == call(hc=C.c_void_p(base + 2)) == call(vb=C.c_void_p(base + 1)) == DS_E_ALIGN
    # beyond the LDS envelope: four source rows wider than 24 KB; one output row whose taps need more than 40 KB of resized rows
    assert call(w=2049, pitch=3 * 2049, hk=39, stride=512 * 3 * 2049) == DS_E_SHAPE
    assert call(h=8192, vk=149, stride=8192 * 1536) == DS_E_SHAPE
    assert call(h=40000, vk=800) == DS_E_SHAPE
    # a skipped pass needs no table: the NULL pointers are not what is refused here, the pitch is
    assert call(h=224, w=224, hb=None, hc=None, vb=None, vc=None, hk=0, vk=0, pitch=671) == DS_E_ARG


def test_kernel_needs_no_scratch():
    """Twelve accumulators, four row pointers and four taps' loads in flight per thread: no private memory in any of the three load
    widths, and registers for at least the four waves per SIMD that the LDS of the smallest band leaves room for (512 / 4 = 128)."""
    import shutil
    import subprocess
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    src = os.path.join(ROOT, 'diff_sampler_amd', 'csrc', 'metrics', 'image_prep.hip')
    r = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-c', src, '-o', os.devnull, '-Rpass-analysis=kernel-resource-usage'],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    found = re.findall(r'Function Name: (\S*resize_crop_kernel\S*).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)',
                       r.stderr, flags=re.S)
    assert len(found) == 3, r.stderr[-1500:]
    for name, vgpr, scratch, occ in found:
        print(f'{name}: VGPRs {vgpr}, scratch {scratch}, occupancy {occ} waves/SIMD')
        assert int(scratch) == 0 and int(vgpr) <= 128


# ------------------------------------------------------------------------------------------------------------------ calc_clip_score
class StubScorer:
    """Scores an image by its first pixel; records what it was given."""

    class spec:
        image_size = 28

    device = 'cpu'

    def __init__(self):
        self.total = torch.zeros(1, dtype=torch.float64)
        self.calls = []

    def reset(self):
        self.total.zero_()

    def score(self, images, prompts):
        assert images.dtype == torch.uint8 and tuple(images.shape[1:]) == (3, 28, 28) and len(images) == len(prompts)
        self.calls.append((images.clone(), list(prompts)))
        self.total += float(len(prompts))
        return torch.zeros(len(prompts))


def test_calc_clip_score_device_resize_groups_by_size_and_keeps_order(tmp_path, monkeypatch):
    import PIL.Image
    sizes = [(33, 33), (53, 37), (33, 33), (53, 37), (53, 37), (33, 33), (33, 33)]
    arrays = [make_image('noise', h, w, seed=i) for i, (h, w) in enumerate(sizes)]
    d = tmp_path / 'images'
    d.mkdir()
    for i, a in enumerate(arrays):
        PIL.Image.fromarray(a, 'RGB').save(d / f'{i:06d}.png')
    captions = [f'caption {i}' for i in range(len(arrays))]
    resized = []

    def host_resize(images, size, device='cuda'):            # stands in for the device call: same contract, computed by the restatement
        resized.append(tuple(images.shape))
        return torch.from_numpy(np.stack([P.resize_reference(a.numpy(), size) for a in images]))

    monkeypatch.setattr(P, 'resize_center_crop', host_resize)
    dev, host = StubScorer(), StubScorer()
    avg, n = CS.calc_clip_score(dev, str(d), captions, max_batch_size=5, log=lambda *a: None, device_resize=True)
    avg_h, n_h = CS.calc_clip_score(host, str(d), captions, max_batch_size=5, log=lambda *a: None)
    assert (avg, n) == (avg_h, n_h) == (1.0, 7)
    # one resize per size of every batch fid.shard_items forms, sizes in order of first appearance
    from diff_sampler_amd import fid
    want = []
    for idx in fid.shard_items(7, 5, 0, 1):
        members = [sizes[i] for i in idx.tolist()]
        want += [(members.count(s), *s, 3) for s in dict.fromkeys(members)]
    assert resized == want and len(want) == 4 and {w[0] for w in want} == {1, 2}       # both batches hold both sizes
    assert len(dev.calls) == len(host.calls) == 2
    for (gi, gp), (wi, wp) in zip(dev.calls, host.calls):
        assert gp == wp and torch.equal(gi, wi)              # every image at its caption's position, with the host path's bytes
    assert [p for _, ps in dev.calls for p in ps] == captions


def test_cli_has_the_flag_off_by_default():
    opts = {o.name: o for o in CS.main.commands['calc'].params}
    assert opts['device_resize'].is_flag and opts['device_resize'].default is False
