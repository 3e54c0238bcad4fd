"""GPU: the device resize and crop of the CLIP score (csrc/metrics/image_prep.hip through clip_preprocess.resize_center_crop) against
``clip_score.preprocess`` (PIL) with ``torch.equal`` -- the arithmetic is integer, so the bar is equality; then the scorer and
``calc_clip_score`` on raw images against the host path, bit for bit.

Shapes: the smallest at which each path of the kernel runs -- a batch (image stride), crop offsets on either axis, a skipped pass of
either kind, the pure copy, upscaling (taps clipped at both edges), the three load widths with and without a row tail (pitch 16-, 4- and
1-byte aligned, from sliced parents so that pitch > 3 w), a size that is no multiple of 4 (byte stores), 512 x 512 -> 224 (15 bands of 15
rows: the last has 14) and 480 x 640 -> 224 (columns outside the crop never staged)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu


def _images(kind, n, h, w, seed=0):
    rng = np.random.default_rng(seed + 1000 * h + w)
    a = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    return a if kind == 'noise' else ((a > 127) * 255).astype(np.uint8)          # 0 / 255 only: both clamps


def _host(batch, size):
    import PIL.Image
    from diff_sampler_amd.clip_score import preprocess
    return torch.stack([preprocess(PIL.Image.fromarray(np.ascontiguousarray(a)), size) for a in batch.cpu().numpy()])


def _compare(x, size):
    from diff_sampler_amd.clip_preprocess import resize_center_crop
    got = resize_center_crop(x, size)
    torch.cuda.synchronize()
    want = _host(x, size)
    assert got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == (x.shape[0], 3, size, size)
    bad = int((got.cpu() != want).sum())
    print(f'{tuple(x.shape)} strides {tuple(x.stride())} -> {size}: {bad} mismatching bytes')
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize('kind', ['noise', 'binary'])
@pytest.mark.parametrize('n,h,w,size', [(3, 33, 33, 28), (1, 53, 37, 28), (1, 37, 53, 28), (1, 29, 28, 28), (1, 28, 29, 28), (2, 28, 28, 28),
                                        (1, 20, 20, 28), (2, 35, 31, 30), (2, 512, 512, 224), (1, 480, 640, 224)])
def test_resize_center_crop_equals_preprocess(n, h, w, size, kind):
    _compare(torch.from_numpy(_images(kind, n, h, w)), size)


@pytest.mark.parametrize('on_device', [False, True])
@pytest.mark.parametrize('parent_w,first', [(39, 1), (40, 0), (40, 3), (48, 0), (64, 16)])
def test_sliced_sources(parent_w, first, on_device):
    """pitch 117 (bytes), 120 (dwords, with and without an offset that leaves the base unaligned), 144 and 192 (16 bytes; the last with
    the window starting 48 bytes into the row): w = 37 of a wider parent, so every row has a tail and pitch > 3 w."""
    parent = torch.from_numpy(_images('noise', 2, 53, parent_w, seed=first))
    if on_device:
        parent = parent.cuda()
    x = parent[:, :, first:first + 37]
    assert x.stride(1) == 3 * parent_w > 3 * 37 and not x.is_contiguous()
    _compare(x, 28)


def test_nothing_is_written_outside_the_output():
    """The C ABI on an output in the middle of a guarded buffer, ragged last band, byte and dword stores."""
    from diff_sampler_amd import _lib, _metrics_lib
    from diff_sampler_amd.clip_preprocess import device_tables
    m = _metrics_lib.load()
    for n, h, w, size in ((2, 75, 71, 34), (2, 80, 76, 36)):             # bands of 32 + 2 and 32 + 4 rows
        x = torch.from_numpy(_images('noise', n, h, w)).cuda()
        nh, nw, top, left, (hb, hc, hk, vb, vc, vk) = device_tables(h, w, size, x.device)
        nbytes, guard = n * 3 * size * size, 4096
        buf = torch.full((guard + nbytes + guard,), 0xA5, dtype=torch.uint8, device='cuda')
        assert buf.data_ptr() % 16 == 0
        p = lambda t: C.c_void_p(t.data_ptr())
        rc = m.dsm_resize_crop_u8(p(x), x.stride(0), x.stride(1), n, h, w, nh, nw, top, left, size, p(hb), p(hc), hk, p(vb), p(vc), vk,
                                  C.c_void_p(buf.data_ptr() + guard), _lib.stream_ptr())
        _metrics_lib.check(rc, 'dsm_resize_crop_u8')
        torch.cuda.synchronize()
        assert bool((buf[:guard] == 0xA5).all()) and bool((buf[guard + nbytes:] == 0xA5).all())
        assert torch.equal(buf[guard:guard + nbytes].view(n, 3, size, size).cpu(), _host(x, size))


def test_refused_geometry_raises_naming_it():
    from diff_sampler_amd import _metrics_lib
    from diff_sampler_amd.clip_preprocess import resize_center_crop
    with pytest.raises(_metrics_lib.DsMetricsError, match=r'1 images 2100x2100 -> 28x28.*unsupported shape'):
        resize_center_crop(torch.zeros(1, 2100, 2100, 3, dtype=torch.uint8), 28)        # four staged rows of 6 300 bytes: beyond the LDS envelope
    with pytest.raises(ValueError):
        resize_center_crop(torch.zeros(1, 3, 8, 8, dtype=torch.uint8), 28)              # planar input


# ---------------------------------------------------------------------------------------------------------------- the scorer
def test_score_raw_equals_score_of_preprocess():
    from diff_sampler_amd.clip_score import ClipScorer
    sc = ClipScorer.from_config('tiny_clip_score')
    size = sc.spec.image_size
    raw = torch.from_numpy(_images('noise', 3, 250, 230))
    tokens = torch.tensor([[1, 5, 9, 2] + [0] * 73, [1, 7, 2] + [0] * 74, [1, 3, 4, 6, 2] + [0] * 72])
    want = sc.score(_host(raw, size), tokens).clone()
    want_total = sc.total.clone()
    sc.reset()
    got = sc.score_raw(raw, tokens).clone()
    got_dev = sc.score_raw(raw.cuda(), tokens).clone()
    torch.cuda.synchronize()
    print(f'scores {got.tolist()} / host path {want.tolist()}')
    assert torch.equal(got, want) and torch.equal(got_dev, want) and not bool(torch.isnan(got).any())
    assert float(sc.total) == 2 * float(want_total) and len({round(float(v), 4) for v in got}) == 3


def test_calc_clip_score_device_resize_equals_the_host_path(tmp_path):
    import PIL.Image
    from diff_sampler_amd import clip_score as CS, clip_score_arch as A
    from diff_sampler_amd.clip_tokenizer import ClipTokenizer
    from tests._clip_tok import write_tokenizer
    vocab = write_tokenizer(str(tmp_path / 'tok'))
    spec = A.clip_score_spec(**dict(A.NAMED_CLIP_SCORE_CONFIGS['tiny_clip_score'], vocab=len(vocab)))
    sc = CS.ClipScorer(spec, A.init_clip_score_params(spec, 11), ClipTokenizer(str(tmp_path / 'tok')))
    d = tmp_path / 'images'
    d.mkdir()
    words = ['lower', 'newer hi', 'hi hi lower', 'low', 'new lower newer', 'hi']
    captions = []
    for i in range(12):
        h, w = ((56, 40), (64, 64))[(i // 2) % 2]               # two sizes, mixed inside every batch of 5
        PIL.Image.fromarray(_images('noise', 1, h, w, seed=i)[0], 'RGB').save(d / f'{i:06d}.png')
        captions.append(words[i % 6])
    host = CS.calc_clip_score(sc, str(d), captions, max_batch_size=5, log=lambda *a: None)
    dev = CS.calc_clip_score(sc, str(d), captions, max_batch_size=5, log=lambda *a: None, device_resize=True)
    print(f'host {host}, device resize {dev}')
    assert dev == host and dev[1] == 12 and dev[0] == dev[0]
