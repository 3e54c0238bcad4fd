"""GPU: the CLIP-score kernels of csrc/metrics/clip_score.hip element by element, both towers against the goldens recorded from
transformers' CLIPModel (tools/gen_clip_score_golden.py), the scorer and the command line.

Bounds: ATTN_TOL = 2e-5 (the project's fp32 attention bound), NET_TOL = 2e-4 of the output absmax (its fp32 network goldens), 1e-6 of
max |y| for a row kernel with one transcendental.

Achieved on the MI355X (profiles/clip_score_parity.json; every test prints its values before it asserts): dsm_attention at d = 88 at most
9.0e-7 (sq = 257), dsm_gelu_rows 3.7e-8, dsm_vit_patch_rows 1.3e-7, dsm_clip_score 1.2e-5 absolute (bound 7.6e-4 at dim 64); towers: tiny
image / text features 8.8e-7 / 9.2e-7, hidden rows 7.9e-7 / 5.4e-7; 2-layer ViT-g-14 1.4e-6 / 1.1e-6, hidden rows 1.2e-6 / 9.0e-7; scores within
4.9e-5 of the fp64 goldens (bounds 0.09 - 0.15); a batch of 3 against 2 + 1 within 1.1e-5."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
G = os.path.join(ROOT, 'tests', 'golden')

pytestmark = pytest.mark.gpu

ATTN_TOL = 2e-5
NET_TOL = 2e-4
GOLDENS = {'tiny_clip_score': 'clip_score_tiny.npz', 'vit_g_14_2l': 'clip_score_vitg2l.npz'}


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


def _p(t):
    return C.c_void_p(t.data_ptr())


@pytest.fixture(scope='module')
def m():
    from diff_sampler_amd import _metrics_lib
    return _metrics_lib.load()


def _check(rc, what=''):
    from diff_sampler_amd import _metrics_lib
    _metrics_lib.check(rc, what)


def _stream():
    from diff_sampler_amd import _lib
    return _lib.stream_ptr()


# ---------------------------------------------------------------------------------------------------------------- dsm_attention
B_, H_, D_ = 2, 4, 88
W_ = H_ * D_
LD_ = 3 * W_ + 8


def _packed(sq, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B_ * sq, LD_, generator=g)
    qkv[:, W_:2 * W_] *= 1.5                                    # K scaled: the softmax is not flat
    return qkv


def _attn_ref(qkv, sq):
    x = qkv.double().view(B_, sq, LD_)
    q, k, v = (x[:, :, i * W_:(i + 1) * W_].reshape(B_, sq, H_, D_).transpose(1, 2) for i in range(3))
    a = torch.softmax(q @ k.transpose(-1, -2) * D_ ** -0.5, dim=-1) @ v
    return a.transpose(1, 2).reshape(B_ * sq, W_)


def _run_attn(m, qkv_dev, sq, out=None):
    from diff_sampler_amd._metrics_lib import DsmAttnArgs
    if out is None:
        out = torch.full((B_ * sq, W_ + 8), float('nan'), device='cuda')
    a = DsmAttnArgs(_p(qkv_dev), C.c_void_p(qkv_dev.data_ptr() + 4 * W_), C.c_void_p(qkv_dev.data_ptr() + 8 * W_), _p(out), LD_, LD_, LD_, W_ + 8,
                    sq * LD_, sq * LD_, sq * LD_, sq * (W_ + 8), B_, H_, sq, sq, D_, D_ ** -0.5)
    _check(m.dsm_attention(C.byref(a), _stream()), 'dsm_attention')
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('sq', [1, 31, 32, 33, 129, 257])
def test_attention_d88_against_fp64(m, sq):
    qkv = _packed(sq, 100 + sq)
    dev = qkv.cuda()
    out = _run_attn(m, dev, sq)
    assert not bool(torch.isnan(out[:, :W_]).any()) and bool(torch.isnan(out[:, W_:]).all())       # the 8 pad columns are not written
    err = _rel(out[:, :W_], _attn_ref(qkv, sq))
    print(f'dsm_attention d=88 sq={sq}: {err:.2e}')
    assert err < ATTN_TOL
    assert torch.equal(dev.cpu(), qkv)                                                              # the operands are read only
    if sq == 1:
        assert _rel(out[:, :W_], qkv[:, 2 * W_:3 * W_]) < 1e-6                                      # one key: the output is v
    if sq == 257:
        again = _run_attn(m, dev, sq)
        assert torch.equal(again[:, :W_], out[:, :W_])                                              # same bits on a second call


def test_attention_d88_never_uses_keys_beyond_skv(m):
    """The packed tensor is a view into a longer buffer whose following rows are NaN: same bits as on its own, all finite."""
    sq = 33
    qkv = _packed(sq, 7)
    alone = _run_attn(m, qkv.cuda(), sq)
    longer = torch.full((B_ * sq + 64, LD_), float('nan'))
    longer[:B_ * sq] = qkv
    dev = longer.cuda()
    out = _run_attn(m, dev[:B_ * sq], sq)
    assert bool(torch.isfinite(out[:, :W_]).all()) and torch.equal(out[:, :W_], alone[:, :W_])
    assert _rel(out[:, :W_], _attn_ref(qkv, sq)) < ATTN_TOL


# ---------------------------------------------------------------------------------------------------------------- row kernels
@pytest.mark.parametrize('rows,cols,ld', [(231, 1536, 1544), (1, 4, 4)])
def test_gelu_rows(m, rows, cols, ld):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(rows, ld, generator=g) * 2.5
    x.view(-1)[:4] = torch.tensor([0.0, -60.0, -20.0, 6.0])
    dev = x.cuda()
    y = torch.full((rows, ld), float('nan'), device='cuda')
    _check(m.dsm_gelu_rows(_p(dev), ld, _p(y), ld, rows, cols, _stream()))
    torch.cuda.synchronize()
    xd = x[:, :cols].double()
    want = 0.5 * xd * (1.0 + torch.erf(xd / 2 ** 0.5))
    err = float((y[:, :cols].double().cpu() - want).abs().max() / want.abs().max())
    print(f'dsm_gelu_rows {rows}x{cols}: {err:.2e} of max |y|')
    assert err <= 1e-6
    assert bool(torch.isnan(y[:, cols:]).all())                                  # pad columns untouched
    assert float(y.view(-1)[0]) == 0.0 and float(y.view(-1)[1]) == 0.0 and float(y.view(-1)[2]) == 0.0
    _check(m.dsm_gelu_rows(_p(dev), ld, _p(dev), ld, rows, cols, _stream()))     # in place: equal bits, pad columns still the input's
    torch.cuda.synchronize()
    assert torch.equal(dev[:, :cols], y[:, :cols]) and torch.equal(dev[:, cols:].cpu(), x[:, cols:])


def _unfold(x, P):
    """[N, 3, S, S] -> [N * (S / P)^2, 3 P^2], column order (channel, py, px)."""
    N, Cc, S, _ = x.shape
    g = S // P
    return x.view(N, Cc, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(N * g * g, Cc * P * P)


@pytest.mark.parametrize('S', [28, 224])
def test_vit_patch_rows(m, S):
    from diff_sampler_amd.clip_score_arch import CLIP_MEAN, CLIP_STD
    N, P, ld = 2, 14, 608
    g = torch.Generator().manual_seed(S)
    u8 = torch.randint(0, 256, (N, 3, S, S), generator=g, dtype=torch.uint8)
    rows = N * (S // P) ** 2
    zero, one = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    mean, std = (C.c_float * 3)(*CLIP_MEAN), (C.c_float * 3)(*CLIP_STD)

    def run(img, f32, mu, sd):
        out = torch.full((rows, ld), float('nan'), device='cuda')
        _check(m.dsm_vit_patch_rows(_p(img), f32, N, S, P, mu, sd, _p(out), ld, _stream()))
        torch.cuda.synchronize()
        assert bool((out[:, 588:] == 0).all())                                   # columns [588, ld) are exactly 0
        return out[:, :588].cpu()

    # layout: integer-valued fp32 input, mean 0, std 1 -> exactly the unfolded image
    f = u8.float()
    assert torch.equal(run(f.cuda(), 1, zero, one), _unfold(f, P))
    assert torch.equal(run(u8.cuda(), 0, zero, one), _unfold(f / 255.0, P))       # uint8: one division by 255
    # values: the CLIP mean / std against fp64
    mu64, sd64 = torch.tensor(CLIP_MEAN, dtype=torch.float64).view(1, 3, 1, 1), torch.tensor(CLIP_STD, dtype=torch.float64).view(1, 3, 1, 1)
    want = _unfold((u8.double() / 255.0 - mu64) / sd64, P)
    for img, f32 in ((u8.cuda(), 0), ((f / 255.0).cuda(), 1)):
        got = run(img, f32, mean, std)
        err = float((got.double() - want).abs().max() / want.abs().max())
        print(f'dsm_vit_patch_rows S={S} f32={f32}: {err:.2e} of max')
        assert err <= 1e-6


def test_vit_tokens_and_gather_rows(m):
    g = torch.Generator().manual_seed(9)
    N, T, W, ld = 3, 5, 352, 360
    pe, cls, pos = torch.randn(N * (T - 1), ld, generator=g), torch.randn(W, generator=g), torch.randn(T, W, generator=g)
    out = torch.full((N * T, ld), float('nan'), device='cuda')
    ped, clsd, posd = pe.cuda(), cls.cuda(), pos.cuda()                          # (named: a temporary's memory is free for the next allocation)
    _check(m.dsm_vit_tokens(_p(ped), ld, _p(clsd), _p(posd), _p(out), ld, N, T, W, _stream()))
    torch.cuda.synchronize()
    want = torch.cat([cls.expand(N, 1, W), pe[:, :W].view(N, T - 1, W)], 1) + pos
    assert torch.equal(out[:, :W].cpu(), want.reshape(N * T, W)) and bool(torch.isnan(out[:, W:]).all())

    x = torch.randn(N * T, ld, generator=g)
    idx = torch.tensor([0, N * T - 1, 7, 7, 0, 3], dtype=torch.int32)            # first, last, repeated
    got = torch.full((len(idx), W + 4), float('nan'), device='cuda')
    xd, idxd = x.cuda(), idx.cuda()
    _check(m.dsm_gather_rows(_p(xd), ld, N * T, _p(idxd), _p(got), W + 4, len(idx), W, _stream()))
    torch.cuda.synchronize()
    assert torch.equal(got[:, :W].cpu(), x[idx.long(), :W]) and bool(torch.isnan(got[:, W:]).all())


@pytest.mark.parametrize('dim', [64, 1024])
@pytest.mark.parametrize('n', [1, 5, 64])
def test_clip_score_kernel(m, n, dim):
    g = torch.Generator().manual_seed(n * dim)
    ld = dim + 8
    a, b = torch.randn(n, ld, generator=g), torch.randn(n, ld, generator=g)
    b[:, :dim] += 0.5 * a[:, :dim]                                              # correlated: scores away from 0
    a[:, dim:], b[:, dim:] = float('nan'), float('nan')                          # the pad columns are not read
    ad, bd = a.cuda(), b.cuda()

    def run(total):
        s = torch.full((n,), float('nan'), device='cuda')
        _check(m.dsm_clip_score(_p(ad), ld, _p(bd), ld, n, dim, _p(s), _p(total), _stream()))
        torch.cuda.synchronize()
        return s

    t1 = torch.zeros(1, dtype=torch.float64, device='cuda')
    s1 = run(t1)
    a64, b64 = a[:, :dim].double(), b[:, :dim].double()
    want = 100.0 * (a64 * b64).sum(-1) / (a64.norm(dim=-1) * b64.norm(dim=-1))
    err = float((s1.double().cpu() - want).abs().max())
    print(f'dsm_clip_score n={n} dim={dim}: max |error| {err:.2e} (bound {100 * 2 * dim * 2.0 ** -24:.2e})')
    assert err <= 100 * 2 * dim * 2.0 ** -24
    tot = float(s1.double().sum())
    assert abs(float(t1) - tot) <= 1e-12 * abs(tot)
    first = float(t1)
    run(t1)                                                                      # a second call accumulates
    assert abs(float(t1) - 2 * tot) <= 1e-12 * abs(2 * tot) and float(t1) != first
    t2 = torch.zeros(1, dtype=torch.float64, device='cuda')
    s2 = run(t2)                                                                 # a fresh run: equal bits
    assert torch.equal(s1, s2) and float(t2) == first


# ---------------------------------------------------------------------------------------------------------------- towers
@pytest.fixture(scope='module')
def cases():
    """golden name -> (npz, spec, params, uint8 images), shared by the tower and scorer tests."""
    from diff_sampler_amd import clip_score_arch as A
    from tests._clip_vit_ref import seed_images
    out = {}
    for name, f in GOLDENS.items():
        z = np.load(os.path.join(G, f))
        spec = A.named_spec(name)
        out[name] = (z, spec, A.init_clip_score_params(spec, int(z['seed'])), seed_images(int(z['image_seed']), z['tokens'].shape[0], spec.image_size))
    return out


@pytest.mark.parametrize('name', list(GOLDENS))
def test_towers_against_the_goldens(cases, name):
    """Achieved (MI355X, profiles/clip_score_parity.json): tiny 8.8e-7 / 7.9e-7 / 9.2e-7 / 5.4e-7, 2-layer ViT-g-14 1.4e-6 / 1.2e-6 / 1.1e-6 / 9.0e-7
    (image features / vision hidden rows / text features / text hidden rows, of the recorded absmax)."""
    from diff_sampler_amd.clip_score_engine import ClipImageEncoder, ClipPooledTextEncoder
    z, spec, params, images = cases[name]
    B = images.shape[0]
    fi, plan = ClipImageEncoder(spec, params).raw(images)
    torch.cuda.synchronize()
    vh = plan.bufs['hidden'].view(B, spec.vision_tokens, -1)[:, z['vision_rows'].tolist()].cpu()
    e_fi = float((fi.cpu() - torch.from_numpy(z['image_features'])).abs().max()) / float(z['image_absmax'])
    e_vh = float((vh - torch.from_numpy(z['vision_hidden'])).abs().max()) / float(z['vision_hidden_absmax'])
    ft, plan = ClipPooledTextEncoder(spec, params).raw(torch.from_numpy(z['tokens']))
    torch.cuda.synchronize()
    th = plan.bufs['hidden'].view(B, spec.positions, -1).cpu()
    tr = torch.from_numpy(z['text_rows'])
    th = torch.stack([th[b, tr[b]] for b in range(B)])
    e_ft = float((ft.cpu() - torch.from_numpy(z['text_features'])).abs().max()) / float(z['text_absmax'])
    e_th = float((th - torch.from_numpy(z['text_hidden'])).abs().max()) / float(z['text_hidden_absmax'])
    print(f'{name}: image features {e_fi:.2e}, vision hidden rows {e_vh:.2e}, text features {e_ft:.2e}, text hidden rows {e_th:.2e} of absmax')
    assert not bool(torch.isnan(fi).any() | torch.isnan(ft).any())
    assert e_fi < NET_TOL and e_ft < NET_TOL and e_vh < NET_TOL and e_th < NET_TOL


def test_image_tower_against_the_restatement_in_fp32_input_form(cases):
    """fp32 images in [0, 1] take the same plan shape as uint8 ones (one division less): same features to NET_TOL."""
    from diff_sampler_amd.clip_score_engine import ClipImageEncoder
    z, spec, params, images = cases['tiny_clip_score']
    enc = ClipImageEncoder(spec, params)
    a, b = enc(images), enc(images.float() / 255.0)
    assert _rel(b, a) < NET_TOL and _rel(a, torch.from_numpy(z['image_features'])) < NET_TOL


# ---------------------------------------------------------------------------------------------------------------- scorer, command line
@pytest.mark.parametrize('name', list(GOLDENS))
def test_scorer_against_the_goldens(cases, name):
    from diff_sampler_amd.clip_score import ClipScorer
    z, spec, params, images = cases[name]
    sc = ClipScorer(spec, params)
    s = sc.score(images, torch.from_numpy(z['tokens']))
    torch.cuda.synchronize()
    err = (s.double().cpu() - torch.from_numpy(z['scores'])).abs()
    print(f'{name}: scores {s.cpu().tolist()} golden {z["scores"].tolist()} |error| {err.tolist()} bound {z["score_bound"].tolist()}')
    assert bool((err <= torch.from_numpy(z['score_bound'])).all())
    assert abs(float(sc.total) - float(s.double().sum())) <= 1e-12 * abs(float(s.double().sum()))


def test_scorer_batch_of_three_as_two_plus_one(cases):
    """Both evaluations are within NET_TOL * absmax per feature element of the exact features, i.e. within `score_bound` of the exact score
    each: they differ by at most twice that."""
    from diff_sampler_amd.clip_score import ClipScorer
    z, spec, params, images = cases['tiny_clip_score']
    t = torch.from_numpy(z['tokens'])
    sc = ClipScorer(spec, params)
    s3 = sc.score(images, t).clone()
    s21 = torch.cat([sc.score(images[:2], t[:2]).clone(), sc.score(images[2:], t[2:]).clone()])
    torch.cuda.synchronize()
    d = (s3.double() - s21.double()).abs().cpu()
    print(f'3 vs 2 + 1: {d.tolist()} (bound {(2 * z["score_bound"]).tolist()})')
    assert not bool(torch.isnan(s3).any() | torch.isnan(s21).any())
    assert bool((d <= 2 * torch.from_numpy(z['score_bound'])).all())
    assert abs(float(sc.total) - float(s3.double().sum() + s21.double().sum())) <= 1e-9


def test_cli_equals_the_api(tmp_path, monkeypatch):
    import PIL.Image
    from click.testing import CliRunner
    from diff_sampler_amd import clip_score as CS, clip_score_arch as A, fid
    from diff_sampler_amd.clip_tokenizer import ClipTokenizer
    from tests._clip_tok import write_tokenizer
    from tests._clip_vit_ref import seed_images
    vocab = write_tokenizer(str(tmp_path / 'tok'))
    spec = A.clip_score_spec(**dict(A.NAMED_CLIP_SCORE_CONFIGS['tiny_clip_score'], vocab=len(vocab)))
    params = A.init_clip_score_params(spec, 11)
    torch.save(A.to_open_clip(spec, params), str(tmp_path / 'clip.pt'))                  # the reference checkpoint's layout
    imgs = seed_images(12, 5)
    d = tmp_path / 'run' / 'images'
    d.mkdir(parents=True)
    for i, a in enumerate(imgs):
        PIL.Image.fromarray(a.permute(1, 2, 0).numpy(), 'RGB').save(d / f'{i:06d}.png')
    prompts = ['lower', 'newer hi', 'hi hi lower', 'low', 'new lower newer']
    with open(tmp_path / 'c.csv', 'w') as fh:
        fh.write('text\n' + ''.join(p + '\n' for p in prompts))
    # the API on the batches the command line forms (--batch 2 over 5 images: ragged)
    sc = CS.ClipScorer(spec, params, ClipTokenizer(str(tmp_path / 'tok')))
    per = []
    for idx in fid.shard_items(5, 2, 0, 1):
        per.append(sc.score(imgs[idx], [prompts[i] for i in idx.tolist()]).clone())
    want = float(sc.total) / 5
    assert sorted(len(b) for b in fid.shard_items(5, 2, 0, 1)) == [1, 2, 2]
    assert abs(want - float(torch.cat(per).double().mean())) <= 1e-12 * abs(want) and len({round(float(v), 3) for v in torch.cat(per)}) == 5
    monkeypatch.chdir(tmp_path)
    args = ['calc', '--images', str(d), '--prompts', str(tmp_path / 'c.csv'), '--model', str(tmp_path / 'clip.pt'), '--tokenizer_path',
            str(tmp_path / 'tok'), '--batch', '2']
    r = CliRunner().invoke(CS.main, args)
    assert r.exit_code == 0, r.output
    assert r.output.splitlines()[-1] == f'CLIP score: {want}'
    assert open(tmp_path / 'clip_score.txt').read() == f'run images {want}\n'            # one line appended
