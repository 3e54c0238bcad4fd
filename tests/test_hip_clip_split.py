"""GPU: the fp16x3 mode of the CLIP score -- dsm_gemm_split (csrc/metrics/gemm_split.hip) element by element against an fp64 product of the
same fp32 inputs, its row invariance, both towers in ``dtype='fp16x3'`` against the plain-torch fp32 restatement (tests/_clip_vit_ref.py),
the scorer against the goldens, and the command line.

The kernel bound is derived, per element (x: [rows, k], w: [cout, k], fp32):

    |out - ref| <= (2^-20 + k 2^-24) sum_k |x||w|  +  2^-24 sum_k |w_jk|  +  2^-22 |ref|

first term: four times the 3 * 2^-22 representation error of the hi / lo split (hi.hi + hi.lo + lo.hi of 11-bit halves) plus the fp32
accumulation; second: the fp16 subnormal quantum of the activations' lo half for |x| < 2^-3; third: the epilogue's bias / residual
additions.  With an activation 1e-6 of the output's absmax is added (one transcendental, the bound of the row kernels).  Towers: NET_TOL =
2e-4 of the absmax, the project's fp32 network bound.  Every test prints what it achieved before it asserts.

Achieved on the MI355X (profiles/clip_score_fp16x3_parity.json): the largest error / bound over the 64 shapes 0.098, at most 0.008 on N(0, 1)
data with any epilogue, 0.22 with x * 1e-3 (the subnormal term), 0.026 with the x 300 columns, 0.25 with all-zero weights and a residual (the
rounding of bias + res itself); towers: tiny image / text features 1.15e-6 / 1.19e-6, hidden rows 1.14e-6 / 1.17e-6, 2-layer ViT-g-14
1.48e-6 / 1.56e-6 and 1.68e-6 / 1.74e-6 (the CPU emulation of the split predicted 1e-6 to 2e-6); scores within 3.0e-5 of the fp64 goldens;
batch 3 against 2 + 1: text features equal bits, scores within 1.1e-5; the command line's fp16x3 average within 5.2e-7 of its fp32 one."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
G = os.path.join(ROOT, 'tests', 'golden')

pytestmark = pytest.mark.gpu

NET_TOL = 2e-4
GOLDENS = {'tiny_clip_score': 'clip_score_tiny.npz', 'vit_g_14_2l': 'clip_score_vitg2l.npz'}
ROWS, KS, COUTS = (1, 77, 130, 257), (32, 64, 352, 1408), (32, 96, 352, 1056)
ACTS = {'none': 0, 'gelu': 1, 'quick_gelu': 2}


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


@pytest.fixture(scope='module')
def m():
    from diff_sampler_amd import _metrics_lib
    return _metrics_lib.load()


def _stream():
    from diff_sampler_amd import _lib
    return _lib.stream_ptr()


def _inputs(rows, k, cout, data, seed):
    """x ~ N(0, 1), w ~ N(0, 0.03^2), bias and residual ~ N(0, 1); `data` picks the variant."""
    g = torch.Generator().manual_seed(seed)
    x, w = torch.randn(rows, k, generator=g), torch.randn(cout, k, generator=g) * 0.03
    bias, res = torch.randn(cout, generator=g), torch.randn(rows, cout, generator=g)
    if data == 'small':
        x = x * 1e-3
    elif data == 'spikes':
        x[:, ::97] *= 300.0
    elif data == 'zero_w':
        w = torch.zeros_like(w)
    else:
        assert data == 'normal'
    return x, w, bias, res


def _run(m, x, w, bias=None, res=None, act='none', pad=8, extra_rows=2):
    """One dsm_gemm_split call on padded operands (ldx = k + pad, out_ld = cout + pad, NaN in every pad column and in `extra_rows` rows behind
    the output) -> the [rows, cout + pad] device result, after checking that nothing outside [rows, cout] was written."""
    from diff_sampler_amd import _metrics_lib
    from diff_sampler_amd.ops import pack_linear_weight_split
    rows, k = x.shape
    cout = w.shape[0]
    packed, shift = pack_linear_weight_split(w)
    xd = torch.full((rows, k + pad), float('nan'))
    xd[:, :k] = x
    xd, wd = xd.cuda(), packed.cuda()
    bd = None if bias is None else bias.cuda()
    rd = None
    if res is not None:
        rd = torch.full((rows, cout + pad), float('nan'))
        rd[:, :cout] = res
        rd = rd.cuda()
    out = torch.full((rows + extra_rows, cout + pad), float('nan'), device='cuda')
    a = _metrics_lib.DsmGemmSplitArgs(_p(xd), k + pad, rows, k, _p(wd), shift, cout, _p(bd), _p(rd), cout + pad if rd is not None else 0, ACTS[act],
                                      _p(out), cout + pad)
    _metrics_lib.check(m.dsm_gemm_split(C.byref(a), _stream()), 'dsm_gemm_split')
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[:rows, cout:]).all()) and bool(torch.isnan(out[rows:]).all())          # columns [cout, out_ld) and rows beyond: untouched
    assert torch.equal(xd[:, :k].cpu(), x)                                                              # the operands are read only
    return out[:rows]


def _check(out, x, w, bias, res, act, what):
    """The derived bound, per element, against the fp64 evaluation of the same fp32 inputs."""
    rows, k = x.shape
    cout = w.shape[0]
    x64, w64 = x.double(), w.double()
    ref = x64 @ w64.t()
    if bias is not None:
        ref = ref + bias.double()
    if act == 'gelu':
        ref = F.gelu(ref)
    elif act == 'quick_gelu':
        ref = ref * torch.sigmoid(1.702 * ref)
    if res is not None:
        ref = ref + res.double()
    bound = (2.0 ** -20 + k * 2.0 ** -24) * (x64.abs() @ w64.abs().t()) + 2.0 ** -24 * w64.abs().sum(1)[None, :] + 2.0 ** -22 * ref.abs()
    if act != 'none':
        bound = bound + 1e-6 * float(ref.abs().max())
    got = out[:, :cout].double().cpu()
    assert bool(torch.isfinite(got).all()), what
    err = (got - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max()) if float(bound.max()) > 0 else 0.0
    print(f'dsm_gemm_split {what}: max |error| {float(err.max()):.3e}, of absmax {float(err.max() / ref.abs().max().clamp_min(1e-30)):.2e}, '
          f'largest error / bound {ratio:.3f}')
    assert bool((err <= bound).all()), what
    return ratio


# ---------------------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize('cout', COUTS)
@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('rows', ROWS)
def test_gemm_split_every_shape_against_fp64(m, rows, k, cout):
    """Every combination of the row counts (one row, below / just above one 128-row tile, two tiles and one row), K (one and two 32-column
    steps, 11 and 44 steps) and output widths (a quarter tile, 96, 2.75 and 8.25 tiles), with a bias, ldx > k and out_ld > cout."""
    x, w, bias, _ = _inputs(rows, k, cout, 'normal', 1000 * rows + k + cout)
    out = _run(m, x, w, bias=bias)
    _check(out, x, w, bias, None, 'none', f'{rows}x{k}->{cout}')


@pytest.mark.parametrize('epi', ['plain', 'bias', 'res', 'gelu', 'quick_gelu'])
@pytest.mark.parametrize('data', ['normal', 'small', 'spikes', 'zero_w'])
@pytest.mark.parametrize('rows,k,cout', [(77, 352, 96), (257, 1408, 1056)])
def test_gemm_split_data_and_epilogues(m, rows, k, cout, data, epi):
    x, w, bias, res = _inputs(rows, k, cout, data, 7 * rows + k)
    bias = None if epi == 'plain' else bias
    res = res if epi == 'res' else None
    act = epi if epi in ('gelu', 'quick_gelu') else 'none'
    out = _run(m, x, w, bias=bias, res=res, act=act)
    _check(out, x, w, bias, res, act, f'{rows}x{k}->{cout} {data} {epi}')
    if data == 'zero_w' and act == 'none':                                        # 0 * 2^-shift + bias + res: no arithmetic error at all
        want = torch.zeros(rows, cout) + (bias if bias is not None else 0.0) + (res if res is not None else 0.0)
        assert torch.equal(out[:, :cout].cpu(), want)


def test_gemm_split_row_invariance(m):
    """No split-K, a fixed K order: the first 130 rows of a 257-row call are the 130-row call bit for bit (other tile, other position in the
    grid), with the bias and the residual in the epilogue; a second call gives the same bits."""
    x, w, bias, res = _inputs(257, 1408, 1056, 'normal', 5)
    full = _run(m, x, w, bias=bias, res=res)
    part = _run(m, x[:130].contiguous(), w, bias=bias, res=res[:130].contiguous())
    one = _run(m, x[129:130].contiguous(), w, bias=bias, res=res[129:130].contiguous())
    assert torch.equal(full[:130, :1056], part[:, :1056]) and torch.equal(full[129:130, :1056], one[:, :1056])
    assert torch.equal(_run(m, x, w, bias=bias, res=res)[:, :1056], full[:, :1056])
    for act in ('gelu', 'quick_gelu'):
        assert torch.equal(_run(m, x, w, bias=bias, act=act)[:130, :1056], _run(m, x[:130].contiguous(), w, bias=bias, act=act)[:, :1056])


# ---------------------------------------------------------------------------------------------------------------- towers
@pytest.fixture(scope='module')
def cases():
    """golden name -> (npz, spec, params of seed 0, three uint8 images, three prompts' tokens, fp32 restatement of both towers on them): computed
    once, shared, never modified."""
    from diff_sampler_amd import clip_score_arch as A
    from tests import _clip_vit_ref as R
    out = {}
    for name, f in GOLDENS.items():
        z = np.load(os.path.join(G, f))
        spec = A.named_spec(name)
        params = A.init_clip_score_params(spec, 0)
        images = R.seed_images(int(z['image_seed']), 3, spec.image_size)
        tok = torch.from_numpy(z['tokens'])
        tokens = tok[torch.arange(3) % tok.shape[0]].contiguous()
        with torch.no_grad():
            ri = R.clip_image_ref(params, images, spec.vision.heads, spec.vision.layers, spec.eps, spec.act)
            rt = R.clip_text_pooled_ref(params, tokens, spec.text.heads, spec.text.layers, spec.eps, spec.act)
        out[name] = (z, spec, params, images, tokens, ri, rt)
    return out


def _of_absmax(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize('name', list(GOLDENS))
def test_fp16x3_towers_against_the_fp32_restatement(cases, name):
    """Features and the last layer's hidden rows (ALL rows) of both towers at batch 3, of the restatement's absmax.  The CPU emulation of
    the split predicts 1e-6 to 2e-6 -- what the fp32 engine achieves."""
    from diff_sampler_amd.clip_score_engine import ClipImageEncoder, ClipPooledTextEncoder
    z, spec, params, images, tokens, (rfi, rvh), (rft, rth) = cases[name]
    fi, plan = ClipImageEncoder(spec, params, dtype='fp16x3').raw(images)
    torch.cuda.synchronize()
    e_fi, e_vh = _of_absmax(fi, rfi), _of_absmax(plan.bufs['hidden'].view(rvh.shape), rvh)
    ft, plan = ClipPooledTextEncoder(spec, params, dtype='fp16x3').raw(tokens)
    torch.cuda.synchronize()
    e_ft, e_th = _of_absmax(ft, rft), _of_absmax(plan.bufs['hidden'].view(rth.shape), rth)
    print(f'fp16x3 {name}: image features {e_fi:.2e}, vision hidden rows {e_vh:.2e}, text features {e_ft:.2e}, text hidden rows {e_th:.2e} of absmax')
    assert bool(torch.isfinite(fi).all() & torch.isfinite(ft).all())
    assert e_fi < NET_TOL and e_ft < NET_TOL and e_vh < NET_TOL and e_th < NET_TOL


@pytest.mark.parametrize('name', list(GOLDENS))
def test_fp16x3_scorer_against_the_goldens(cases, name):
    """The goldens' own images, prompts and weights (their recorded seed): scores within twice the recorded first-order bound."""
    from diff_sampler_amd import clip_score_arch as A
    from diff_sampler_amd.clip_score import ClipScorer
    from tests._clip_vit_ref import seed_images
    z, spec = cases[name][0], cases[name][1]
    tokens = torch.from_numpy(z['tokens'])
    images = seed_images(int(z['image_seed']), tokens.shape[0], spec.image_size)
    sc = ClipScorer(spec, A.init_clip_score_params(spec, int(z['seed'])), dtype='fp16x3')
    s = sc.score(images, tokens)
    torch.cuda.synchronize()
    err = (s.double().cpu() - torch.from_numpy(z['scores'])).abs()
    print(f'fp16x3 {name}: scores {s.cpu().tolist()} golden {z["scores"].tolist()} |error| {err.tolist()} bound {(2 * z["score_bound"]).tolist()}')
    assert bool((err <= 2 * torch.from_numpy(z['score_bound'])).all())
    assert abs(float(sc.total) - float(s.double().sum())) <= 1e-12 * abs(float(s.double().sum()))


def test_fp16x3_scorer_batch_of_three_as_two_plus_one(cases):
    """dsm_gemm_split is row invariant; the fp32 launches around it decide whether the batch is.  Text tower: every launch is, so the
    features of a batch of 3 are those of 2 + 1 BIT FOR BIT.  Image tower: one launch is not -- `patch_embedding` (ds_conv2d_nhwc, taps = 1:
    it picks its split-K factor from the number of output tiles, i.e. from the row count, 768 against 512 rows here); every launch behind it
    gave equal bits on equal inputs (measured launch by launch on the MI355X).  So the scores get the fp32 test's rule: both evaluations lie
    within the first-order bound 100 eps sqrt(E) (max|a| / |a| + max|b| / |b|), eps = NET_TOL, of the exact score, and differ by at most
    twice that.  Achieved: at most 1.1e-5, as in fp32 mode."""
    from diff_sampler_amd.clip_score import ClipScorer
    z, spec, params, images, tokens = cases['tiny_clip_score'][:5]
    sc = ClipScorer(spec, params, dtype='fp16x3')
    t3 = sc.text(tokens)
    t21 = torch.cat([sc.text(tokens[:2]), sc.text(tokens[2:])])
    i3 = sc.image(images)
    i21 = torch.cat([sc.image(images[:2]), sc.image(images[2:])])
    s3 = sc.score(images, tokens).clone()
    s21 = torch.cat([sc.score(images[:2], tokens[:2]).clone(), sc.score(images[2:], tokens[2:]).clone()])
    torch.cuda.synchronize()
    ratio = lambda f: (f.abs().max(-1).values / f.norm(dim=-1)).double().cpu()
    bound = 100.0 * NET_TOL * spec.embed ** 0.5 * (ratio(i3) + ratio(t3))
    d = (s3.double() - s21.double()).abs().cpu()
    print(f'fp16x3 3 vs 2 + 1: scores {d.tolist()} (bound {(2 * bound).tolist()}), image features {_of_absmax(i21, i3):.2e} of absmax, '
          f'text features equal bits: {torch.equal(t3, t21)}')
    assert not bool(torch.isnan(s3).any() | torch.isnan(s21).any())
    assert torch.equal(t3, t21)
    assert _of_absmax(i21, i3) < NET_TOL and bool((d <= 2 * bound).all())


def test_scorer_names_the_operand_range_when_features_are_not_finite(cases):
    """An activation beyond 65504 has an infinite hi half: the scorer refuses the batch and says what to do."""
    from diff_sampler_amd.clip_score import ClipScorer
    z, spec, params, images, tokens = cases['tiny_clip_score'][:5]
    big = dict(params)
    key = 'vision_model.encoder.layers.0.layer_norm1.weight'                     # the input of the first q | k | v projection
    big[key] = params[key] * 1e6
    sc = ClipScorer(spec, big, dtype='fp16x3')
    with pytest.raises(FloatingPointError, match=r'65504.*--dtype fp32'):
        sc.score(images, tokens)


# ---------------------------------------------------------------------------------------------------------------- command line
def test_cli_dtype_fp16x3(tmp_path, monkeypatch):
    """The folder of tests/test_hip_clip_score.py::test_cli_equals_the_api, scored by the command line in both modes.  Either run is within
    NET_TOL * absmax per feature element of the exact features, i.e. its average within the mean of the goldens' first-order bound
    100 eps sqrt(E) (max|a| / |a| + max|b| / |b|) of the exact average: the two differ by at most twice that."""
    import PIL.Image
    from click.testing import CliRunner
    from diff_sampler_amd import clip_score as CS, clip_score_arch as A
    from diff_sampler_amd.clip_tokenizer import ClipTokenizer
    from tests._clip_tok import write_tokenizer
    from tests._clip_vit_ref import seed_images
    vocab = write_tokenizer(str(tmp_path / 'tok'))
    spec = A.clip_score_spec(**dict(A.NAMED_CLIP_SCORE_CONFIGS['tiny_clip_score'], vocab=len(vocab)))
    params = A.init_clip_score_params(spec, 11)
    torch.save(A.to_open_clip(spec, params), str(tmp_path / 'clip.pt'))
    imgs = seed_images(12, 5)
    d = tmp_path / 'run' / 'images'
    d.mkdir(parents=True)
    for i, a in enumerate(imgs):
        PIL.Image.fromarray(a.permute(1, 2, 0).numpy(), 'RGB').save(d / f'{i:06d}.png')
    prompts = ['lower', 'newer hi', 'hi hi lower', 'low', 'new lower newer']
    with open(tmp_path / 'c.csv', 'w') as fh:
        fh.write('text\n' + ''.join(p + '\n' for p in prompts))
    sc = CS.ClipScorer(spec, params, ClipTokenizer(str(tmp_path / 'tok')))
    fi, ft = sc.image(imgs).double().cpu(), sc.text(sc.tokens(prompts)).double().cpu()
    ratio = lambda f: f.abs().max(-1).values / f.norm(dim=-1)
    bound = float((100.0 * NET_TOL * spec.embed ** 0.5 * (ratio(fi) + ratio(ft))).mean())
    monkeypatch.chdir(tmp_path)
    got = {}
    for dtype in ('fp32', 'fp16x3'):
        args = ['calc', '--images', str(d), '--prompts', str(tmp_path / 'c.csv'), '--model', str(tmp_path / 'clip.pt'), '--tokenizer_path',
                str(tmp_path / 'tok'), '--batch', '2', '--dtype', dtype]
        r = CliRunner().invoke(CS.main, args)
        assert r.exit_code == 0, r.output
        last = r.output.splitlines()[-1]
        assert last.startswith('CLIP score: ')
        got[dtype] = last[len('CLIP score: '):]
    lines = open(tmp_path / 'clip_score.txt').read().splitlines()
    assert lines == [f'run images {got["fp32"]}', f'run images {got["fp16x3"]}']                      # the same line format, one line per run
    diff = abs(float(got['fp16x3']) - float(got['fp32']))
    print(f'calc --dtype fp16x3 {got["fp16x3"]} vs fp32 {got["fp32"]}: |difference| {diff:.3e} (bound {2 * bound:.3e})')
    assert diff <= 2 * bound
