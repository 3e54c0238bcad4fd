"""GPU: the CLIP text encoder (diff_sampler_amd/clip_engine.py) and the three kernels it added (csrc/text_encoder.hip): the token +
position embedding, quick_gelu and the causal self-attention.  Goldens come from the real class (tools/gen_clip_golden.py); nothing here
reads the reference tree."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
G = os.path.join(ROOT, 'tests', 'golden')

pytestmark = pytest.mark.gpu

ATTN_TOL = 2e-5          # the bound of the fp32 attention test in tests/test_hip_kernels.py (TOL)
NET_TOL = 2e-4           # the bound of the project's fp32 network goldens (tests/test_hip_vae.py)


def _rel(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


def _p(t):
    return C.c_void_p(t.data_ptr())


# ---------------------------------------------------------------------------------------------------------------- kernels
def test_token_embed_is_a_gather_and_one_add():
    from diff_sampler_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(1)
    V, W, B, S, ld = 512, 128, 3, 77, 136
    tok, pos = torch.randn(V, W, generator=g).cuda(), torch.randn(S, W, generator=g).cuda()
    ids = torch.randint(0, V, (B, S), generator=g)
    ids[0, 0], ids[1, 5], ids[2, 76] = 0, 511, 511
    idd = ids.to(torch.int32).cuda()
    out = torch.full((B * S, ld), float('nan'), device='cuda')
    _lib.check(lib.ds_token_embed(_p(idd), _p(tok), _p(pos), _p(out), ld, B, S, W, V, _lib.stream_ptr()))
    torch.cuda.synchronize()
    want = (tok[ids.cuda()] + pos[None]).reshape(B * S, W)
    assert torch.equal(out[:, :W], want)
    assert bool(torch.isnan(out[:, W:]).all())               # the pad columns are not written
    # ids outside the table are clamped by the kernel (the host refuses them first: tests/test_clip_cpu.py)
    bad = idd.clone()
    bad[0, 1], bad[0, 2] = -7, 9999
    _lib.check(lib.ds_token_embed(_p(bad), _p(tok), _p(pos), _p(out), ld, B, S, W, V, _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(out[1, :W], tok[0] + pos[1]) and torch.equal(out[2, :W], tok[511] + pos[2])


@pytest.mark.parametrize('rows,cols,ld', [(231, 512, 520), (1, 4, 4)])
def test_quick_gelu(rows, cols, ld):
    """x * sigmoid(1.702 x) against fp64: 1e-6 of max |y| -- a handful of fp32 roundings of one exp, one reciprocal and two products."""
    from diff_sampler_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(rows)
    x = torch.randn(rows, ld, generator=g)
    x[0, :4] = torch.tensor([0.0, -60.0, -20.0, -1.0])         # exp overflows at -60: the result is (minus) zero, never NaN
    want = (x.double() * torch.sigmoid(1.702 * x.double()))[:, :cols]
    xd = x.cuda()
    y = torch.full((rows, ld), float('nan'), device='cuda')
    _lib.check(lib.ds_quick_gelu(_p(xd), ld, _p(y), ld, rows, cols, _lib.stream_ptr()))
    torch.cuda.synchronize()
    err = float((y[:, :cols].double().cpu() - want).abs().max() / want.abs().max())
    print(f'quick_gelu {rows}x{cols}: {err:.2e} of max |y|')
    assert err < 1e-6
    assert ld == cols or bool(torch.isnan(y[:, cols:]).all())
    _lib.check(lib.ds_quick_gelu(_p(xd), ld, _p(xd), ld, rows, cols, _lib.stream_ptr()))       # in place
    torch.cuda.synchronize()
    assert torch.equal(xd[:, :cols], y[:, :cols]) and torch.equal(xd[:, cols:].cpu(), x[:, cols:])


def _packed(sq, seed, Bz=2, heads=2, d=64):
    """q | k | v as slices of one packed [rows][3 * 128 + 8] tensor."""
    g = torch.Generator().manual_seed(seed)
    C_ = heads * d
    qkv = torch.randn(Bz, sq, 3 * C_ + 8, generator=g)
    qkv[:, :, C_:2 * C_] *= 1.5
    return qkv


def _run_causal(qkv, sq, Bz=2, heads=2, d=64):
    from diff_sampler_amd import _lib
    C_ = heads * d
    ld = 3 * C_ + 8
    qd = qkv.cuda().contiguous()
    out = torch.full((Bz, sq, C_), float('nan'), device='cuda')
    a = _lib.AttnArgs(_p(qd), _p(qd[:, :, C_:]), _p(qd[:, :, 2 * C_:]), _p(out), ld, ld, ld, C_, sq * ld, sq * ld, sq * ld, sq * C_, Bz, heads,
                      sq, sq, d, d ** -0.5)
    _lib.check(_lib.load().ds_attention_causal(C.byref(a), _lib.stream_ptr()), 'ds_attention_causal')
    torch.cuda.synchronize()
    return out.cpu()


def _causal_ref(qkv, sq, Bz=2, heads=2, d=64):
    C_ = heads * d
    q, k, v = (qkv[:, :, i * C_:(i + 1) * C_].reshape(Bz, sq, heads, d).double() for i in range(3))
    s = torch.einsum('bqhd,bkhd->bhqk', q, k) * d ** -0.5
    s = s.masked_fill(torch.ones(sq, sq, dtype=torch.bool).triu(1), float('-inf'))
    return torch.einsum('bhqk,bkhd->bqhd', s.softmax(-1), v).reshape(Bz, sq, C_)


@pytest.mark.parametrize('sq', [1, 31, 32, 33, 77, 128])
def test_causal_attention_matches_a_masked_fp64_softmax(sq):
    from diff_sampler_amd import _lib
    assert _lib.load().ds_attention_causal_supported(64, sq)
    qkv = _packed(sq, 100 + sq)
    out, ref = _run_causal(qkv, sq), _causal_ref(qkv, sq)
    assert not bool(torch.isnan(out).any())
    err = _rel(out, ref)
    print(f'ds_attention_causal sq={sq}: {err:.2e}')
    assert err < ATTN_TOL
    assert _rel(out[:, 0], qkv[:, 0, 256:384]) < 1e-6          # row 0 attends to itself only: its output is v[0]


@pytest.mark.parametrize('t', [1, 32, 33, 76])
def test_causal_attention_never_looks_ahead(t):
    """K and V rows >= t multiplied by 1e3: output rows < t keep their bits."""
    sq = 77
    qkv = _packed(sq, 7)
    clean = _run_causal(qkv, sq)
    poisoned = qkv.clone()
    poisoned[:, t:, 128:384] *= 1e3
    out = _run_causal(poisoned, sq)
    assert torch.equal(out[:, :t], clean[:, :t])
    assert not torch.equal(out[:, t:], clean[:, t:])


def test_causal_attention_rejects_what_it_does_not_cover():
    from diff_sampler_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(4 * 129 * 3 * 128, device='cuda')
    out = torch.zeros(129 * 128, device='cuda')

    def rc(sq, skv, d, **kw):
        a = _lib.AttnArgs(_p(buf), _p(buf), _p(buf), _p(out), 384, 384, 384, 128, sq * 384, sq * 384, sq * 384, sq * 128, 1, 1, sq, skv, d, 0.125)
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.ds_attention_causal(C.byref(a), _lib.stream_ptr())
    assert rc(129, 129, 64) == -3 and rc(77, 77, 40) == -3
    assert rc(77, 64, 64) in (-1, -3)
    assert rc(77, 77, 64, in_f16=1) == -1 and rc(77, 77, 64, out_f16=1) == -1
    assert lib.ds_attention_causal_supported(64, 129) == 0 and lib.ds_attention_causal_supported(40, 77) == 0
    torch.cuda.synchronize()
    assert float(out.abs().max()) == 0.0                      # never a launch


# ---------------------------------------------------------------------------------------------------------------- encoder
@pytest.mark.parametrize('gold', ['clip_tiny.npz', 'clip_sd15.npz'])
def test_encoder_matches_the_real_class(gold):
    """Whole encoder against transformers' CLIPTextModel (golden): 2e-4 of the output absmax, the bound of the project's fp32 network goldens.
    Achieved on an MI355X: 1.24e-6 (clip_tiny) and 1.44e-6 (clip_sd15) -- fp32 rounding.  The goldens record that dropping the mask moves the output by 0.93 / 1.07 of that scale and erf-GELU by
    1.1e-2 / 1.2e-2."""
    from test_clip_cpu import golden_distance
    from diff_sampler_amd.clip_engine import ClipTextEncoder
    z = np.load(os.path.join(G, gold))
    enc = ClipTextEncoder.from_config(str(z['config']), seed=int(z['seed']))
    out = enc(torch.from_numpy(z['tokens']))
    torch.cuda.synchronize()
    assert out.shape == (3, 77, enc.spec.width) and out.dtype == torch.float32
    err = golden_distance(z, out)
    print(f'{gold}: {err:.2e} of the output absmax')
    assert err < NET_TOL == float(z['bound'])


@pytest.fixture(scope='module')
def tiny():
    z = np.load(os.path.join(G, 'clip_tiny.npz'))
    g = torch.Generator().manual_seed(11)
    tokens = torch.randint(0, 512, (5, 77), generator=g)
    tokens[3, 6:] = 511
    return int(z['seed']), tokens


@pytest.mark.parametrize('invariant', [False, True])
def test_encoder_rows_do_not_depend_on_their_batch(tiny, invariant):
    """B = 5 against five B = 1 runs: within the network bound, and the same bits under batch_invariant=True."""
    from diff_sampler_amd.clip_engine import ClipTextEncoder
    seed, tokens = tiny
    enc = ClipTextEncoder.from_config('tiny_clip', seed=seed, batch_invariant=invariant)
    all5 = enc(tokens)
    for i in range(5):
        one = enc(tokens[i:i + 1])
        assert _rel(all5[i], one[0]) < NET_TOL
        if invariant:
            assert torch.equal(all5[i], one[0]), i
    assert not torch.equal(all5[0], all5[1])


def test_encoder_graph_replay_and_repeat_runs_are_bit_equal(tiny):
    from diff_sampler_amd.clip_engine import ClipTextEncoder
    seed, tokens = tiny
    enc = ClipTextEncoder.from_config('tiny_clip', seed=seed)
    out, plan = enc.raw(tokens)
    eager = out.clone()
    again, _ = enc.raw(tokens)
    assert torch.equal(again, eager)                          # the same plan run twice
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sp = C.c_void_p(side.cuda_stream)
        plan.graph_capture(sp)
        plan.bufs['out'].zero_()
        plan.graph_launch(sp)
        side.synchronize()
    assert torch.equal(plan.bufs['out'].view_as(eager), eager)


def test_loader_gives_the_bits_of_from_config(tiny):
    from diff_sampler_amd import clip_arch as ca
    from diff_sampler_amd.clip_engine import ClipTextEncoder
    seed, tokens = tiny
    spec = ca.clip_text_spec(**ca.NAMED_CLIP_CONFIGS['tiny_clip'])
    sd = {'cond_stage_model.transformer.' + k: v for k, v in ca.init_clip_params(spec, seed=seed).items()}
    sd['cond_stage_model.transformer.text_model.embeddings.position_ids'] = torch.arange(77)[None]
    a = ClipTextEncoder.from_state_dict(sd, name_or_kwargs='tiny_clip')(tokens[:2])
    b = ClipTextEncoder.from_config('tiny_clip', seed=seed)(tokens[:2])
    assert torch.equal(a, b)
    del sd['cond_stage_model.transformer.text_model.encoder.layers.1.layer_norm2.weight']
    with pytest.raises(KeyError):
        ClipTextEncoder.from_state_dict(sd, name_or_kwargs='tiny_clip')
    with pytest.raises(ValueError):
        ClipTextEncoder.from_config('tiny_clip', seed=seed)(tokens + 512)


def test_conditioning_helper_of_the_sampler(tmp_path):
    """sample.encode_conditions with the tiny encoder (its vocabulary widened to the synthetic tokenizer's) and a tokenizer directory the test
    writes: equal prompts give equal rows, uc is the encoding of "", guidance 1.0 gives uc None."""
    from _clip_tok import write_tokenizer
    from diff_sampler_amd import clip_arch as ca, sample
    from diff_sampler_amd.clip_engine import ClipTextEncoder
    from diff_sampler_amd.clip_tokenizer import ClipTokenizer
    write_tokenizer(str(tmp_path))
    tok = ClipTokenizer(str(tmp_path))
    enc = ClipTextEncoder.from_config(dict(ca.NAMED_CLIP_CONFIGS['tiny_clip'], vocab=tok.vocab_size), seed=2)
    prompts = ['lower', 'newer hi', 'lower', 'lower']
    c, uc = sample.encode_conditions(enc, tok, prompts, 7.5)
    assert c.shape == (4, 77, 128) and uc.shape == (4, 77, 128)
    assert torch.equal(c[0], c[2]) and torch.equal(c[0], c[3]) and not torch.equal(c[0], c[1])
    assert len(enc._plans) == 1 and 3 in enc._plans            # 'lower', 'newer hi', '': identical prompts are encoded once
    empty = enc(tok(['']))
    assert _rel(uc[0], empty[0]) < NET_TOL and torch.equal(uc[0], uc[3])
    assert _rel(c[1], enc(tok(['newer hi']))[0]) < NET_TOL
    c1, uc1 = sample.encode_conditions(enc, tok, prompts, 1.0)
    assert uc1 is None and _rel(c1, c) < NET_TOL
    c2, uc2 = sample.encode_conditions(enc, tok, ['', 'low'], None)
    assert torch.equal(c2[0], uc2[0]) and torch.equal(uc2[0], uc2[1])


def test_cli_tokenizer_path_conditions_the_latents_on_the_prompt(tmp_path, monkeypatch):
    """`--dataset_name ms_coco --random_init True --tokenizer_path DIR --prompts_path FILE`: run() asks create_model for the text encoder and
    the latents equal a sampler call on encode_conditions' states of the file's lines (line i = seed i) -- and not one on other prompts.
    The model is built once and handed to run() through create_model."""
    from _clip_tok import write_tokenizer
    from diff_sampler_amd import sample, solvers, solver_utils
    from diff_sampler_amd.clip_tokenizer import ClipTokenizer
    tok_dir = str(tmp_path / 'tok')
    write_tokenizer(tok_dir)
    with open(tmp_path / 'prompts.txt', 'w') as fh:
        fh.write('lower newer\nhi low\n')
    net, kind = sample.create_model('ms_coco', None, True, 'cuda', guidance_type='cfg', guidance_rate=7.5, text_encoder=True)
    assert kind == 'ldm' and net.text_encoder.spec.width == net.spec.context_dim == 768 and net.decoder is None
    asked = []
    monkeypatch.setattr(sample, 'create_model', lambda *a, **k: (asked.append(k), (net, kind))[1])
    kw = dict(max_batch_size=2, seeds='0-1', solver='dpmpp', max_order=2, num_steps=3, predict_x0=False, lower_order_final=True,
              schedule_type='discrete', schedule_rho=1, guidance_type='cfg', guidance_rate=7.5, random_init=True)
    out_dir, n = sample.run('ms_coco', outdir=str(tmp_path / 'a'), tokenizer_path=tok_dir, prompts_path=str(tmp_path / 'prompts.txt'), **kw)
    assert n == 2 and asked[-1].get('text_encoder') is True
    got = np.stack([np.load(os.path.join(out_dir, '000000', f'{s:06d}.npy')) for s in (0, 1)])
    lat = sample.StackedRandomGenerator('cuda', [0, 1]).randn([2, 4, 64, 64], device='cuda')
    ts = solver_utils.get_schedule(3, net.sigma_min, net.sigma_max, device='cuda', schedule_type='discrete', schedule_rho=1, net=net)

    def direct(prompts):
        c, uc = sample.encode_conditions(net.text_encoder, ClipTokenizer(tok_dir), prompts, 7.5)
        return solvers.dpm_pp_sampler(net, lat, condition=c, unconditional_condition=uc, num_steps=3, sigma_min=net.sigma_min, sigma_max=net.sigma_max,
                                      schedule_type='discrete', schedule_rho=1, max_order=2, predict_x0=False, lower_order_final=True, t_steps=ts)
    assert np.isfinite(got).all() and _rel(got, direct(['lower newer', 'hi low'])) < 5e-4       # the trajectory bound of DESIGN.md section 2
    assert _rel(got, direct(['hi low', 'lower newer'])) > 1e-2                                  # the prompts matter
    sample.run('ms_coco', outdir=str(tmp_path / 'b'), **kw)
    assert 'text_encoder' not in asked[-1]                                                      # without --tokenizer_path nothing is asked for
