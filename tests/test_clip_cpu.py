"""CPU: the CLIP text encoder's host side -- the restatement the GPU tests compare with (tests/_clip_ref.py) against the real class's
goldens, the parameter table against the real class, the launch plan (built on the CPU: nothing runs), the new ABI symbols, the byte-pair
tokenizer on a vocabulary written by the test, and the CLI options."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
G = os.path.join(ROOT, 'tests', 'golden')
GOLDS = ['clip_tiny.npz', 'clip_sd15.npz']


def _spec_params(z):
    from diff_sampler_amd import clip_arch as ca
    spec = ca.clip_text_spec(**ca.NAMED_CLIP_CONFIGS[str(z['config'])])
    return spec, ca.init_clip_params(spec, seed=int(z['seed']))


def golden_distance(z, out):
    """max |out - golden| / max |golden| over what the golden stores (clip_sd15.npz: image 0 whole, chosen rows of the others)."""
    out = torch.as_tensor(out).detach().double().cpu()
    if 'out' in z.files:
        d = (out - torch.from_numpy(z['out']).double()).abs().max()
    else:
        rows = torch.from_numpy(z['rows']).long()
        d = torch.maximum((out[0] - torch.from_numpy(z['out0']).double()).abs().max(),
                          (out[1:][:, rows] - torch.from_numpy(z['out_rows']).double()).abs().max())
    return float(d) / float(z['out_absmax'])


@pytest.mark.parametrize('gold', GOLDS)
def test_restatement_equals_the_real_class(gold):
    """tests/_clip_ref.py == transformers' CLIPTextModel (recorded by tools/gen_clip_golden.py) to fp32 rounding: 1e-5 of the output scale
    (measured 6e-7 / 1e-6 on the recording machine; another thread count may order the sums differently)."""
    from _clip_ref import clip_text_ref
    z = np.load(os.path.join(G, gold))
    spec, params = _spec_params(z)
    with torch.no_grad():
        out = clip_text_ref(params, z['tokens'], spec.heads, spec.layers, spec.eps)
    assert out.shape == (3, spec.positions, spec.width) and out.dtype == torch.float32
    assert golden_distance(z, out) < 1e-5


@pytest.mark.parametrize('gold', GOLDS)
def test_goldens_tell_a_missing_mask_and_a_wrong_activation_apart(gold):
    """The sensitivity condition the generator asserts and stores: without the causal mask, and with erf-GELU for quick_gelu, the output moves
    by at least 50 x the bound of the engine's test.  Recomputed here for the tiny golden."""
    from _clip_ref import clip_text_ref
    z = np.load(os.path.join(G, gold))
    bound = float(z['bound'])
    assert bound == 2e-4
    assert float(z['nomask_dist']) >= 50 * bound and float(z['erf_dist']) >= 50 * bound
    assert 3.0 < float(z['out_absmax']) < 8.0 and float(z['ref_dist']) < 1e-5
    tok = z['tokens']
    assert tok.shape == (3, 77) and tok.min() >= 0 and (tok[1, 10:] == tok[1, 76]).all() and len(set(tok[0].tolist())) > 60
    assert os.path.getsize(os.path.join(G, gold)) < (1 << 20)
    if gold == 'clip_tiny.npz':
        spec, params = _spec_params(z)
        with torch.no_grad():
            for kw, key in ((dict(causal=False), 'nomask_dist'), (dict(act='gelu'), 'erf_dist')):
                d = golden_distance(z, clip_text_ref(params, tok, spec.heads, spec.layers, spec.eps, **kw))
                assert d >= 50 * bound and abs(d - float(z[key])) < 1e-4, (key, d)


def test_parameter_table_loads_strictly_into_the_real_class():
    transformers = pytest.importorskip('transformers')
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import gen_clip_golden as gen
    from diff_sampler_amd import clip_arch as ca
    spec = ca.clip_text_spec(**ca.NAMED_CLIP_CONFIGS['tiny_clip'])
    params = ca.init_clip_params(spec, seed=1)
    model = gen.real_model(spec)
    gen.load_strict(model, params)                    # strict=True inside: every key and shape is the real class's
    got = {k.split('text_model.')[-1]: v for k, v in model.state_dict().items() if not k.endswith('position_ids')}
    assert set(got) == {k[len('text_model.'):] for k in params}
    assert all(torch.equal(got[k[len('text_model.'):]], v) for k, v in params.items())


def test_spec_and_init():
    from diff_sampler_amd import clip_arch as ca
    sd15 = ca.clip_text_spec(**ca.NAMED_CLIP_CONFIGS['sd15'])
    assert (sd15.vocab, sd15.width, sd15.layers, sd15.heads, sd15.head_dim, sd15.ffn, sd15.positions, sd15.eps) == (49408, 768, 12, 12, 64, 3072, 77, 1e-5)
    tiny = ca.clip_text_spec(**ca.NAMED_CLIP_CONFIGS['tiny_clip'])
    assert (tiny.vocab, tiny.width, tiny.layers, tiny.heads, tiny.head_dim, tiny.ffn, tiny.positions) == (512, 128, 2, 2, 64, 512, 77)
    assert len(ca.clip_param_table(sd15)) == 2 + 12 * 16 + 2
    # the issue's arithmetic: 14.2 MFLOP per token and layer in the projections, about 13.1 GFLOP per prompt
    assert 2.0 * (4 * 768 * 768 + 2 * 768 * 3072) == 14155776.0
    assert 13.0e9 < 12 * 77 * 14155776.0 < 13.2e9 < ca.clip_flops_per_prompt(sd15) < 13.4e9
    a, b = ca.init_clip_params(tiny, seed=3), ca.init_clip_params(tiny, seed=3)
    assert all(torch.equal(a[k], b[k]) for k in a) and not torch.equal(a['text_model.final_layer_norm.bias'], ca.init_clip_params(tiny, seed=4)['text_model.final_layer_norm.bias'])


def test_the_new_symbols_bind_and_answer_host_side_queries():
    from diff_sampler_amd import build, _lib
    build.build_lib(verbose=False)
    lib = _lib.load()
    for name in ('ds_attention_causal', 'ds_attention_causal_supported', 'ds_token_embed', 'ds_quick_gelu'):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.ds_version() == 7 and len(_lib.EXPORTS) == 61
    assert (_lib.DS_OP_TOKEN_EMBED, _lib.DS_OP_ATTENTION_CAUSAL, _lib.DS_OP_QUICK_GELU) == (14, 15, 16)
    ok = lib.ds_attention_causal_supported
    assert [ok(64, s) for s in (1, 31, 32, 33, 77, 128)] == [1] * 6
    assert ok(64, 0) == 0 and ok(64, 129) == 0 and ok(40, 77) == 0 and ok(128, 77) == 0
    # argument errors are host-side answers: nothing is launched (there is no GPU here)
    buf = torch.zeros(64)
    p = buf.data_ptr()
    mk = lambda sq, skv, d: _lib.AttnArgs(p, p, p, p, 64, 64, 64, 64, 64 * sq, 64 * sq, 64 * sq, 64 * sq, 1, 1, sq, skv, d, 0.125)
    assert lib.ds_attention_causal(C.byref(mk(129, 129, 64)), None) == -3
    assert lib.ds_attention_causal(C.byref(mk(77, 77, 40)), None) == -3
    assert lib.ds_attention_causal(C.byref(mk(77, 64, 64)), None) == -1
    a = mk(77, 77, 64)
    a.in_f16 = 1
    assert lib.ds_attention_causal(C.byref(a), None) == -1
    assert lib.ds_quick_gelu(p, 6, p, 8, 1, 4, None) == -2 and lib.ds_token_embed(p, p, p, p, 130, 1, 77, 128, 512, None) == -2
    # ds_plan_add takes the three new op codes with their struct sizes only
    h = C.c_void_p()
    assert lib.ds_plan_create(C.byref(h)) == 0
    for code, st in ((14, _lib.TokenEmbedArgs()), (15, _lib.AttnArgs()), (16, _lib.QuickGeluArgs())):
        assert lib.ds_plan_add(h, code, C.byref(st), C.sizeof(st)) == 0
        assert lib.ds_plan_add(h, code, C.byref(st), C.sizeof(st) - 4) != 0
    assert lib.ds_plan_size(h) == 3
    lib.ds_plan_destroy(h)


@pytest.mark.parametrize('name,B', [('tiny_clip', 1), ('tiny_clip', 5), ('sd15', 17)])
def test_plan_builds_without_a_gpu(name, B):
    """1 embedding launch + per layer {LayerNorm, q|k|v, causal attention, out_proj, LayerNorm, fc1, quick_gelu, fc2} + the final LayerNorm;
    finish() finds a kernel for every projection and the native plan takes every launch.  (The issue's hand count says nine launches per
    layer; the eight listed here are every operation of a layer -- with q | k | v packed as one projection there is no ninth.)"""
    from diff_sampler_amd import _lib
    from diff_sampler_amd.clip_engine import ClipTextEncoder
    lib = _lib.load()
    enc = ClipTextEncoder.from_config(name, seed=0, device='cpu')
    spec = enc.spec
    P = enc.plan(B)
    assert P is enc.plan(B)
    names = [op.name for op in P.ops]
    per_layer = ['layer_norm1', 'qkv', 'attention', 'out_proj', 'layer_norm2', 'fc1', 'quick_gelu', 'fc2']
    assert names == ['embeddings'] + [f'layers.{i}.{n}' for i in range(spec.layers) for n in per_layer] + ['final_layer_norm']
    assert len(P.ops) == 1 + spec.layers * 8 + 1
    convs = [op for op in P.ops if op.fn is lib.ds_conv2d_nhwc]
    assert len(convs) == 4 * spec.layers and len(P.kernel_ids) == len(convs) and min(P.kernel_ids.values()) >= 0
    for op in convs:
        a = op.keep[0]
        assert (a.taps, a.n, a.h, a.w, a.wgt_f16, a.in_f16, a.out_f16) == (1, B * spec.positions, 1, 1, 0, 0, 0), op.name     # fp32, ragged rows
        assert bool(a.res) == op.name.endswith(('out_proj', 'fc2')) and a.bias
    att = [op.keep[0] for op in P.ops if op.fn is lib.ds_attention_causal]
    assert len(att) == spec.layers and all((a.batch, a.heads, a.sq, a.skv, a.d, a.ldq, a.ldo) == (B, spec.heads, 77, 77, 64, 3 * spec.width, spec.width) for a in att)
    assert all(abs(a.scale - 0.125) < 1e-9 and a.k - a.q == 4 * spec.width and a.v - a.q == 8 * spec.width for a in att)   # packed q|k|v read in place
    assert lib.ds_plan_size(P.native()) == len(P.ops)
    P.close()
    inv = ClipTextEncoder.from_config(name, seed=0, device='cpu', batch_invariant=True) if name == 'tiny_clip' else None
    if inv is not None:
        assert all(op.keep[0].tune.invariant == 1 for op in inv.plan(B).ops if op.fn is lib.ds_conv2d_nhwc)
        assert all(op.keep[0].tune.invariant == 0 for op in convs)


def test_token_ids_are_validated_on_the_host():
    from diff_sampler_amd.clip_engine import ClipTextEncoder
    enc = ClipTextEncoder.from_config('tiny_clip', seed=0, device='cpu')
    good = torch.zeros(2, 77, dtype=torch.int64)
    assert enc.check_tokens(good).dtype == torch.int32
    for bad in (good[:, :76], good.float(), good + 512, good - 1, good[0]):
        with pytest.raises(ValueError):
            enc.check_tokens(bad)


def test_loader_takes_the_checkpoint_names_and_nothing_else():
    from diff_sampler_amd import clip_arch as ca
    from diff_sampler_amd.clip_engine import ClipTextEncoder
    spec = ca.clip_text_spec(**ca.NAMED_CLIP_CONFIGS['tiny_clip'])
    params = ca.init_clip_params(spec, seed=5)
    sd = {'cond_stage_model.transformer.' + k: v.clone() for k, v in params.items()}
    sd['cond_stage_model.transformer.text_model.embeddings.position_ids'] = torch.arange(77)[None]
    sd['model.diffusion_model.time_embed.0.weight'] = torch.ones(4, 4)
    sd['first_stage_model.decoder.conv_in.bias'] = torch.ones(4)
    a = ClipTextEncoder.from_state_dict(sd, name_or_kwargs='tiny_clip', device='cpu')
    b = ClipTextEncoder.from_config('tiny_clip', seed=5, device='cpu')
    assert set(a.w) == set(b.w) and all(torch.equal(a.w[k], b.w[k]) for k in a.w)
    # q | k | v are packed in that order, rows padded to the 128-row tile
    q = params['text_model.encoder.layers.1.self_attn.q_proj.weight']
    v = params['text_model.encoder.layers.1.self_attn.v_proj.bias']
    assert a.w['1.qkv.w'].shape == (384, 128) and torch.equal(a.w['1.qkv.w'][:128], q) and torch.equal(a.w['1.qkv.b'][256:], v)
    assert set(ca.split_cond_stage(sd)) == {k for k in sd if k.startswith('cond_stage_model.')}
    missing = dict(sd)
    del missing['cond_stage_model.transformer.text_model.encoder.layers.0.mlp.fc2.bias']
    with pytest.raises(KeyError):
        ClipTextEncoder.from_state_dict(missing, name_or_kwargs='tiny_clip', device='cpu')
    extra = dict(sd)
    extra['cond_stage_model.transformer.text_model.encoder.layers.2.mlp.fc2.bias'] = torch.zeros(128)
    with pytest.raises(KeyError):
        ClipTextEncoder.from_state_dict(extra, name_or_kwargs='tiny_clip', device='cpu')
    wrong = dict(sd)
    wrong['cond_stage_model.transformer.text_model.final_layer_norm.bias'] = torch.zeros(64)
    with pytest.raises(ValueError):
        ClipTextEncoder.from_state_dict(wrong, name_or_kwargs='tiny_clip', device='cpu')
    bare = ClipTextEncoder.from_state_dict(params, prefix='', name_or_kwargs='tiny_clip', device='cpu')
    assert all(torch.equal(bare.w[k], b.w[k]) for k in b.w)


# ---------------------------------------------------------------------------------------------------------------- tokenizer
def test_tokenizer_follows_the_published_rules(tmp_path):
    from diff_sampler_amd.clip_tokenizer import ClipTokenizer, bytes_to_unicode
    from _clip_tok import write_tokenizer
    v = write_tokenizer(str(tmp_path))
    tok = ClipTokenizer(str(tmp_path))
    bos, eos = v['<|startoftext|>'], v['<|endoftext|>']
    assert (tok.bos, tok.eos, tok.vocab_size) == (bos, eos, 256 + 256 + 6 + 2)
    tb = bytes_to_unicode()
    assert len(set(tb.values())) == 256 and tb[ord('a')] == 'a' and tb[ord(' ')] == chr(256 + 32) and tb[0xA1] == chr(0xA1) and tb[0xAD] == chr(256 + 67)
    # merges in rank order, by hand.  "lower": l o w e r</w> -> (l,o) rank 0: lo w e r</w> -> (e,r</w>) rank 2 beats none better: lo w er</w>;
    # (lo, w</w>) does not apply (the w is not a word end) -> [lo, w, er</w>]
    assert tok.encode('lower') == [v['lo'], v['w'], v['er</w>']]
    # "low": l o w</w> -> lo w</w> -> low</w>
    assert tok.encode('low') == [v['low</w>']]
    # "newer": n e w e r</w>: rank 2 (e, r</w>) first -> n e w er</w>; rank 3 (n, e) -> ne w er</w>; rank 4 (ne, w) -> new er</w>
    assert tok.encode('newer') == [v['new'], v['er</w>']]
    # case folding and whitespace: the same ids
    assert tok.encode('  LoW \t\n nEwEr ') == [v['low</w>'], v['new'], v['er</w>']]
    # an unmergeable word: its characters, the last with the word-end mark
    assert tok.encode('xyz') == [v['x'], v['y'], v['z</w>']]
    # digits split one by one, punctuation runs stay together, contractions split off
    assert tok.encode("hi42!?") == [v['hi</w>'], v['4</w>'], v['2</w>'], v['!'], v['?</w>']]
    assert tok.encode("hi's") == [v['hi</w>'], v["'"], v['s</w>']]
    # a non-ASCII character: its UTF-8 bytes 0xC3 0xA9 through the byte table, one word
    assert tok.encode('é') == [v[tb[0xC3]], v[tb[0xA9] + '</w>']]
    # the empty prompt, padding, truncation
    ids = tok([''])
    assert ids.shape == (1, 77) and ids.dtype == torch.int64 and ids[0].tolist() == [bos] + [eos] * 76
    ids = tok(['low', 'x ' * 100])
    assert ids[0].tolist() == [bos, v['low</w>']] + [eos] * 75
    assert ids[1].tolist() == [bos] + [v['x</w>']] * 75 + [eos]
    assert tok('low').shape == (1, 77)
    with pytest.raises(FileNotFoundError):
        ClipTokenizer(str(tmp_path / 'nowhere'))


def test_batch_prompts_follow_the_reference_rule(tmp_path):
    from diff_sampler_amd import sample
    assert sample.batch_prompts([4, 5, 6], prompt='a cat') == ['a cat'] * 3
    lines = [f'p{i}' for i in range(10)]
    assert sample.batch_prompts(torch.tensor([4, 5, 6]), prompt='ignored', prompts=lines) == ['p4', 'p5', 'p6']
    with pytest.raises(ValueError):
        sample.batch_prompts([8, 9, 10], prompts=lines)
    with pytest.raises(ValueError):
        sample.batch_prompts([0, 1])


def test_cli_parses_tokenizer_path_and_leaves_every_other_run_alone(tmp_path, monkeypatch):
    import PIL.Image
    from click.testing import CliRunner
    from diff_sampler_amd import sample
    base = ['--stub', 'true', '--dataset_name', 'cifar10', '--solver', 'ipndm', '--num_steps', '6', '--batch', '4', '--seeds', '0-5', '--prompt', 'a cat']
    seen = []
    real_run = sample.run
    monkeypatch.setattr(sample, 'run', lambda **kw: (seen.append(dict(kw)), real_run(**kw))[1])
    outs = []
    for i, extra in enumerate(([], ['--tokenizer_path', str(tmp_path / 'tok'), '--prompts_path', str(tmp_path / 'p.txt')])):
        out = tmp_path / f'o{i}'
        r = CliRunner().invoke(sample.main, base + ['--outdir', str(out)] + extra)
        assert r.exit_code == 0, r.output
        files = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)
        outs.append((files, [np.asarray(PIL.Image.open(out / f)).tobytes() for f in files]))
    assert outs[0] == outs[1] and len(outs[0][0]) == 6
    assert seen[0]['tokenizer_path'] is None and seen[0]['prompts_path'] is None
    assert seen[1]['tokenizer_path'] == str(tmp_path / 'tok') and seen[1]['prompts_path'] == str(tmp_path / 'p.txt')
    # without the option the dictionary click hands to run() is the earlier one plus two None entries that run() removes first
    strip = lambda kw: {k: v for k, v in kw.items() if k not in ('tokenizer_path', 'prompts_path', 'outdir')}
    assert strip(seen[0]) == strip(seen[1]) and seen[0]['prompt'] == 'a cat'
    import inspect
    assert 'text_encoder' in inspect.signature(sample.create_model).parameters
    assert inspect.signature(sample.create_model).parameters['text_encoder'].default is False
