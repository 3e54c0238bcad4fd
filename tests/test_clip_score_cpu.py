"""CPU-only: CLIP score (diff_sampler_amd/clip_score*.py; reference clip_score.py of the four repositories).

The parameter table is that of the real class; the open_clip converter round-trips and is strict; the plain-torch restatement reproduces the
goldens recorded from transformers' CLIPModel; the goldens carry their sensitivity distances; padding cannot reach the pooled text feature;
the host preprocessing has open_clip's geometry; captions pair with the full listing and shard like fid.py; both towers' plans build
without a GPU with the expected launches; every new entry point rejects bad arguments on the host; the d = 88 attention kernel needs no
scratch."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diff_sampler_amd import clip_score as CS, clip_score_arch as A  # noqa: E402
from tests import _clip_vit_ref as R  # noqa: E402

GOLDENS = {'tiny_clip_score': 'clip_score_tiny.npz', 'vit_g_14_2l': 'clip_score_vitg2l.npz'}
EPS = 2e-4


@pytest.fixture(scope='module')
def goldens(golden_dir):
    return {k: np.load(os.path.join(golden_dir, f)) for k, f in GOLDENS.items()}


@pytest.fixture(scope='module')
def libs():
    from diff_sampler_amd import build, _lib, _metrics_lib
    build.build_metrics_lib(verbose=False)
    return _lib.load(), _metrics_lib.load()


# ------------------------------------------------------------------------------------------------------------------ architecture
def test_named_configs():
    g = A.named_spec('vit_g_14')
    assert (g.vision.width, g.vision.layers, g.vision.heads, g.vision.ffn, g.vision.head_dim) == (1408, 40, 16, 6144, 88)
    assert (g.text.width, g.text.layers, g.text.heads, g.text.ffn, g.text.head_dim) == (1024, 24, 16, 4096, 64)
    assert (g.patch, g.image_size, g.vision_tokens, g.vocab, g.positions, g.embed, g.act) == (14, 224, 257, 49408, 77, 1024, 'gelu')
    l2 = A.named_spec('vit_g_14_2l')
    assert (l2.vision.layers, l2.text.layers) == (2, 2) and l2.vision.width == 1408 and l2.embed == 1024
    t = A.named_spec('tiny_clip_score')
    assert (t.vision.width, t.vision.heads, t.vision.head_dim, t.vision.layers, t.vision.ffn, t.vision_tokens) == (352, 4, 88, 2, 1536, 257)
    assert (t.text.width, t.text.heads, t.text.ffn, t.vocab, t.embed) == (128, 2, 512, 512, 64)
    with pytest.raises(ValueError):
        A.clip_score_spec(**dict(A.NAMED_CLIP_SCORE_CONFIGS['tiny_clip_score'], act='relu'))


@pytest.mark.parametrize('name', ['tiny_clip_score', 'vit_g_14_2l'])
def test_parameter_table_is_the_real_class_state_dict(name):
    pytest.importorskip('transformers')
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import gen_clip_score_golden as G
    spec = A.named_spec(name)
    with torch.device('meta'):
        sd = G.real_model(spec).state_dict()
    table = {k: s for k, s, _ in A.clip_score_param_table(spec)}
    real = {k: tuple(v.shape) for k, v in sd.items() if k not in A.IGNORED_KEYS}
    assert 'logit_scale' in sd and real == {k: tuple(s) for k, s in table.items()}


def test_init_is_deterministic_and_state_dict_is_strict():
    spec = A.named_spec('tiny_clip_score')
    p, q = A.init_clip_score_params(spec, 4), A.init_clip_score_params(spec, 4)
    assert all(torch.equal(p[k], q[k]) for k in p) and not torch.equal(p['text_projection.weight'], A.init_clip_score_params(spec, 5)['text_projection.weight'])
    got = A.params_from_state_dict(spec, dict(p, logit_scale=torch.tensor(4.6)))            # accepted and ignored
    assert set(got) == set(p)
    with pytest.raises(KeyError):
        A.params_from_state_dict(spec, {k: v for k, v in p.items() if k != 'visual_projection.weight'})
    with pytest.raises(KeyError):
        A.params_from_state_dict(spec, dict(p, surplus=torch.zeros(1)))
    with pytest.raises(ValueError):
        A.params_from_state_dict(spec, dict(p, **{'text_projection.weight': torch.zeros(64, 127)}))


def test_open_clip_converter_round_trips_and_is_strict():
    spec = A.named_spec('tiny_clip_score')
    p = A.init_clip_score_params(spec, 2)
    oc = A.to_open_clip(spec, p)
    assert tuple(oc['visual.proj'].shape) == (352, 64) and tuple(oc['text_projection'].shape) == (128, 64)        # stored [width, embed]
    assert tuple(oc['visual.transformer.resblocks.1.attn.in_proj_weight'].shape) == (3 * 352, 352)
    assert tuple(oc['transformer.resblocks.0.attn.in_proj_bias'].shape) == (3 * 128,)
    assert {'visual.conv1.weight', 'visual.class_embedding', 'visual.positional_embedding', 'visual.ln_pre.weight', 'visual.ln_post.bias',
            'token_embedding.weight', 'positional_embedding', 'ln_final.weight', 'visual.transformer.resblocks.0.mlp.c_fc.weight',
            'transformer.resblocks.1.mlp.c_proj.bias', 'transformer.resblocks.1.ln_2.weight'} <= set(oc)
    assert A.is_open_clip(oc) and not A.is_open_clip(p)
    assert A.spec_from_state_dict(oc) == spec and A.spec_from_state_dict(p) == spec
    back = A.from_open_clip(spec, dict(oc, logit_scale=torch.tensor(4.6)))
    assert set(back) == set(p) and all(torch.equal(back[k], p[k]) for k in p)
    # q | k | v order of in_proj: the q rows come first
    assert torch.equal(oc['transformer.resblocks.0.attn.in_proj_weight'][:128], p['text_model.encoder.layers.0.self_attn.q_proj.weight'])
    with pytest.raises(KeyError):
        A.from_open_clip(spec, {k: v for k, v in oc.items() if k != 'visual.ln_pre.bias'})
    with pytest.raises(KeyError):
        A.from_open_clip(spec, dict(oc, **{'visual.extra': torch.zeros(1)}))
    with pytest.raises(ValueError):
        A.from_open_clip(spec, dict(oc, **{'visual.proj': oc['visual.proj'].t().contiguous()}))
    with pytest.raises(ValueError):
        A.from_open_clip(spec, dict(oc, **{'transformer.resblocks.0.attn.in_proj_bias': torch.zeros(2 * 128)}))


# ------------------------------------------------------------------------------------------------------------------ goldens
@pytest.fixture(scope='module')
def restated(goldens):
    """The restatement's outputs on every golden's inputs, computed once."""
    out = {}
    for name, z in goldens.items():
        spec = A.named_spec(name)
        p = A.init_clip_score_params(spec, int(z['seed']))
        images = R.seed_images(int(z['image_seed']), z['tokens'].shape[0], spec.image_size)
        with torch.no_grad():
            fi, vh = R.clip_image_ref(p, images, spec.vision.heads, spec.vision.layers, spec.eps, spec.act)
            ft, th = R.clip_text_pooled_ref(p, torch.from_numpy(z['tokens']), spec.text.heads, spec.text.layers, spec.eps, spec.act)
        out[name] = (spec, p, fi, vh, ft, th)
    return out


@pytest.mark.parametrize('name', list(GOLDENS))
def test_restatement_reproduces_the_goldens(goldens, restated, name):
    z = goldens[name]
    spec, _, fi, vh, ft, th = restated[name]
    rel = lambda a, b, amax: float((a - torch.from_numpy(b)).abs().max()) / float(amax)
    assert rel(fi, z['image_features'], z['image_absmax']) <= 1e-5 and rel(ft, z['text_features'], z['text_absmax']) <= 1e-5
    assert rel(vh[:, z['vision_rows'].tolist()], z['vision_hidden'], z['vision_hidden_absmax']) <= 1e-5
    tr = torch.from_numpy(z['text_rows'])
    assert rel(torch.stack([th[b, tr[b]] for b in range(tr.shape[0])]), z['text_hidden'], z['text_hidden_absmax']) <= 1e-5
    assert float(z['image_absmax']) == float(np.abs(z['image_features']).max()) and float(z['text_absmax']) == float(np.abs(z['text_features']).max())
    s = R.scores_ref(torch.from_numpy(z['image_features']), torch.from_numpy(z['text_features'])).numpy()
    assert np.abs(s - z['scores']).max() <= 1e-9
    fi64, ft64 = z['image_features'].astype(np.float64), z['text_features'].astype(np.float64)
    ratio = lambda f: np.abs(f).max(-1) / np.linalg.norm(f, axis=-1)
    assert np.allclose(z['score_bound'], 100 * EPS * np.sqrt(spec.embed) * (ratio(fi64) + ratio(ft64)), rtol=1e-6)
    assert z['vision_rows'].tolist() == [0, 1, 31, 32, 33, 127, 128, 129, 255, 256]


def test_goldens_carry_the_sensitivity_distances_and_eot_positions(goldens):
    eots = []
    for name, z in goldens.items():
        assert float(z['eps']) == EPS
        assert float(z['quick_gelu_image_dist']) >= 25 * EPS and float(z['quick_gelu_text_dist']) >= 25 * EPS
        for k in ('pool_last_text', 'pool_patch_image', 'no_pre_ln_image'):
            assert float(z[k + '_dist']) >= 50 * EPS, (name, k)
        assert float(z['ref_dist']) <= 1e-5
        t = torch.from_numpy(z['tokens'])
        e = t.argmax(-1)
        assert z['text_rows'][:, :4].tolist() == [[0, 31, 32, 33]] * len(e) and z['text_rows'][:, 4].tolist() == e.tolist()
        eots += e.tolist()
    assert 76 in eots and 10 in eots and any(20 < e < 60 for e in eots)
    assert all(os.path.getsize(os.path.join(ROOT, 'tests', 'golden', f)) < 400_000 for f in GOLDENS.values())


def test_restatement_switches_move_the_output(goldens, restated):
    """The wrong forms the recorded distances are about are the ones the restatement's switches evaluate."""
    z = goldens['tiny_clip_score']
    spec, p, fi, _, ft, _ = restated['tiny_clip_score']
    tokens = torch.from_numpy(z['tokens'])
    with torch.no_grad():
        last = R.clip_text_pooled_ref(p, tokens, spec.text.heads, spec.text.layers, spec.eps, spec.act, pool='last')[0]
    d = float((last - ft).abs().max()) / float(z['text_absmax'])
    assert abs(d - float(z['pool_last_text_dist'])) <= 1e-4 * d
    assert torch.equal(last[0], ft[0])                       # prompt 0 has its end-of-text token at position 76: the last position IS the pool


def test_padding_cannot_reach_the_pooled_text_feature(goldens):
    """Causal mask + pooling at the first end-of-text token: zeros (open_clip) or the end-of-text id (HF) behind it give EQUAL bits."""
    from diff_sampler_amd.clip_score_engine import eot_index
    z = goldens['tiny_clip_score']
    spec = A.named_spec('tiny_clip_score')
    p = A.init_clip_score_params(spec, int(z['seed']))
    t0 = torch.from_numpy(z['tokens']).long()
    e = eot_index(t0)
    t1 = t0.clone()
    for b in range(t0.shape[0]):
        t1[b, int(e[b]) + 1:] = spec.vocab - 1
    assert not torch.equal(t0, t1) and torch.equal(eot_index(t1), e)
    with torch.no_grad():
        f0 = R.clip_text_pooled_ref(p, t0, spec.text.heads, spec.text.layers, spec.eps, spec.act)[0]
        f1 = R.clip_text_pooled_ref(p, t1, spec.text.heads, spec.text.layers, spec.eps, spec.act)[0]
    assert torch.equal(f0, f1)


def test_eot_index_is_the_first_argmax_also_for_a_truncated_prompt(tmp_path):
    from diff_sampler_amd.clip_score_engine import eot_index
    from diff_sampler_amd.clip_tokenizer import ClipTokenizer
    from tests._clip_tok import write_tokenizer
    write_tokenizer(str(tmp_path))
    tok = ClipTokenizer(str(tmp_path))
    t = tok(['hi', 'lower newer ' * 60, ''])
    assert t.shape == (3, 77) and eot_index(t).tolist() == [2, 76, 1]
    assert int(t[1, 76]) == tok.eos and int(t[1, 75]) != tok.eos          # truncated to 77 with the end token last
    assert eot_index(torch.tensor([[5, 9, 9, 0], [9, 1, 2, 3]])).tolist() == [1, 0]


# ------------------------------------------------------------------------------------------------------------------ host preprocessing
def _pil(h, w, seed=0):
    import PIL.Image
    return PIL.Image.fromarray(np.random.RandomState(seed).randint(0, 256, size=(h, w, 3), dtype=np.uint8), 'RGB')


def test_preprocess_geometry():
    import PIL.Image
    chw = lambda im: torch.from_numpy(np.asarray(im).transpose(2, 0, 1).copy())
    im = _pil(224, 224)
    assert torch.equal(CS.preprocess(im), chw(im))
    im = _pil(300, 224, 1)                                               # taller: no resize, rows 38 .. 261
    assert torch.equal(CS.preprocess(im), chw(im)[:, 38:262]) and int(round((300 - 224) / 2)) == 38
    im = _pil(224, 301, 2)                                               # wider by an odd amount: columns 38 .. 261 (round(38.5) = 38)
    assert torch.equal(CS.preprocess(im), chw(im)[:, :, 38:262]) and int(round((301 - 224) / 2)) == 38
    im = _pil(512, 512, 3)
    assert torch.equal(CS.preprocess(im), chw(im.resize((224, 224), PIL.Image.BICUBIC)))
    im = _pil(400, 600, 4)                                               # shorter side to 224, long side int(224 * 600 / 400) = 336, crop 56
    assert torch.equal(CS.preprocess(im), chw(im.resize((336, 224), PIL.Image.BICUBIC))[:, :, 56:280])
    g = CS.preprocess(_pil(224, 224).convert('L'))
    assert g.shape == (3, 224, 224) and g.dtype == torch.uint8 and torch.equal(g[0], g[2])


def test_caption_pairing_and_rank_sharding(tmp_path):
    from diff_sampler_amd import fid
    d = tmp_path / 'imgs'
    d.mkdir()
    for i in range(7):
        _pil(8, 8, i).save(d / f'{i:06d}.png')
    with open(tmp_path / 'c.csv', 'w') as fh:
        fh.write('id,text\n' + ''.join(f'{i},"caption, {i}"\n' for i in range(7)))
    caps = CS.read_captions(str(tmp_path / 'c.csv'))
    assert caps == [f'caption, {i}' for i in range(7)]
    full = fid.ImageFolder(str(d))
    assert CS.pair_captions(full.idx, caps) == caps                       # no subset: the reference's pairing
    sub = fid.ImageFolder(str(d), max_size=4, random_seed=1)
    want = [caps[i] for i in sub.idx.tolist()]
    assert CS.pair_captions(sub.idx, caps) == want and want != caps[:4]   # a subset keeps every image's OWN caption
    with pytest.raises(ValueError):
        CS.pair_captions(full.idx, caps[:6])
    with open(tmp_path / 'bad.csv', 'w') as fh:
        fh.write('id,caption\n0,x\n')
    with pytest.raises(ValueError):
        CS.read_captions(str(tmp_path / 'bad.csv'))
    shards = [fid.shard_items(7, 2, r, 2) for r in range(2)]
    seen = sorted(int(i) for s in shards for b in s for i in b)
    assert seen == list(range(7)) and all(len(b) <= 2 for s in shards for b in s)
    assert CS.result_line('out/run/images', 31.5) == 'run images 31.5\n' and CS.result_line('x', 2.0, 'note') == 'note 2.0\n'


# ------------------------------------------------------------------------------------------------------------------ plans
def _names(plan):
    return [op.name for op in plan.ops]


def test_both_plans_build_on_the_cpu_with_the_expected_launches(libs):
    from diff_sampler_amd.clip_score_engine import ClipImageEncoder, ClipPooledTextEncoder
    lib, mlib = libs
    spec = A.named_spec('tiny_clip_score')
    p = A.init_clip_score_params(spec, 1)
    im = ClipImageEncoder(spec, p, device='cpu')
    P = im.plan(2)
    assert im.plan(2) is P and im.plan(3) is not P                        # one plan per batch size
    n = _names(P)
    L = spec.vision.layers
    assert n[:4] == ['patch_rows', 'patch_embedding', 'tokens', 'pre_layrnorm'] and n[-3:] == ['pool', 'post_layernorm', 'visual_projection']
    assert len(n) == 4 + 8 * L + 3
    assert n[4:12] == [f'vision.layers.0.{x}' for x in ('layer_norm1', 'qkv', 'attention', 'out_proj', 'layer_norm2', 'fc1', 'gelu', 'fc2')]
    by = {op.name: op.fn for op in P.ops}
    assert by['vision.layers.0.attention'] is mlib.dsm_attention and by['vision.layers.1.gelu'] is mlib.dsm_gelu_rows
    assert by['patch_rows'] is mlib.dsm_vit_patch_rows and by['tokens'] is mlib.dsm_vit_tokens and by['pool'] is mlib.dsm_gather_rows
    assert by['vision.layers.0.qkv'] is lib.ds_conv2d_nhwc and by['pre_layrnorm'] is lib.ds_layernorm_rows
    assert tuple(P.bufs['out'].shape) == (2, spec.embed) and tuple(P.bufs['hidden'].shape) == (2 * 257, 352)
    assert P.bufs['images'].dtype == torch.uint8 and im.plan(2, f32=True).bufs['images'].dtype == torch.float32
    assert im.kpad == 608 and im.w['patch.w'].shape[1] == 608 and float(im.w['patch.w'][:, 588:].abs().max()) == 0.0

    tx = ClipPooledTextEncoder(spec, p, device='cpu')
    T = tx.plan(3)
    n = _names(T)
    assert n[0] == 'embeddings' and n[-3:] == ['pool', 'final_layer_norm', 'text_projection'] and len(n) == 1 + 8 * spec.text.layers + 3
    by = {op.name: op.fn for op in T.ops}
    assert by['text.layers.0.attention'] is lib.ds_attention_causal and by['text.layers.0.gelu'] is mlib.dsm_gelu_rows
    assert tuple(T.bufs['out'].shape) == (3, spec.embed)
    with pytest.raises(ValueError):
        tx.check_tokens(torch.full((1, 77), spec.vocab))
    with pytest.raises(ValueError):
        im.check_images(torch.zeros(1, 3, 32, 32, dtype=torch.uint8))


@pytest.mark.parametrize('heads,d', [(4, 88), (5, 64), (4, 80)])
def test_attention_routing_by_head_size(libs, heads, d):
    """d = 88: the metrics library's kernel; head sizes ds_attention covers go there; the OpenAI activation is ds_quick_gelu."""
    from diff_sampler_amd.clip_score_engine import ClipImageEncoder
    lib, mlib = libs
    cfg = dict(A.NAMED_CLIP_SCORE_CONFIGS['tiny_clip_score'], act='quick_gelu')
    cfg['vision'] = dict(cfg['vision'], width=heads * d, heads=heads, layers=1, ffn=64)
    spec = A.clip_score_spec(**cfg)
    P = ClipImageEncoder(spec, A.init_clip_score_params(spec, 0), device='cpu').plan(1)
    by = {op.name: op.fn for op in P.ops}
    assert by['vision.layers.0.attention'] is (mlib.dsm_attention if d == 88 else lib.ds_attention)
    assert by['vision.layers.0.quick_gelu'] is lib.ds_quick_gelu


def test_geometry_without_a_kernel_is_refused_at_build_time(libs):
    from diff_sampler_amd.clip_score_engine import ClipImageEncoder, ClipPooledTextEncoder
    cfg = dict(A.NAMED_CLIP_SCORE_CONFIGS['tiny_clip_score'])
    bad_v = A.clip_score_spec(**dict(cfg, vision=dict(cfg['vision'], width=4 * 72, heads=4)))       # head size 72: neither library
    with pytest.raises(NotImplementedError):
        ClipImageEncoder(bad_v, A.init_clip_score_params(bad_v, 0), device='cpu')
    bad_t = A.clip_score_spec(**dict(cfg, text=dict(cfg['text'], width=160, heads=2)))              # causal kernel: head size 64 only
    with pytest.raises(NotImplementedError):
        ClipPooledTextEncoder(bad_t, A.init_clip_score_params(bad_t, 0), device='cpu')


# ------------------------------------------------------------------------------------------------------------------ library surface
def test_new_entry_points_reject_bad_arguments_on_the_host(libs):
    from diff_sampler_amd._metrics_lib import DS_E_ALIGN, DS_E_ARG, DS_E_SHAPE, DsmAttnArgs, DSM_VERSION
    _, m = libs
    assert m.dsm_version() == DSM_VERSION == 2
    buf = (C.c_float * 4096)()
    base = (C.addressof(buf) + 63) & ~63
    p, off = C.c_void_p(base), C.c_void_p(base + 4)                       # 64-byte aligned / 4 bytes beyond
    f3 = (C.c_float * 3)(1, 1, 1)
    z3 = (C.c_float * 3)(1, 0, 1)

    def attn(**kw):
        a = dict(q=base, k=base, v=base, out=base, ldq=1064, ldk=1064, ldv=1064, ldo=352, q_bs=8, k_bs=8, v_bs=8, o_bs=8, batch=1, heads=4,
                 sq=5, skv=5, d=88, scale=0.1)
        a.update(kw)
        return m.dsm_attention(C.byref(DsmAttnArgs(**a)), None)

    assert m.dsm_attention(None, None) == DS_E_ARG
    assert attn(q=None) == attn(k=None) == attn(v=None) == attn(out=None) == DS_E_ARG
    assert attn(sq=0) == attn(skv=0) == attn(batch=0) == attn(heads=0) == attn(batch=65536) == DS_E_ARG
    assert attn(ldo=348) == attn(ldq=351) == DS_E_ARG                     # ld < heads * d
    assert attn(ldq=1066) == attn(q_bs=6) == attn(out=base + 4) == attn(k=base + 8) == DS_E_ALIGN
    for d in (64, 80, 96, 87, 0):
        assert attn(d=d) == DS_E_SHAPE and m.dsm_attention_supported(d) == 0
    assert m.dsm_attention_supported(88) == 1

    gelu = lambda x=p, ldx=8, y=p, ldy=8, rows=2, cols=8: m.dsm_gelu_rows(x, ldx, y, ldy, rows, cols, None)
    assert gelu(x=None) == gelu(y=None) == gelu(rows=0) == gelu(cols=0) == gelu(ldx=4) == gelu(ldy=4) == DS_E_ARG
    assert gelu(cols=6) == gelu(ldx=10) == gelu(x=off) == gelu(y=off) == DS_E_ALIGN

    patch = lambda img=p, f32=0, n=1, size=28, pt=14, mean=f3, std=f3, out=p, ld=608: m.dsm_vit_patch_rows(img, f32, n, size, pt, mean, std, out, ld, None)
    assert patch(img=None) == patch(out=None) == patch(mean=None) == patch(std=None) == patch(n=0) == patch(size=0) == patch(pt=0) == DS_E_ARG
    assert patch(ld=587) == patch(f32=2) == patch(std=z3) == DS_E_ARG
    assert patch(size=30) == DS_E_SHAPE and patch(out=off) == DS_E_ALIGN

    tok = lambda pe=p, ldp=8, cls=p, pos=p, out=p, ldo=8, n=1, t=5, w=8: m.dsm_vit_tokens(pe, ldp, cls, pos, out, ldo, n, t, w, None)
    assert tok(pe=None) == tok(cls=None) == tok(pos=None) == tok(out=None) == tok(n=0) == tok(t=1) == tok(w=0) == tok(ldp=4) == tok(ldo=4) == DS_E_ARG
    assert tok(w=6, ldp=8) == tok(ldo=10) == tok(cls=off) == tok(out=off) == DS_E_ALIGN

    gat = lambda x=p, ldx=8, xr=4, idx=p, out=p, ldo=8, n=2, cols=8: m.dsm_gather_rows(x, ldx, xr, idx, out, ldo, n, cols, None)
    assert gat(x=None) == gat(idx=None) == gat(out=None) == gat(xr=0) == gat(n=0) == gat(cols=0) == gat(ldx=4) == gat(ldo=4) == DS_E_ARG
    assert gat(cols=6) == gat(ldx=10) == gat(x=off) == gat(out=off) == DS_E_ALIGN and gat(xr=1 << 31) == DS_E_SHAPE

    sc = lambda a=p, lda=8, b=p, ldb=8, n=2, dim=8, s=p, tot=p: m.dsm_clip_score(a, lda, b, ldb, n, dim, s, tot, None)
    assert sc(a=None) == sc(b=None) == sc(s=None) == sc(tot=None) == sc(n=0) == sc(dim=0) == sc(lda=7) == sc(ldb=7) == DS_E_ARG
    assert sc(tot=off) == sc(a=C.c_void_p(base + 2)) == DS_E_ALIGN


def test_d88_attention_kernel_needs_no_scratch():
    """The 44 + 48 + 16 + 24 live registers of the d = 88 tile fit: no private memory (the precedent: tests/test_abi_cpu.py)."""
    import shutil
    import subprocess
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    src = os.path.join(ROOT, 'diff_sampler_amd', 'csrc', 'metrics', 'clip_score.hip')
    r = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-c', src, '-o', os.devnull, '-Rpass-analysis=kernel-resource-usage'],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    found = re.findall(r'Function Name: (\S*attn88_kernel\S*).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)',
                       r.stderr, flags=re.S)
    assert len(found) == 1, r.stderr[-1500:]
    _, vgpr, agpr, scratch, occ = found[0]
    print(f'attn88_kernel: VGPRs {vgpr}, AGPRs {agpr}, scratch {scratch}, occupancy {occ} waves/SIMD')
    assert int(scratch) == 0 and int(vgpr) + int(agpr) <= 256
