#!/usr/bin/env python
"""Record the CLIP-score goldens tests/golden/clip_score_*.npz from the REAL class, on the CPU.

    python tools/gen_clip_score_golden.py [tiny] [vitg2l]

The reference's clip_score.py runs open_clip's ViT-g-14; transformers' ``CLIPModel`` is the same two-tower network with a public
architecture.  It is built here from a ``CLIPConfig`` holding the numbers of ``clip_score_arch.NAMED_CLIP_SCORE_CONFIGS`` (never
``from_pretrained``: nothing is downloaded); the weights ``clip_score_arch.init_clip_score_params(spec, seed)`` are loaded with
``strict=True`` (plus the class's own ``logit_scale``), so the key names and shapes of our table are pinned to the real class.  The goldens
hold the seed, the token ids, the seed of the uint8 images (tests/_clip_vit_ref.py ``seed_images``) and recorded outputs only:

  image_features / text_features   get_image_features / get_text_features, and their absmax
  vision_hidden / text_hidden      the last encoder layer's hidden state at VISION_ROWS (both sides of the 32-key tile borders of the 257
                                   tokens, the class row, the ragged last row) and at TEXT_ROWS + the end-of-text row of every prompt
  scores                           100 cos per pair in fp64 from the fp32 features
  score_bound                      100 eps sqrt(E) (max|a| / |a| + max|b| / |b|), eps = 2e-4: the first-order effect on a cosine of a feature
                                   error of eps * absmax per element

Prompts: start token, random ids, the end-of-text token (the largest id) at EOT_AT, zeros behind it (open_clip's padding).

Every golden also records how far WRONG evaluations of the same weights land from it (tests/_clip_vit_ref.py; max |a - b| / absmax), and
this script fails unless they clear their thresholds -- a kernel with one of these mistakes cannot pass the 2e-4 test:
  quick_gelu for erf-GELU (both towers)          >= 25 x eps   (6e-3 ... 1.6e-2 over seeds at the tiny geometry: 50 x does not hold for both)
  text pooled at the last position               >= 50 x eps
  vision pooled from patch row 1                 >= 50 x eps
  no pre_layrnorm                                >= 50 x eps
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

# case -> (config, seed, EOT positions (one per prompt), file); the assertions in make() hold the seeds to the thresholds
CASES = {'tiny': ('tiny_clip_score', 3, (76, 10, 40), 'clip_score_tiny.npz'),
         'vitg2l': ('vit_g_14_2l', 5, (76, 10), 'clip_score_vitg2l.npz')}
VISION_ROWS = [0, 1, 31, 32, 33, 127, 128, 129, 255, 256]
TEXT_ROWS = [0, 31, 32, 33]
EPS = 2e-4


def real_model(spec):
    from transformers import CLIPConfig, CLIPModel
    text = dict(vocab_size=spec.vocab, hidden_size=spec.text.width, intermediate_size=spec.text.ffn, num_hidden_layers=spec.text.layers,
                num_attention_heads=spec.text.heads, max_position_embeddings=spec.positions, hidden_act=spec.act, layer_norm_eps=spec.eps,
                attention_dropout=0.0, bos_token_id=spec.vocab - 2, eos_token_id=spec.vocab - 1, pad_token_id=0, projection_dim=spec.embed)
    vision = dict(hidden_size=spec.vision.width, intermediate_size=spec.vision.ffn, num_hidden_layers=spec.vision.layers,
                  num_attention_heads=spec.vision.heads, image_size=spec.image_size, patch_size=spec.patch, hidden_act=spec.act,
                  layer_norm_eps=spec.eps, attention_dropout=0.0, projection_dim=spec.embed)
    return CLIPModel(CLIPConfig(text_config=text, vision_config=vision, projection_dim=spec.embed)).eval()


def load_strict(model, params):
    sd = dict(params)
    for k, v in model.state_dict().items():
        if k == 'logit_scale' or k.endswith('position_ids'):
            sd[k] = v
    model.load_state_dict(sd, strict=True)


def _features(out):
    return (out if torch.is_tensor(out) else out.pooler_output).float()


def make_tokens(spec, seed, eot_at):
    g = torch.Generator().manual_seed(seed + 1000)
    tokens = torch.randint(1, spec.vocab - 2, (len(eot_at), spec.positions), generator=g)
    tokens[:, 0] = spec.vocab - 2
    for b, e in enumerate(eot_at):
        tokens[b, e] = spec.vocab - 1
        tokens[b, e + 1:] = 0
    return tokens


def make(case):
    import diff_sampler_amd.clip_score_arch as A
    import _clip_vit_ref as R
    name, seed, eot_at, fname = CASES[case]
    spec = A.named_spec(name)
    params = A.init_clip_score_params(spec, seed=seed)
    B = len(eot_at)
    tokens = make_tokens(spec, seed, eot_at)
    image_seed = seed + 2000
    images = R.seed_images(image_seed, B, spec.image_size)
    V, T = spec.vision, spec.text
    with torch.no_grad():
        m = real_model(spec)
        load_strict(m, params)
        pixels = R.normalise_images(images)
        fi = _features(m.get_image_features(pixel_values=pixels))
        ft = _features(m.get_text_features(input_ids=tokens))
        vh = m.vision_model(pixel_values=pixels, output_hidden_states=True).hidden_states[-1].float()
        th = m.text_model(input_ids=tokens, output_hidden_states=True).hidden_states[-1].float()
        ri, rvh = R.clip_image_ref(params, images, V.heads, V.layers, spec.eps, spec.act)
        rt, rth = R.clip_text_pooled_ref(params, tokens, T.heads, T.layers, spec.eps, spec.act)
        wrong = dict(quick_gelu_image=R.clip_image_ref(params, images, V.heads, V.layers, spec.eps, 'quick_gelu')[0],
                     quick_gelu_text=R.clip_text_pooled_ref(params, tokens, T.heads, T.layers, spec.eps, 'quick_gelu')[0],
                     pool_last_text=R.clip_text_pooled_ref(params, tokens, T.heads, T.layers, spec.eps, spec.act, pool='last')[0],
                     pool_patch_image=R.clip_image_ref(params, images, V.heads, V.layers, spec.eps, spec.act, pool='patch')[0],
                     no_pre_ln_image=R.clip_image_ref(params, images, V.heads, V.layers, spec.eps, spec.act, pre_ln=False)[0])
    ai, at = float(fi.abs().max()), float(ft.abs().max())
    dist = lambda t, ref, amax: float((t - ref).abs().max()) / amax
    d = {k: dist(v, fi if k.endswith('image') else ft, ai if k.endswith('image') else at) for k, v in wrong.items()}
    need = dict(quick_gelu_image=25, quick_gelu_text=25, pool_last_text=50, pool_patch_image=50, no_pre_ln_image=50)
    bad = {k: (v, need[k] * EPS) for k, v in d.items() if v < need[k] * EPS}
    assert not bad, (case, seed, bad, 'this seed gives a wrong form too little weight: choose another')
    ref_dist = max(dist(ri, fi, ai), dist(rt, ft, at), dist(rvh, vh, float(vh.abs().max())), dist(rth, th, float(th.abs().max())))
    assert ref_dist <= 1e-5, ('the restatement does not reproduce the real class', ref_dist)
    eot = tokens.argmax(-1)
    assert eot.tolist() == list(eot_at)
    trows = [TEXT_ROWS + [int(e)] for e in eot]
    E = spec.embed
    ratio = lambda f: (f.abs().max(-1).values / f.norm(dim=-1)).double()
    out = dict(config=name, seed=seed, image_seed=image_seed, tokens=tokens.numpy().astype(np.int32), eps=np.float64(EPS),
               image_features=fi.numpy(), text_features=ft.numpy(), image_absmax=np.float64(ai), text_absmax=np.float64(at),
               vision_rows=np.array(VISION_ROWS), vision_hidden=vh[:, VISION_ROWS].numpy(), vision_hidden_absmax=np.float64(vh.abs().max()),
               text_rows=np.array(trows), text_hidden=torch.stack([th[b, trows[b]] for b in range(B)]).numpy(),
               text_hidden_absmax=np.float64(th.abs().max()),
               scores=R.scores_ref(fi, ft).numpy(), score_bound=(100.0 * EPS * np.sqrt(E) * (ratio(fi) + ratio(ft))).numpy(),
               ref_dist=np.float64(ref_dist), **{k + '_dist': np.float64(v) for k, v in d.items()})
    path = os.path.join(OUT, fname)
    np.savez_compressed(path, **out)
    print(fname, 'features', tuple(fi.shape), 'absmax %.3f / %.3f' % (ai, at), 'restatement %.2e' % ref_dist,
          ' '.join('%s %.2e' % kv for kv in d.items()), 'scores', np.round(out['scores'], 3), '%d bytes' % os.path.getsize(path))


if __name__ == '__main__':
    torch.manual_seed(0)
    for c in (sys.argv[1:] or list(CASES)):
        make(c)
