"""Both CLIP towers (transformers CLIPModel.get_image_features / get_text_features) restated in plain torch: the checker of
tests/test_clip_score_cpu.py and tests/test_hip_clip_score.py and the stock-PyTorch yardstick of tools/time_clip_score.py.  The switches
evaluate the WRONG forms the goldens' sensitivity conditions are about: `act` (quick_gelu for erf-GELU), `pool` ('last' position instead of
the end-of-text token; 'patch' row 1 instead of the class row), `pre_ln=False` (no pre_layrnorm)."""
import torch
import torch.nn.functional as F

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def _layers(sd, prefix, x, heads, layers, eps, act, causal):
    g = lambda k: sd[prefix + k].to(x.dtype)
    B, S, W = x.shape
    d = W // heads
    mask = torch.full((S, S), float('-inf'), dtype=x.dtype, device=x.device).triu(1) if causal else 0
    for i in range(layers):
        p = f'encoder.layers.{i}.'
        lin = lambda n, t: F.linear(t, g(p + n + '.weight'), g(p + n + '.bias'))
        h = F.layer_norm(x, (W,), g(p + 'layer_norm1.weight'), g(p + 'layer_norm1.bias'), eps)
        q, k, v = (lin('self_attn.' + n, h).view(B, S, heads, d).transpose(1, 2) for n in ('q_proj', 'k_proj', 'v_proj'))
        a = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5 + mask, dim=-1) @ v
        x = x + lin('self_attn.out_proj', a.transpose(1, 2).reshape(B, S, W))
        h = lin('mlp.fc1', F.layer_norm(x, (W,), g(p + 'layer_norm2.weight'), g(p + 'layer_norm2.bias'), eps))
        h = h * torch.sigmoid(1.702 * h) if act == 'quick_gelu' else F.gelu(h)
        x = x + lin('mlp.fc2', h)
    return x


def normalise_images(images, dtype=torch.float32):
    """uint8 (or float in [0, 1]) [B, 3, S, S] -> (v / 255 - mean) / std."""
    x = images.to(dtype) / 255.0 if images.dtype == torch.uint8 else images.to(dtype)
    mean = torch.tensor(CLIP_MEAN, dtype=dtype, device=x.device).view(1, 3, 1, 1)
    std = torch.tensor(CLIP_STD, dtype=dtype, device=x.device).view(1, 3, 1, 1)
    return (x - mean) / std


def clip_image_ref(sd, images, heads, layers, eps=1e-5, act='gelu', pool='class', pre_ln=True, dtype=torch.float32):
    """-> (features [B, embed], last encoder layer's hidden state [B, tokens, width])."""
    g = lambda k: sd['vision_model.' + k].to(dtype)
    x = normalise_images(images.to(g('post_layernorm.weight').device), dtype)
    wp = g('embeddings.patch_embedding.weight')
    W = wp.shape[0]
    pe = F.conv2d(x, wp, stride=wp.shape[-1]).flatten(2).transpose(1, 2)
    x = torch.cat([g('embeddings.class_embedding').expand(pe.shape[0], 1, W), pe], 1) + g('embeddings.position_embedding.weight')
    if pre_ln:
        x = F.layer_norm(x, (W,), g('pre_layrnorm.weight'), g('pre_layrnorm.bias'), eps)
    x = _layers(sd, 'vision_model.', x, heads, layers, eps, act, False)
    pooled = F.layer_norm(x[:, 1 if pool == 'patch' else 0], (W,), g('post_layernorm.weight'), g('post_layernorm.bias'), eps)
    return F.linear(pooled, sd['visual_projection.weight'].to(dtype)), x


def clip_text_pooled_ref(sd, tokens, heads, layers, eps=1e-5, act='gelu', pool='eot', dtype=torch.float32):
    """-> (features [B, embed], last encoder layer's hidden state [B, 77, width]); pooled at the first argmax(ids)."""
    g = lambda k: sd['text_model.' + k].to(dtype)
    tokens = torch.as_tensor(tokens).long().to(g('final_layer_norm.weight').device)
    B, S = tokens.shape
    x = g('embeddings.token_embedding.weight')[tokens] + g('embeddings.position_embedding.weight')[:S]
    W = x.shape[-1]
    x = _layers(sd, 'text_model.', x, heads, layers, eps, act, True)
    at = torch.full((B,), S - 1, device=x.device) if pool == 'last' else tokens.argmax(dim=-1)
    pooled = F.layer_norm(x[torch.arange(B, device=x.device), at], (W,), g('final_layer_norm.weight'), g('final_layer_norm.bias'), eps)
    return F.linear(pooled, sd['text_projection.weight'].to(dtype)), x


def scores_ref(fi, ft):
    """100 cos per pair in fp64 from the given features."""
    a, b = fi.double(), ft.double()
    return 100.0 * (a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1))


def seed_images(seed, B, size=224):
    """The goldens' uint8 images: a smooth random field per image and channel plus noise (so resampled patches differ and pixels span 0..255)."""
    g = torch.Generator().manual_seed(int(seed))
    low = torch.rand(B, 3, 8, 8, generator=g)
    x = F.interpolate(low, size=(size, size), mode='bilinear', align_corners=False) * 0.8 + torch.rand(B, 3, size, size, generator=g) * 0.2
    return (x * 255.0).round().clamp(0, 255).to(torch.uint8)
