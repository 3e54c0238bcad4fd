"""The CLIP text encoder (transformers CLIPTextModel(...).last_hidden_state) restated in plain torch: the checker of tests/test_clip_cpu.py
and tests/test_hip_text_encoder.py, and the stock-PyTorch yardstick of tools/time_text_encoder.py.  `causal` / `act` exist so that the
goldens' sensitivity condition (no mask, erf-GELU) can be evaluated."""
import torch
import torch.nn.functional as F


def clip_text_ref(sd, tokens, heads, layers, eps=1e-5, causal=True, act='quick_gelu', dtype=torch.float32):
    g = lambda k: sd['text_model.' + k].to(dtype)
    tokens = torch.as_tensor(tokens).long().to(sd['text_model.final_layer_norm.weight'].device)
    B, S = tokens.shape
    x = g('embeddings.token_embedding.weight')[tokens] + g('embeddings.position_embedding.weight')[:S]
    W = x.shape[-1]
    d = W // heads
    mask = torch.full((S, S), float('-inf'), dtype=dtype, device=x.device).triu(1) if causal else 0
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
    return F.layer_norm(x, (W,), g('final_layer_norm.weight'), g('final_layer_norm.bias'), eps)
