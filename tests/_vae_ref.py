"""CPU restatement of the AutoencoderKL decode path (``decode_first_stage``: z / scale_factor -> post_quant_conv -> Decoder) in plain
torch, driven by ``vae_arch.VAEDecoderSpec`` and a state_dict with the reference's key names.  Our own code in the style of
oracle/ldm_net.py; it is pinned to the real classes (ldm/modules/diffusionmodules/model.py ``Decoder``, autoencoder.py
``post_quant_conv``) by the goldens tests/golden/vae_*.npz, which tools/gen_vae_golden.py records from them."""
import torch
import torch.nn.functional as F


def _gn_swish(x, p, key, swish=True):
    h = F.group_norm(x, 32, p[f'{key}.weight'], p[f'{key}.bias'], eps=1e-6)
    return h * torch.sigmoid(h) if swish else h


def _conv(x, p, key, pad):
    return F.conv2d(x, p[f'{key}.weight'], p[f'{key}.bias'], padding=pad)


def _res(x, p, key, cin, cout):
    h = _conv(_gn_swish(x, p, f'{key}.norm1'), p, f'{key}.conv1', 1)
    h = _conv(_gn_swish(h, p, f'{key}.norm2'), p, f'{key}.conv2', 1)
    if cin != cout:
        x = _conv(x, p, f'{key}.nin_shortcut', 0)
    return x + h


def _attn(x, p, key):
    b, c, hh, ww = x.shape
    n = _gn_swish(x, p, f'{key}.norm', swish=False)
    q, k, v = (_conv(n, p, f'{key}.{t}', 0).reshape(b, c, hh * ww) for t in 'qkv')
    wgt = torch.softmax(torch.bmm(q.transpose(1, 2), k) * (int(c) ** -0.5), dim=2)        # [b, query, key]
    o = torch.bmm(v, wgt.transpose(1, 2)).reshape(b, c, hh, ww)
    return x + _conv(o, p, f'{key}.proj_out', 0)


def decode(spec, params, z):
    """z [B, z_channels, R, R] -> image [B, out_ch, 8 R, 8 R] (fp32 or fp64, following the dtype of `params` and `z`)."""
    p = params
    h = _conv(z / spec.scale_factor, p, 'post_quant_conv', 0)
    for l in spec.layers:
        if l.kind == 'conv_in':
            h = _conv(h, p, l.key, 1)
        elif l.kind == 'res':
            h = _res(h, p, l.key, l.cin, l.cout)
        elif l.kind == 'attn':
            h = _attn(h, p, l.key)
        elif l.kind == 'up':
            h = _conv(F.interpolate(h, scale_factor=2.0, mode='nearest'), p, f'{l.key}.conv', 1)
        elif l.kind == 'conv_out':
            h = _conv(_gn_swish(h, p, 'decoder.norm_out'), p, l.key, 1)
    return h


def quantize_u8(x):
    """The reference's image quantisation (sample.py:311): (x * 127.5 + 128).clip(0, 255).to(uint8), NHWC."""
    return (x * 127.5 + 128).clip(0, 255).to(torch.uint8).permute(0, 2, 3, 1)
