"""A torch-functional restatement of the EDM SongUNet forward with the NCSN++ options (test infrastructure, written from the layer list of
``arch.UNetSpec``; networks_edm.py:312-355 is what it restates, for fp32 and fp64 alike), and the depthwise FIR references of the resampling
kernel written the way ``Conv2d.forward`` (networks_edm.py:60-82) writes them.

``edm_ncsnpp(params, spec, x, sigma, labels)`` -> D(x; sigma) with weights keyed like the reference state dict (``arch.init_params``).
    dtype        torch.float32 makes the ATen calls the reference makes (tests/test_ncsnpp_cpu.py holds it to the goldens at 1e-6, observed 0);
                 torch.float64 is the reference of the per-element kernel bounds.
    taps         a dict that receives every skip-stack tensor under its layer's name, AFTER the aux replacement
                 (``enc.RxR_aux_residual`` is the entry that replaced ``enc.RxR_down``'s).
    emb_rows     [B, noise_channels] rows to use INSTEAD of the computed sin | cos embedding (the device's own rows: tells an embedding
                 difference from any other).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F


def filter2d(taps, dtype=torch.float32, device='cpu'):
    """The reference's ``resample_filter`` buffer [1, 1, k, k]: f (x) f / (sum f)^2, formed in fp32 (networks_edm.py:56-57), then cast."""
    f = torch.as_tensor(list(taps), dtype=torch.float32)
    return (f.ger(f).unsqueeze(0).unsqueeze(1) / f.sum().square()).to(device=device, dtype=dtype)


def fir_down(x, taps, pad):
    """NCHW depthwise stride-2 filter; pad = 1: the stand-alone form (networks_edm.py:77), pad = 0: the second half of fused_resample (:72)."""
    c = x.shape[1]
    return F.conv2d(x, filter2d(taps, x.dtype, x.device).tile([c, 1, 1, 1]), groups=c, stride=2, padding=pad)


def fir_up(x, taps):
    """NCHW depthwise x2 upsampling: conv_transpose2d with 4 f2d, stride 2, padding (k - 1) // 2 (networks_edm.py:75)."""
    c = x.shape[1]
    f = filter2d(taps, x.dtype, x.device)
    return F.conv_transpose2d(x, f.mul(4).tile([c, 1, 1, 1]), groups=c, stride=2, padding=(f.shape[-1] - 1) // 2)


def _linear(p, key, x):
    y = x @ p[f'{key}.weight'].t()
    if f'{key}.bias' in p:
        y = y.add_(p[f'{key}.bias'])
    return y


def _conv(p, key, x, taps, up=False, down=False, fused=False):
    """Conv2d.forward: optional resampling around an optional kernel (no ``.weight`` under `key`: the filter alone)."""
    w, b = p.get(f'{key}.weight'), p.get(f'{key}.bias')
    w_pad = w.shape[-1] // 2 if w is not None else 0
    f_pad = (len(taps) - 1) // 2
    if fused and down and w is not None:
        x = F.conv2d(x, w, padding=w_pad + f_pad)
        x = fir_down(x, taps, 0)
    else:
        if up:
            x = fir_up(x, taps)
        if down:
            x = fir_down(x, taps, f_pad)
        if w is not None:
            x = F.conv2d(x, w, padding=w_pad)
    if b is not None:
        x = x.add_(b.reshape(1, -1, 1, 1))
    return x


def _gn(p, key, x, eps):
    c = x.shape[1]
    return F.group_norm(x, num_groups=min(32, c // 4), weight=p[f'{key}.weight'], bias=p[f'{key}.bias'], eps=eps)


def _block(p, b, spec, x, emb):
    key, taps = f'model.{b.name}', spec.resample_filter
    orig = x
    x = _conv(p, f'{key}.conv0', F.silu(_gn(p, f'{key}.norm0', x, b.eps)), taps, up=b.up, down=b.down)
    params = _linear(p, f'{key}.affine', emb).unsqueeze(2).unsqueeze(3)
    assert not b.adaptive_scale
    x = F.silu(_gn(p, f'{key}.norm1', x.add_(params), b.eps))
    x = _conv(p, f'{key}.conv1', x, taps)
    if b.skip_conv or b.up or b.down:
        x = x.add_(_conv(p, f'{key}.skip', orig, taps, up=b.up, down=b.down))
    else:
        x = x.add_(orig)
    x = x * b.skip_scale
    if b.heads:
        n, c = x.shape[0] * b.heads, x.shape[1] // b.heads
        q, k, v = _conv(p, f'{key}.qkv', _gn(p, f'{key}.norm2', x, b.eps), taps).reshape(n, c, 3, -1).unbind(2)
        w = torch.einsum('ncq,nck->nqk', q, k / np.sqrt(k.shape[1])).softmax(dim=2)
        a = torch.einsum('nqk,nck->ncq', w, v)
        x = _conv(p, f'{key}.proj', a.reshape(*x.shape), taps).add_(x)
        x = x * b.skip_scale
    return x


def embedding_rows(p, spec, c_noise):
    """[B, noise_channels] = [sin | cos] of the noise embedding (SongUNet flips the [cos | sin] of both embedding types)."""
    half = spec.noise_channels // 2
    if spec.embedding_type == 'fourier':
        freqs = (2 * np.pi * p['model.map_noise.freqs']).to(c_noise.dtype)
    else:
        freqs = torch.arange(start=0, end=half, dtype=torch.float32, device=c_noise.device)
        freqs = freqs / (half - (1 if spec.pos_endpoint else 0))
        freqs = ((1 / spec.pos_max_positions) ** freqs).to(c_noise.dtype)
    e = c_noise.ger(freqs)
    e = torch.cat([e.cos(), e.sin()], dim=1)
    return e.reshape(e.shape[0], 2, -1).flip(1).reshape(*e.shape)


def song_unet(p, spec, x, c_noise, labels=None, taps=None, emb_rows=None):
    emb = embedding_rows(p, spec, c_noise) if emb_rows is None else emb_rows.to(x.dtype)
    if spec.label_dim:
        emb = emb + _linear(p, 'model.map_label', labels * np.sqrt(spec.label_dim))
    emb = F.silu(_linear(p, 'model.map_layer0', emb))
    emb = F.silu(_linear(p, 'model.map_layer1', emb))
    skips, names, aux = [], [], x
    for b in spec.enc:
        if b.kind == 'aux':
            x = skips[-1] = aux = (x + _conv(p, f'model.{b.name}', aux, spec.resample_filter, down=True, fused=True)) / np.sqrt(2)
            names[-1] = b.name
        else:
            x = _conv(p, f'model.{b.name}', x, spec.resample_filter) if b.kind == 'conv' else _block(p, b, spec, x, emb)
            skips.append(x)
            names.append(b.name)
    if taps is not None:
        taps.update({n: t.clone() for n, t in zip(names, skips)})
    for b in spec.dec:
        if b.pops_skip:
            x = torch.cat([x, skips.pop()], dim=1)
        x = _block(p, b, spec, x, emb)
    x = F.silu(_gn(p, f'model.{spec.out_norm}', x, spec.out_eps))
    return _conv(p, f'model.{spec.out_conv}', x, spec.resample_filter)


def edm_ncsnpp(params, spec, x, sigma, labels=None, dtype=torch.float32, taps=None, emb_rows=None):
    """EDMPrecond.forward (networks_edm.py:482-496) around ``song_unet``; the preconditioning coefficients are fp32 expressions there."""
    with torch.no_grad():
        p = {k: v.to(dtype) for k, v in params.items()}
        x = x.to(torch.float32)
        sigma = torch.as_tensor(sigma).to(torch.float32).reshape(-1, 1, 1, 1)
        if spec.label_dim:
            labels = torch.zeros([1, spec.label_dim], device=x.device) if labels is None else labels.to(torch.float32).reshape(-1, spec.label_dim)
        sd = spec.sigma_data
        c_skip = sd ** 2 / (sigma ** 2 + sd ** 2)
        c_out = sigma * sd / (sigma ** 2 + sd ** 2).sqrt()
        c_in = 1 / (sd ** 2 + sigma ** 2).sqrt()
        c_noise = sigma.log() / 4
        f_x = song_unet(p, spec, (c_in * x).to(dtype), c_noise.flatten().to(dtype), None if labels is None else labels.to(dtype), taps, emb_rows)
        return c_skip.to(dtype) * x.to(dtype) + c_out.to(dtype) * f_x


# ---- NHWC-row references of the two kernels (fp64) ----------------------------------------------------------------------------------------
def fir_rows_ref(x_rows, n, h, w, c, taps, up, pad, bias=None, res_rows=None, scale=1.0):
    """(out rows, magnitude rows) in fp64 of dsm_fir_resample on x_rows [n*h*w, >= c]: out = (fir + bias + res) * scale, and
    mag = (sum |tap x| + |bias| + |res|) |scale| -- the quantity the kernel's rounding bound is stated in."""
    x = x_rows[:, :c].double().reshape(n, h, w, c).permute(0, 3, 1, 2)
    fn = (lambda t: fir_up(t, taps)) if up else (lambda t: fir_down(t, taps, pad))
    y, m = fn(x), fn(x.abs())          # the 2-D weights are positive for [1,1] and [1,3,3,1]
    to_rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, c)
    y, m = to_rows(y), to_rows(m)
    if bias is not None:
        y, m = y + bias.double(), m + bias.double().abs()
    if res_rows is not None:
        y, m = y + res_rows[:, :c].double(), m + res_rows[:, :c].double().abs()
    return y * scale, m * abs(scale)


def fir_bound(mag, up):
    """Per-element bound of the fp32 kernel against fp64: one rounding per tap FMA (16 down, 4 up) + bias add, residual add, scale."""
    return ((4 if up else 16) + 3) * 2.0 ** -24 * mag


def assert_close_rows(got, ref, bound, what):
    err = (got.double() - ref).abs()
    bad = err > bound
    assert not bool(bad.any()), (what, int(bad.sum()), float(err.max()), float((err / bound.clamp_min(1e-300)).max()))
    return float((err / bound.clamp_min(1e-300)).max())
