"""A torch-functional restatement of SFD's step-conditioned EDM networks (test infrastructure, written from the layer list of ``arch.UNetSpec``;
what it restates is sfd-main/models/networks_edm.py:166-202 UNetBlock, :339-399 SongUNet, :475-520 DhariwalUNet, :549-570 EDMPrecond), and the
fp32 emulation / fp64 reference / rounding bound of the one kernel the feature adds (``DS_OP_AFFINE_COMPOSE``).

``edm_sfd(params, spec, x, sigma, labels, step)`` -> D(x; sigma) with weights keyed like the reference state dict (``arch.init_params`` of a
spec with ``step_condition``).  ``step`` None is the plain network: the ``map_step*`` / ``affine_step`` weights are not touched.  The layers both
families share come from tests/_ncsnpp_ref.py.
"""
import numpy as np
import torch
import torch.nn.functional as F

from _ncsnpp_ref import _conv, _gn, _linear


def embedding_rows(p, spec, v, which='noise'):
    """[rows, noise_channels] sin / cos embedding of `v` through ``map_noise`` or ``map_step`` (a FourierEmbedding has a buffer per module);
    SongUNet flips [cos | sin] to [sin | cos] for both (networks_edm.py:342, :356), DhariwalUNet does not."""
    half = spec.noise_channels // 2
    if spec.embedding_type == 'fourier':
        freqs = (2 * np.pi * p[f'model.map_{which}.freqs']).to(v.dtype)
    else:
        freqs = torch.arange(start=0, end=half, dtype=torch.float32, device=v.device)
        freqs = freqs / (half - (1 if spec.pos_endpoint else 0))
        freqs = ((1 / spec.pos_max_positions) ** freqs).to(v.dtype)
    e = v.ger(freqs)
    e = torch.cat([e.cos(), e.sin()], dim=1)
    if spec.swap_sincos:
        e = e.reshape(e.shape[0], 2, -1).flip(1).reshape(*e.shape)
    return e


def _block(p, b, spec, x, emb, emb_step):
    key, taps = f'model.{b.name}', spec.resample_filter
    orig = x
    x = _conv(p, f'{key}.conv0', F.silu(_gn(p, f'{key}.norm0', x, b.eps)), taps, up=b.up, down=b.down)
    params = _linear(p, f'{key}.affine', emb).unsqueeze(2).unsqueeze(3)
    step = None if emb_step is None else _linear(p, f'{key}.affine_step', emb_step).unsqueeze(2).unsqueeze(3)
    if b.adaptive_scale:
        scale, shift = params.chunk(chunks=2, dim=1)
        x = torch.addcmul(shift, _gn(p, f'{key}.norm1', x, b.eps), scale + 1)
        if step is not None:          # the second affine acts on the first one's result (networks_edm.py:176-179)
            scale_step, shift_step = step.chunk(chunks=2, dim=1)
            x = torch.addcmul(shift_step, x, scale_step + 1)
        x = F.silu(x)
    else:
        x = x.add_(params)
        if step is not None:          # both projections are added before the norm (networks_edm.py:188)
            x = x.add_(step)
        x = F.silu(_gn(p, f'{key}.norm1', x, b.eps))
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


def unet(p, spec, x, c_noise, labels=None, step=None):
    """SongUNet / DhariwalUNet forward; `step` a one-element tensor of the network dtype, or None."""
    song = spec.model_type == 'SongUNet'
    emb = embedding_rows(p, spec, c_noise)
    if song:
        if spec.label_dim:
            emb = emb + _linear(p, 'model.map_label', labels * np.sqrt(spec.label_dim))
        emb = F.silu(_linear(p, 'model.map_layer0', emb))
        emb = F.silu(_linear(p, 'model.map_layer1', emb))
    else:
        emb = F.silu(_linear(p, 'model.map_layer0', emb))
        emb = _linear(p, 'model.map_layer1', emb)
        if spec.label_dim:
            emb = emb + _linear(p, 'model.map_label', labels)
        emb = F.silu(emb)
    emb_step = None
    if step is not None:
        emb_step = embedding_rows(p, spec, step, 'step')
        emb_step = F.silu(_linear(p, 'model.map_step_layer0', emb_step))
        emb_step = F.silu(_linear(p, 'model.map_step_layer1', emb_step))
    skips, aux = [], x
    for b in spec.enc:
        if b.kind == 'aux':
            x = skips[-1] = aux = (x + _conv(p, f'model.{b.name}', aux, spec.resample_filter, down=True, fused=True)) / np.sqrt(2)
        else:
            x = _conv(p, f'model.{b.name}', x, spec.resample_filter) if b.kind == 'conv' else _block(p, b, spec, x, emb, emb_step)
            skips.append(x)
    for b in spec.dec:
        if b.pops_skip:
            x = torch.cat([x, skips.pop()], dim=1)
        x = _block(p, b, spec, x, emb, emb_step)
    x = F.silu(_gn(p, f'model.{spec.out_norm}', x, spec.out_eps))
    return _conv(p, f'model.{spec.out_conv}', x, spec.resample_filter)


def edm_sfd(params, spec, x, sigma, labels=None, step=None, dtype=torch.float32):
    """EDMPrecond.forward (networks_edm.py:549-570): fp32 preconditioning coefficients around ``unet``; the step value becomes a one-element
    tensor of the network dtype (:553-554)."""
    with torch.no_grad():
        p = {k: v.to(dtype) for k, v in params.items()}
        x = x.to(torch.float32)
        sigma = torch.as_tensor(sigma).to(torch.float32).reshape(-1, 1, 1, 1)
        if spec.label_dim:
            labels = torch.zeros([1, spec.label_dim], device=x.device) if labels is None else labels.to(torch.float32).reshape(-1, spec.label_dim)
        if step is not None:
            step = torch.as_tensor(step).to(dtype).reshape(-1)
        sd = spec.sigma_data
        c_skip = sd ** 2 / (sigma ** 2 + sd ** 2)
        c_out = sigma * sd / (sigma ** 2 + sd ** 2).sqrt()
        c_in = 1 / (sd ** 2 + sigma ** 2).sqrt()
        c_noise = sigma.log() / 4
        f_x = unet(p, spec, (c_in * x).to(dtype), c_noise.flatten().to(dtype), None if labels is None else labels.to(dtype), step)
        return c_skip.to(dtype) * x.to(dtype) + c_out.to(dtype) * f_x


def euler(params, spec, latents, t_steps, step=None, afs=False, labels=None):
    """The reference's Euler loop (sfd-main/solvers.py:60-92) on ``edm_sfd``: [len(t_steps)] stacked states, the first one latents * t_0."""
    x = latents.to(torch.float32) * t_steps[0]
    out = [x]
    for i in range(len(t_steps) - 1):
        t, tn = t_steps[i], t_steps[i + 1]
        if afs and i == 0:
            d = x / ((1 + t ** 2).sqrt())
        else:
            d = (x - edm_sfd(params, spec, x, t, labels, step)) / t
        x = x + (tn - t) * d
        out.append(x)
    return torch.stack(out)


# ---- the latent-diffusion U-Net (sfd-main/models/ldm/modules/diffusionmodules/openaimodel.py:783-786, :298-316) ---------------------------------
def ldm_step_rows(params, spec, step, n=1):
    """{ResBlock key: emb_nfe_layers(nfe_embed(timestep_embedding(step)))} as [n, cout] rows per block -- n equal rows, as the reference
    computes them after expanding one step value to the batch (networks_edm.py:612-613; ATen sums a one-row product in another order)."""
    from oracle.ldm_net import timestep_embedding
    e = timestep_embedding(torch.full((n,), float(step), dtype=torch.float32), spec.model_channels)
    e = F.linear(F.silu(F.linear(e, params['nfe_embed.0.weight'], params['nfe_embed.0.bias'])), params['nfe_embed.2.weight'], params['nfe_embed.2.bias'])
    return {l.key: F.linear(F.silu(e), params[f'{l.key}.emb_nfe_layers.1.weight'], params[f'{l.key}.emb_nfe_layers.1.bias']) for l in spec.res_layers()}


class cfg_sfd:
    """oracle.ldm_net.OracleCFG (the project's restatement of CFGPrecond + UNetModel) with the step condition: its ResBlock is replaced, for the
    duration of a call, by one that adds the block's step row after the time-embedding row -- h + emb_out + emb_nfe_out in the reference's order
    (no scale-shift norm in this U-Net, openaimodel.py:314-316).  step None: the plain network.  A callable
    net(x, sigma, condition=, unconditional_condition=) with OracleCFG's attributes (sigma_min, sigma_max, sigma, sigma_inv, ...)."""

    def __init__(self, params, cfg, spec, guidance_rate=7.5, step=None):
        import diff_sampler_amd.ldm_arch as la
        from oracle.ldm_net import OracleCFG
        plain = {k: v for k, v in params.items() if not (k.startswith('nfe_embed.') or '.emb_nfe_layers.' in k)}
        self.net = OracleCFG(plain, cfg, la.alphas_cumprod(spec), guidance_rate=guidance_rate)
        self.params, self.spec, self.step, self.rows = params, spec, step, {}

    def __getattr__(self, name):
        return getattr(self.net, name)

    def __call__(self, *a, **k):
        import oracle.ldm_net as O
        if self.step is None:
            return self.net(*a, **k)
        conv, gn, lin = O._conv, O._gn32, O._lin

        def res(p, prefix, x, emb):
            n = x.shape[0]
            if n not in self.rows:
                with torch.no_grad():
                    self.rows[n] = ldm_step_rows(self.params, self.spec, self.step, n)
            h = conv(p, prefix + '.in_layers.2', F.silu(gn(p, prefix + '.in_layers.0', x, 1e-5)))
            h = h + lin(p, prefix + '.emb_layers.1', F.silu(emb))[:, :, None, None]
            h = h + self.rows[n][prefix][:, :, None, None]
            h = conv(p, prefix + '.out_layers.3', F.silu(gn(p, prefix + '.out_layers.0', h, 1e-5)))
            skip = conv(p, prefix + '.skip_connection', x) if (prefix + '.skip_connection.weight') in p else x
            return skip + h
        old, O._res = O._res, res
        try:
            return self.net(*a, **k)
        finally:
            O._res = old


# ---- DS_OP_AFFINE_COMPOSE: aff[r][scale] = fmaf(1 + s, 1 + ss, -1), aff[r][shift] = fmaf(h, 1 + ss, hs) -----------------------------------------
U = 2.0 ** -24          # unit roundoff of fp32 (round to nearest)


def compose_pairs(blocks):
    """int32 [groups][2] table for `blocks` = [(first column, cout)]: scale columns [off, off + cout), shift columns behind them."""
    return torch.tensor([(off + j, off + c + j) for off, c in blocks for j in range(0, c, 4)], dtype=torch.int32)


def _fma32(a, b, c):
    """fp32 fused multiply-add of fp32 tensors: the exact product and sum fit fp64's 53 bits only in part, but the fp64 value a*b + c is within
    2**-53 relative of exact and is then rounded once to fp32 -- a double rounding that can differ from fmaf in the last bit only."""
    return (a.double() * b.double() + c.double()).float()


def compose_emulate(aff, step, blocks):
    """The kernel's arithmetic in fp32 on a copy of `aff` [rows, ld]; columns outside `blocks` are left as they are."""
    out = aff.clone()
    one = torch.ones((), dtype=torch.float32)
    for off, c in blocks:
        g = one + step[off:off + c]
        out[:, off:off + c] = _fma32(one + aff[:, off:off + c], g, -one)
        out[:, off + c:off + 2 * c] = _fma32(aff[:, off + c:off + 2 * c], g, step[off + c:off + 2 * c])
    return out


def compose_ref64(aff, step, blocks):
    """(scale', shift') exact in fp64 and their per-element bounds for the kernel's fp32 result.
    Roundings, each at most U relative: a = fl(1 + s), g = fl(1 + ss), then ONE for the fused multiply-add.
        scale': fl(a g - 1) with a = (1+s)(1+e1), g = (1+ss)(1+e2):  |error| <= 2U |(1+s)(1+ss)| + U |scale'|  (+ second-order terms: x 1.01)
        shift': fl(h g + hs):                                        |error| <=  U |h (1+ss)|    + U |shift'|
    """
    a, st = aff.double(), step.double()
    ref, bound = a.clone(), torch.zeros_like(a)
    for off, c in blocks:
        s, h = a[:, off:off + c], a[:, off + c:off + 2 * c]
        ss, hs = st[off:off + c], st[off + c:off + 2 * c]
        prod = (1 + s) * (1 + ss)
        ref[:, off:off + c] = prod - 1
        ref[:, off + c:off + 2 * c] = h * (1 + ss) + hs
        bound[:, off:off + c] = 1.01 * U * (2 * prod.abs() + (prod - 1).abs())
        bound[:, off + c:off + 2 * c] = 1.01 * U * ((h * (1 + ss)).abs() + (h * (1 + ss) + hs).abs())
    return ref, bound


def two_stage64(n, aff, step, off, c):
    """The reference's two-stage expression in fp64 on normalised values n [rows, c]: shift_step + (shift + n (scale + 1)) (scale_step + 1),
    and the bound of the consumers' `fl(fl(fl(1 + scale') n) + shift')` in fp32 on the kernel's outputs.  With S = (1+s)(1+ss), H = h(1+ss) + hs:
        scale' = (S (1+e1)(1+e2) - 1)(1+e3), so 1 + scale' = S (1+e1)(1+e2)(1+e3) - e3 and q = fl(1 + scale') differs from S by <= 4U |S| + U;
        fl(q n) adds U |S n|:                     (5 |S| + 1) U |n|
        shift' = (h (1+ss)(1+e2) + hs)(1+e5):      U |h (1+ss)| + U |H|
        the last addition:                         U |result|
    to first order; x 1.01 for the second-order terms.  (A consumer that fuses the multiply-add rounds once less.)"""
    a, st = aff.double(), step.double()
    s, h = a[:, off:off + c], a[:, off + c:off + 2 * c]
    ss, hs = st[off:off + c], st[off + c:off + 2 * c]
    n = n.double()
    ref = hs + (h + n * (s + 1)) * (ss + 1)
    S, H1 = ((1 + s) * (1 + ss)).abs(), (h * (1 + ss)).abs()
    bound = 1.01 * U * ((5 * S + 1) * n.abs() + H1 + (h * (1 + ss) + hs).abs() + ref.abs())
    return ref, bound
