"""``CMDenoiser``: the drop-in for the reference's ``CMPrecond`` (networks_edm.py:504-552) around a consistency-model ``UNetModel``
(models/cm/unet.py), backed by the same ``UNetEngine`` plans as the EDM nets.

``c_skip`` / ``c_out`` / ``c_in`` of CMPrecond are EDM's with ``sigma_data = 0.5``, so ``raw()`` and the head-fused solver update apply
unchanged; only the embedding argument differs (``arch.UNetSpec.cm_noise``).  What is new here is the loading (``cm_arch``) and the batch
ceiling of a 256-pixel plan.

Batch ceiling.  A plan's workspaces hold B images of the largest layer: at 256 pixels the concatenated level-0 tensor (512 channels) is
2**25 elements per image, 2**31 at 64 images -- ``sample.py``'s default ``--batch``.  Every kernel a plan launches addresses rows and pixels
with 32-bit integers and widens to 64 bits where a row index meets a row pitch (the ``(size_t)row * ld`` form of csrc/), and
``ds_conv2d_nhwc`` refuses n * h * w beyond 2**31 - 128; but rather than rest on every such product of every kernel, one plan takes only
what keeps EVERY tensor it touches below 2**31 BYTES, so that neither an element index nor a byte offset of any kernel can leave 31 bits:
``max_plan_batch = (2**31 - 1) // (4 * elements per image of the largest workspace)`` -- 15 images for the LSUN nets, thousands for a
64-pixel net.  A larger call is evaluated in sub-batches of at most that size, in order; with ``batch_invariant`` the result does not depend
on where the cuts fall.
"""
from __future__ import annotations


import torch

from . import arch, cm_arch
from .engine import EDMDenoiser


def plan_elements_per_image(spec: arch.UNetSpec) -> int:
    """Elements per image of the largest tensor a UNetEngine plan allocates (UNetEngine._workspaces: activations, and the packed q | k | v rows)."""
    n = spec.img_resolution ** 2 * (-(-9 * spec.in_channels // 32) * 32)
    for b in spec.blocks:
        hw = b.res_out ** 2
        n = max(n, b.cin * hw, b.cout * hw, 3 * b.cout * hw if b.heads else 0)
    return n


def split_batch(total: int, ceiling: int):
    """[(begin, end)] of the sub-batches a call of `total` images is evaluated in: as many full ones as fit, then the rest."""
    if ceiling < 1:
        raise ValueError('the batch ceiling must be at least 1')
    return [(i, min(i + ceiling, total)) for i in range(0, total, ceiling)]


class CMDenoiser(EDMDenoiser):
    """``net(x, sigma)`` -> denoised NCHW fp32, like ``CMPrecond``; duck-types its attributes (``img_resolution``, ``img_channels``,
    ``label_dim`` = 0, ``sigma_min`` / ``sigma_max`` / ``sigma_data``, ``round_sigma``)."""

    def __init__(self, spec, params, device='cuda', use_fp16=False, batch_invariant=False, wide16=True, **kw):
        if not spec.cm_noise or spec.label_dim:
            raise ValueError('CMDenoiser takes a spec of cm_arch.cm_unet_spec')
        super().__init__(spec, params, device, use_fp16=use_fp16, batch_invariant=batch_invariant, wide16=wide16, **kw)
        self._build = dict(params=params, device=device, batch_invariant=batch_invariant)
        self._fp32 = None
        self.max_plan_batch = max(1, (2 ** 31 - 1) // (4 * plan_elements_per_image(spec)))
        self.bottleneck_name = cm_arch.middle_block_name(spec)
        self._chunk_bott = self._chunk_tap = None

    # ---- constructors ---------------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_config(cls, name_or_kwargs, seed=0, mode='signal', device='cuda', use_fp16=False, batch_invariant=False, wide16=True):
        """Random-init net of a named config (cm_arch.NAMED_CM_CONFIGS) or of ``create_model`` keywords; fp32 unless asked, like the other nets."""
        spec = cm_arch.cm_precond_spec(name_or_kwargs)
        return cls(spec, arch.init_params(spec, seed=seed, mode=mode), device, use_fp16=use_fp16, batch_invariant=batch_invariant, wide16=wide16)

    @classmethod
    def from_state_dict(cls, path_or_dict, setting, device='cuda', use_fp16=None, batch_invariant=False, wide16=True):
        """A ``UNetModel`` checkpoint (path or state dict) of ``setting`` (a config name or ``create_model`` keywords).  ``use_fp16`` None
        follows the setting (``lsun_setting()``: True -- ``load_cm_model`` converts the body to fp16)."""
        spec = cm_arch.cm_precond_spec(setting)
        sd = torch.load(path_or_dict, map_location='cpu') if isinstance(path_or_dict, (str, bytes)) or hasattr(path_or_dict, '__fspath__') else path_or_dict
        if use_fp16 is None:
            use_fp16 = spec.use_fp16
        return cls(spec, cm_arch.engine_params(spec, sd), device, use_fp16=bool(use_fp16), batch_invariant=batch_invariant, wide16=wide16)

    @classmethod
    def from_reference_module(cls, net, device='cuda', use_fp16=None, batch_invariant=False, wide16=True):
        """From a live ``CMPrecond``: the setting is recovered from the ``UNetModel``'s own attributes."""
        spec = spec_from_cm_module(net)
        if use_fp16 is None:
            use_fp16 = bool(getattr(net, 'use_fp16', False))
        sd = {k: v.detach().float() for k, v in net.model.state_dict().items()}
        return cls(spec, cm_arch.engine_params(spec, sd), device, use_fp16=bool(use_fp16), batch_invariant=batch_invariant, wide16=wide16)

    def round_sigma(self, sigma):
        return torch.as_tensor(sigma)

    # ---- evaluation in sub-batches ------------------------------------------------------------------------------------------------------
    def _chunks(self, B):
        return split_batch(B, int(self.max_plan_batch))

    @staticmethod
    def _part(sigma, i, j):
        if isinstance(sigma, (int, float)):
            return sigma
        s = torch.as_tensor(sigma).reshape(-1)
        return s if s.numel() == 1 else s[i:j]

    def head_update_ok(self, B, sigma, class_labels=None, step_condition=None):
        if B > self.max_plan_batch:          # the update then runs as a launch of its own over the whole batch
            return False
        return super().head_update_ok(B, sigma, class_labels, step_condition)

    def raw(self, x, sigma, class_labels=None, update=None, step_condition=None):
        B = x.shape[0]
        if B <= self.max_plan_batch:
            self._chunk_bott = None
            return super().raw(x, sigma, class_labels, update=update, step_condition=step_condition)
        if update is not None:
            raise ValueError('a call beyond max_plan_batch cannot carry a head-fused update (head_update_ok says so)')
        out = torch.empty(B, *x.shape[1:], dtype=torch.float32, device=self.device)
        botts, plan = [], None
        for i, j in self._chunks(B):
            f, plan = super().raw(x[i:j].contiguous(), self._part(sigma, i, j), None, step_condition=step_condition)
            out[i:j].copy_(f)
            botts.append(self._tap_mean(plan, j - i))
        self._chunk_bott = (plan, torch.cat(botts, 0))
        return out, plan

    def __call__(self, x, sigma, class_labels=None, force_fp32=False, **kwargs):
        """force_fp32: evaluated by an fp32 engine on the same weights, built on first use (CMPrecond.forward: the body's dtype)."""
        if force_fp32 and self.use_fp16:
            if self._fp32 is None:
                self._fp32 = CMDenoiser(self.spec, self._build['params'], self._build['device'], use_fp16=False,
                                        batch_invariant=self._build['batch_invariant'])
                self._fp32.max_plan_batch = self.max_plan_batch
            return self._fp32(x, sigma, class_labels, **kwargs)
        B = x.shape[0]
        if B <= self.max_plan_batch:
            self._chunk_bott = None
            return super().__call__(x, sigma, class_labels, **kwargs)
        outs, botts, taps = [], [], []
        for i, j in self._chunks(B):
            outs.append(super().__call__(x[i:j], self._part(sigma, i, j), None, **kwargs))
            botts.append(self._tap_mean(self._last[0], j - i))
            taps.append(super().block_output(self.bottleneck_name))
        self._chunk_bott = (self._last[0], torch.cat(botts, 0))
        self._chunk_tap = torch.cat(taps, 0)
        return torch.cat(outs, 0)

    # ---- the AMED tap: the output of middle_block ----------------------------------------------------------------------------------------
    def block_output(self, name):
        if self._chunk_bott is not None:
            if name != self.bottleneck_name:
                raise KeyError(f'a call in sub-batches keeps the AMED tap {self.bottleneck_name!r} only')
            return self._chunk_tap
        return super().block_output(name)

    def tap_shape(self):
        """(channels, side) of the AMED tap."""
        b = [b for b in self.spec.blocks if b.name == self.bottleneck_name][0]
        return b.cout, b.res_out

    def bottleneck_mean(self, plan, B, class_cond=False):
        """Channel mean of ``middle_block``'s output, [B, h, h] (h = 8 for the 256-pixel nets: the 64 values the AMED predictor reads)."""
        if self._chunk_bott is not None and plan is self._chunk_bott[0]:
            return self._chunk_bott[1]
        return self._tap_mean(plan, B)

    def _tap_mean(self, plan, B):
        from . import ops
        t = plan.bufs[self.bottleneck_name].float()
        c = t.shape[1]
        h = int(round((t.shape[0] // B) ** 0.5))
        out = torch.empty(B, h, h, dtype=torch.float32, device=self.device)
        ops.channel_mean(t, c, c, B * h * h, out)
        return out


def spec_from_cm_module(net) -> arch.UNetSpec:
    """The spec of a live ``CMPrecond``: ``create_model`` keywords read back from its ``UNetModel``."""
    m = net.model
    R = int(m.image_size)
    res_blocks = [b for b in m.input_blocks if type(b[0]).__name__ == 'ResBlock']
    updown = any(getattr(b[0], 'updown', False) for b in res_blocks)
    attn = [mod for mod in m.modules() if type(mod).__name__ == 'AttentionBlock']
    head_ch = {a.qkv.weight.shape[1] // a.num_heads for a in attn}
    flash = all(type(a.attention).__name__ == 'QKVFlashAttention' for a in attn)
    if len(head_ch) != 1 or not flash:
        raise NotImplementedError('CM UNetModel whose attention blocks are not QKVFlashAttention with one head width is not supported')
    ds_attn = sorted(R // r for r in m.attention_resolutions)
    kw = dict(image_size=R, num_channels=int(m.model_channels), num_res_blocks=int(m.num_res_blocks),
              channel_mult=','.join(str(int(c)) if int(c) == c else str(c) for c in m.channel_mult),
              class_cond=m.num_classes is not None, attention_resolutions=','.join(str(r) for r in ds_attn),
              num_head_channels=head_ch.pop(), use_scale_shift_norm=bool(res_blocks[0][0].use_scale_shift_norm), resblock_updown=updown,
              use_fp16=bool(getattr(net, 'use_fp16', False)), learn_sigma=int(m.out_channels) != int(m.in_channels),
              sigma_min=float(net.sigma_min), sigma_max=float(net.sigma_max), sigma_data=float(net.sigma_data))
    return cm_arch.cm_unet_spec(**kw)
