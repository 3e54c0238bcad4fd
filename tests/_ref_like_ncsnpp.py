"""The duck-typed stand-in of tests/_ref_like.py for a SongUNet with the NCSN++ options (test infrastructure; no reference code).

What the options leave in an unpickled module tree, and what ``engine.spec_from_module`` reads them from:

  * ``model.map_noise``: a module with a ``freqs`` buffer [noise_channels / 2] for ``embedding_type='fourier'`` (networks_edm.py:207), one
    without any state for ``'positional'``;
  * ``model.enc['<res>x<res>_aux_residual']`` right after ``'<res>x<res>_down'``: a 3x3 convolution ``caux -> cout`` with ``down`` and
    ``fused_resample`` set and a ``resample_filter`` buffer (networks_edm.py:283);
  * the ``resample_filter`` buffers of every up / down convolution: [1, 1, k, k] = f (x) f / (sum f)^2, k = 2 for [1,1] and 4 for [1,3,3,1].

``build(..., skip_variant=True)`` adds the ``aux_down`` / ``aux_skip`` layers of ``encoder_type='skip'`` (networks_edm.py:279-281): a tree the
engine must refuse.
"""
import torch

from _ref_like import _Block, _Leaf, _Norm


def _filter(taps):
    f = torch.as_tensor(list(taps), dtype=torch.float32)
    return (f.ger(f) / f.sum().square())[None, None]


class _Embedding(torch.nn.Module):
    def __init__(self, channels, fourier):
        super().__init__()
        if fourier:
            self.register_buffer('freqs', torch.zeros(channels // 2))


class _UNet(torch.nn.Module):
    def __init__(self, spec, skip_variant=False):
        super().__init__()
        assert spec.model_type == 'SongUNet'
        E, NC, filt = spec.emb_channels, spec.noise_channels, _filter(spec.resample_filter)
        self.map_noise = _Embedding(NC, spec.embedding_type == 'fourier')
        self.map_label = _Leaf((NC, spec.label_dim)) if spec.label_dim else None
        self.map_augment = _Leaf((NC, spec.augment_dim), bias=False) if spec.augment_dim else None
        self.map_layer0 = _Leaf((E, NC))
        self.map_layer1 = _Leaf((E, E))
        self.enc, self.dec = torch.nn.ModuleDict(), torch.nn.ModuleDict()
        for b in spec.blocks:
            side, key = b.name.split('.', 1)
            if b.kind == 'conv':
                mod = _Leaf((b.cout, b.cin, 3, 3), in_channels=b.cin, out_channels=b.cout)
            elif b.kind == 'aux':
                mod = _Leaf((b.cout, b.cin, 3, 3), resample=True, in_channels=b.cin, out_channels=b.cout, up=False, down=True, fused_resample=True)
                mod.resample_filter = filt.clone()
            else:
                mod = _Block(b, E, True)
                if b.up or b.down:
                    mod.conv0.resample_filter, mod.skip.resample_filter = filt.clone(), filt.clone()
            (self.enc if side == 'enc' else self.dec)[key] = mod
            if skip_variant and b.kind == 'block' and b.down:
                r = f'{b.res_out}x{b.res_out}'
                self.enc[f'{r}_aux_down'] = _Leaf(None, resample=True, in_channels=spec.in_channels, out_channels=spec.in_channels, down=True)
                self.enc[f'{r}_aux_skip'] = _Leaf((b.cout, spec.in_channels, 1, 1), in_channels=spec.in_channels, out_channels=b.cout)
        last = spec.blocks[-1].cout
        self.dec[spec.out_norm.split('.', 1)[1]] = _Norm(last)
        self.dec[spec.out_conv.split('.', 1)[1]] = _Leaf((spec.out_channels, last, 3, 3), in_channels=last, out_channels=spec.out_channels)


class EDMPrecond(torch.nn.Module):
    """Attributes and module tree of the reference object of the same name around an NCSN++-capable SongUNet; ``forward`` has no arithmetic."""

    def __init__(self, img_resolution, img_channels, label_dim=0, use_fp16=False, sigma_min=0.002, sigma_max=80.0, sigma_data=0.5,
                 model_type='SongUNet', skip_variant=False, **model_kwargs):
        super().__init__()
        import diff_sampler_amd.arch as arch
        self.img_resolution, self.img_channels, self.label_dim, self.use_fp16 = img_resolution, img_channels, label_dim, use_fp16
        self.sigma_min, self.sigma_max, self.sigma_data = sigma_min, sigma_max, sigma_data
        self.model = _UNet(arch.edm_precond_spec(img_resolution, img_channels, label_dim=label_dim, model_type=model_type, **model_kwargs),
                           skip_variant)

    def forward(self, x, sigma, class_labels=None, force_fp32=False, **model_kwargs):
        raise NotImplementedError('duck-typed EDMPrecond: this call was not routed to the HIP engine')

    def round_sigma(self, sigma):
        return torch.as_tensor(sigma)


def build(name_or_kwargs, seed=0, mode='signal', skip_variant=False):
    """A filled duck: weights = ``arch.init_params(spec, seed, mode)`` loaded by state_dict key (``map_noise.freqs`` included)."""
    import diff_sampler_amd.arch as arch
    kw = dict(arch.NAMED_CONFIGS[name_or_kwargs] if isinstance(name_or_kwargs, str) else name_or_kwargs)
    net = EDMPrecond(skip_variant=skip_variant, **kw).eval().requires_grad_(False)
    missing, unexpected = net.load_state_dict(arch.init_params(arch.edm_precond_spec(**kw), seed=seed, mode=mode), strict=False)
    assert not unexpected and all('resample_filter' in m or 'aux_skip' in m for m in missing), (missing, unexpected)
    return net
