"""The duck-typed stand-ins of tests/_ref_like.py / tests/_ref_like_ncsnpp.py with what SFD's step-conditioned nets add to the module tree (test
infrastructure; no reference code).

An unpickled SFD ``EDMPrecond`` (sfd-main/models/networks_edm.py) differs from an EDM one in three places, which is what
``engine.spec_from_module`` reads the ``step_condition`` flag from:

  * ``model.map_step``: an embedding module right after the noise path's layers -- with a ``freqs`` buffer of its own for NCSN++ (:290 / :438);
  * ``model.map_step_layer0 / map_step_layer1``: two Linear layers shaped like ``map_layer0 / map_layer1`` (:291-292 / :439-440);
  * ``affine_step`` in every U-Net block, shaped like its ``affine`` and registered after ``conv1`` (:153).

``build(..., drop='map' | 'affine')`` leaves one of the two groups out: a tree the engine must refuse.
"""
from collections import OrderedDict

import torch

import _ref_like
import _ref_like_ncsnpp
from _ref_like import _Block, _Leaf


def _insert_after(module, after, name, child):
    """Register `child` as `name` right behind the child `after` (state_dict order is registration order)."""
    items = list(module._modules.items())
    at = [k for k, _ in items].index(after) + 1
    module._modules = OrderedDict(items[:at] + [(name, child)] + items[at:])


def add_step_layers(net, spec, drop=None):
    model = net.model
    E, NC = spec.emb_channels, spec.noise_channels
    last = 'map_label' if (spec.model_type != 'SongUNet' and 'map_label' in model._modules) else 'map_layer1'
    if drop != 'map':
        _insert_after(model, last, 'map_step', _ref_like_ncsnpp._Embedding(NC, spec.embedding_type == 'fourier'))
        _insert_after(model, 'map_step', 'map_step_layer0', _Leaf((E, NC)))
        _insert_after(model, 'map_step_layer0', 'map_step_layer1', _Leaf((E, E)))
    if drop != 'affine':
        for part in (model.enc, model.dec):
            for blk in part.values():
                if isinstance(blk, _Block):
                    _insert_after(blk, 'conv1', 'affine_step', _Leaf(tuple(blk.affine.weight.shape)))
    return net


def build(name_or_kwargs, seed=0, mode='signal', use_fp16=None, drop=None, training_kwargs=None):
    """A filled duck of the config with step-condition layers: weights = ``arch.init_params(spec with step_condition, seed, mode)``."""
    import diff_sampler_amd.arch as arch
    kw = dict(arch.NAMED_CONFIGS[name_or_kwargs] if isinstance(name_or_kwargs, str) else name_or_kwargs)
    kw.pop('step_condition', None)
    if use_fp16 is not None:
        kw['use_fp16'] = use_fp16
    spec = arch.edm_precond_spec(**kw, step_condition=True)
    cls = _ref_like_ncsnpp.EDMPrecond if spec.ncsnpp else _ref_like.EDMPrecond
    net = add_step_layers(cls(**kw), spec, drop).eval().requires_grad_(False)
    missing, unexpected = net.load_state_dict(arch.init_params(spec, seed=seed, mode=mode), strict=False)
    assert all('resample_filter' in m for m in missing), missing
    assert drop is not None or not unexpected, unexpected
    if training_kwargs is not None:
        net.training_kwargs = dict(training_kwargs)
    return net


# ---- the latent-diffusion snapshot: CFGPrecond -> LatentDiffusion -> DiffusionWrapper -> UNetModel ---------------------------------------------
class _Tree(torch.nn.Module):
    """A module tree that holds `params` under their dotted state-dict keys (containers named by the key's components, no arithmetic)."""

    def __init__(self, params=None):
        super().__init__()
        for key, value in (params or {}).items():
            node, parts = self, key.split('.')
            for part in parts[:-1]:
                if part not in node._modules:
                    node.add_module(part, _Tree())
                node = node._modules[part]
            node.register_parameter(parts[-1], torch.nn.Parameter(value.clone(), requires_grad=False))

    def forward(self, *a, **k):
        raise NotImplementedError('duck-typed module: this call was not routed to the HIP engine')


class CFGPrecond(torch.nn.Module):
    """What ``pickle.load(f)['model']`` of an SFD ms_coco snapshot exposes to ``sample.load_sfd``: ``img_resolution`` / ``img_channels``
    (sfd-main/models/networks_edm.py:589-590), ``training_kwargs``, and ``.model`` -- the LatentDiffusion -- whose state dict is keyed
    ``model.diffusion_model.*`` (ddpm.py:1399) and whose U-Net keeps its constructor arguments as attributes (openaimodel.py:540-553)."""

    def __init__(self, cfg, params, training_kwargs):
        super().__init__()
        self.img_resolution, self.img_channels, self.label_dim = cfg['img_resolution'], cfg['in_channels'], True
        self.guidance_type, self.guidance_rate = 'classifier-free', training_kwargs.get('guidance_rate')
        self.training_kwargs = dict(training_kwargs)
        unet = _Tree(params)
        unet.image_size, unet.in_channels, unet.out_channels = 32, cfg['in_channels'], cfg['out_channels']
        unet.model_channels, unet.num_res_blocks, unet.num_heads = cfg['model_channels'], cfg['num_res_blocks'], cfg['num_heads']
        unet.attention_resolutions, unet.channel_mult = list(cfg['attention_resolutions']), list(cfg['channel_mult'])
        self.model = _Tree()
        self.model.add_module('model', _Tree())
        self.model.model.add_module('diffusion_model', unet)

    def forward(self, *a, **k):
        raise NotImplementedError('duck-typed CFGPrecond: this call was not routed to the HIP engine')


def build_ldm(name, seed=0, training_kwargs=None, drop=None):
    """A filled duck of the named latent-diffusion config with step-condition layers: weights = ``ldm_arch.init_ldm_params(spec, seed)``.
    drop='nfe_embed' | 'emb_nfe_layers' leaves one group of step layers out: a tree the engine must refuse."""
    import diff_sampler_amd.ldm_arch as la
    cfg = dict(la.NAMED_LDM_CONFIGS[name])
    params = la.init_ldm_params(la.ldm_unet_spec(**cfg, step_condition=True), seed=seed)
    if drop:
        params = {k: v for k, v in params.items() if drop not in k}
    return CFGPrecond(cfg, params, training_kwargs or {}).eval()
