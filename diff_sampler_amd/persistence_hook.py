"""Zero-edit route into the reference: its own sanctioned extension point ``torch_utils.persistence.import_hook``.

Reference: ``torch_utils/persistence.py:153-181`` (``import_hook(hook)``: every registered ``hook(meta) -> meta`` sees each
persistent object while it is unpickled and may rewrite ``meta.module_src``, the pickled module source that is then
``exec``'d, ``persistence.py:222-233``) and ``sample.py:83-87`` (``create_model`` unpickles ``['ema']`` -- an ``EDMPrecond`` --
and moves it to the device).  SURVEY section 8(b) names this hook as the way an accelerated package substitutes the denoiser
without editing ``sample.py``.

    import torch_utils.persistence                     # the reference's module (diff-solvers-main / gits-main / amed-solver-main)
    import diff_sampler_amd.persistence_hook as hook
    hook.install()                                     # before the first pickle.load of an EDM snapshot

After ``install()`` every ``EDMPrecond`` that is unpickled keeps its class, attributes, ``state_dict`` and module tree
(``net.sigma_min``, ``net.label_dim``, ``net.model.enc[...]`` stay exactly what ``sample.py`` and the AMED code read), but a
call ``net(x, sigma, class_labels)`` with ``x`` on the GPU is evaluated by ``engine.EDMDenoiser`` (the HIP plan, built lazily from
the module's own weights on the first call and cached on the instance).  Nothing else changes: the samplers that call it are
still the reference's ``solvers.py``; for the fused update kernels and the one-launch DPM-Solver++ step import
``diff_sampler_amd.solvers`` instead of ``solvers``.

An SFD-distilled snapshot (a module with ``map_step_layer0``) is routed with its ``step_condition`` keyword too.

What the route does NOT do, on purpose: it computes nothing itself, and it is INFERENCE-ONLY.  Calls with CPU tensors, with
``augment_labels`` / other ``model_kwargs`` (``skip_tuning=True`` among them), or that autograd would record (grad mode on and an input or a parameter of the module
requires grad: amed-solver-main's training path, ``solvers_amed.py:141-143`` with ``train=True``) go to the module's ORIGINAL
``forward`` -- the reference's own code, not a fallback of this package -- so gradients are never silently dropped; a GPU call
whose HIP library is missing (``_lib.DsError``) or whose module ``engine.spec_from_module`` does not recognise raises, like every
other entry point.  The inner modules are not executed under the route; the one place the reference observes them -- the AMED
bottleneck tap, a forward hook on ``net.model.enc['8x8_block2' | '8x8_block3']`` (``solvers_amed.py:7-18``) -- is honoured: hooks
registered on those two blocks are called with the engine's output of the same block, so amed-solver-main's own ``solvers_amed.py``
runs on a routed net (``diff_sampler_amd.solvers_amed`` does the same without hooks, taking the bottleneck from the plan).  Weights are
packed when the engine is built; call ``invalidate(net)`` after changing them.
"""
from __future__ import annotations

import torch

MARK = '# --- appended by diff_sampler_amd.persistence_hook ---'
ROUTED_CLASSES = ('EDMPrecond',)

_PATCH = '''

%s
def _ds_amd_route():
    try:
        import diff_sampler_amd.persistence_hook as _h
    except ImportError:          # a snapshot re-saved under the route, loaded where the package is absent: plain reference
        return
    for _name in _h.ROUTED_CLASSES:
        if _name in globals():
            _h.route_class(globals()[_name])
_ds_amd_route()
del _ds_amd_route
''' % MARK

_ENGINES = '_ds_amd_engines'


def hook(meta):
    """``persistence.import_hook`` callback: append the routing stub to every pickled module source that defines a routed class
    (the same patched source for the outer ``EDMPrecond`` and its inner ``SongUNet`` / ``DhariwalUNet`` objects, so that
    ``_src_to_module`` still creates ONE module for them, persistence.py:222-233)."""
    src = getattr(meta, 'module_src', None)
    if getattr(meta, 'type', None) == 'class' and isinstance(src, str) and MARK not in src \
            and any(f'class {name}' in src for name in ROUTED_CLASSES):
        meta.module_src = src + _PATCH
    return meta


def install(persistence=None):
    """Register ``hook`` with the reference's ``torch_utils.persistence`` (imported from ``sys.path`` unless given).  Idempotent.
    Returns the persistence module."""
    if persistence is None:
        import importlib
        persistence = importlib.import_module('torch_utils.persistence')
    hooks = getattr(persistence, '_import_hooks')
    if hook not in hooks:
        persistence.import_hook(hook)
    return persistence


def uninstall(persistence=None):
    if persistence is None:
        import importlib
        persistence = importlib.import_module('torch_utils.persistence')
    hooks = getattr(persistence, '_import_hooks')
    while hook in hooks:
        hooks.remove(hook)


def make_engine(net, device, use_fp16):
    """The engine of one (module, device, precision): separate function so that tests can substitute it."""
    from .engine import EDMDenoiser
    return EDMDenoiser.from_reference_module(net, device=device, use_fp16=use_fp16)


def invalidate(net):
    """Drop the cached engines of ``net`` (after ``load_state_dict`` / weight edits); the next GPU call rebuilds them."""
    net.__dict__.pop(_ENGINES, None)


AMED_TAPS = ('8x8_block2', '8x8_block3')          # solvers_amed.py:15-17: class-conditional / unconditional EDM nets


def _fire_bottleneck_hooks(net, eng):
    """The AMED code taps the U-Net bottleneck with a forward hook on ``net.model.enc['8x8_block2' | '8x8_block3']``
    (amed-solver-main/solvers_amed.py:7-18).  Under the route that block's module does not execute, so its registered forward hooks are
    called here with the engine's output of the same block (``EDMDenoiser.block_output``): the reference's ``solvers_amed.py`` then runs
    unchanged on a routed net."""
    enc = getattr(getattr(net, 'model', None), 'enc', None)
    if enc is None:
        return
    for key in AMED_TAPS:
        mod = enc[key] if key in enc else None
        hooks = getattr(mod, '_forward_hooks', None) if mod is not None else None
        if hooks:
            out = eng.block_output('enc.' + key)
            for fn in list(hooks.values()):
                fn(mod, (), out)


def _needs_autograd(net, *inputs):
    """The route is INFERENCE-ONLY: the engine's output has no grad_fn.  A call that autograd would record -- grad mode on and an
    input that requires grad (amed-solver-main/solvers_amed.py:141-143 with train=True differentiates through
    net(x_mid(r), scale_time * t_mid(r)); training_loop.py:205 backward) or a trainable parameter of the module itself -- goes to the
    reference forward, so gradients are never silently dropped."""
    if not torch.is_grad_enabled():
        return False
    if any(isinstance(t, torch.Tensor) and t.requires_grad for t in inputs):
        return True
    return any(p.requires_grad for p in net.parameters())


def route_class(cls):
    """Wrap ``cls.forward`` (``EDMPrecond.forward``, networks_edm.py:482-496) so that GPU calls run on the HIP engine.  Same
    signature, same return (denoised NCHW fp32).  Idempotent per class object."""
    if cls.__dict__.get('_ds_amd_routed', False):
        return cls
    reference_forward = cls.forward

    def forward(self, x, sigma, class_labels=None, force_fp32=False, **model_kwargs):
        # an SFD-distilled net (it has map_step_layer0) takes `step_condition` -- and the `skip_tuning=False` sfd-main's sampler always
        # passes -- on the engine; every other keyword, and these two on a module without step layers, stay the reference's business
        step_kw = {}
        if getattr(getattr(self, 'model', None), 'map_step_layer0', None) is not None and not model_kwargs.get('skip_tuning', False):
            rest = {k: v for k, v in model_kwargs.items() if k not in ('step_condition', 'skip_tuning')}
            if not rest:
                step_kw, model_kwargs = dict(step_condition=model_kwargs.get('step_condition')), {}
        if not getattr(x, 'is_cuda', False) or model_kwargs or _needs_autograd(self, x, sigma, class_labels):
            return reference_forward(self, x, sigma, class_labels, force_fp32=force_fp32, **model_kwargs, **step_kw)
        # networks_edm.py:486: fp16 body only when the module asks for it and the caller does not force fp32
        use_fp16 = bool(getattr(self, 'use_fp16', False)) and not force_fp32
        engines = self.__dict__.setdefault(_ENGINES, {})
        key = (str(x.device), use_fp16)
        eng = engines.get(key)
        if eng is None:
            eng = engines[key] = make_engine(self, x.device, use_fp16)
        out = eng(x, sigma, class_labels=class_labels, **step_kw)
        _fire_bottleneck_hooks(self, eng)
        return out

    forward.__doc__ = reference_forward.__doc__
    forward.reference_forward = reference_forward
    cls.forward = forward
    cls._ds_amd_routed = True
    return cls
