"""The reference ``EDMPrecond`` as recorded by ``oracle/gen_ref_structure.py`` (``tests/golden/ref_structure.json.gz``; test infrastructure).

``recorded(name, use_fp16)`` rebuilds, from the fixture alone, an object that exposes what the adapters read from a live reference module:
the attributes, ``.model.enc`` / ``.model.dec`` ``ModuleDict``s whose blocks carry the recorded ``in_channels / out_channels / num_heads``,
and the embedding layers' ``weight`` (meta tensors of the recorded shapes).  ``state_dict_entries(...)`` is the recorded
``[(key, shape, dtype)]`` list in the reference's order.
"""
import gzip
import json
import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_structure.json.gz')
_CACHE = {}


def load():
    if 'z' not in _CACHE:
        with gzip.open(GOLDEN, 'rt') as fh:
            _CACHE['z'] = json.load(fh)
    return _CACHE['z']


def case(name, use_fp16=False):
    return load()['cases'][f'{name}/use_fp16={int(bool(use_fp16))}']


def state_dict_entries(name, use_fp16=False):
    return [(k, tuple(s), getattr(torch, d)) for k, s, d in case(name, use_fp16)['state_dict']]


class _Rec(torch.nn.Module):
    def __init__(self, attrs=None, weight=None):
        super().__init__()
        for k, v in (attrs or {}).items():
            setattr(self, k, v)
        if weight is not None:
            self.weight = torch.nn.Parameter(torch.empty(weight, device='meta'), requires_grad=False)


def recorded(name, use_fp16=False):
    c = case(name, use_fp16)
    net = _Rec(c['attrs'])
    net.model = _Rec()
    net.model.enc = torch.nn.ModuleDict([(k, _Rec(a)) for k, a in c['enc']])
    net.model.dec = torch.nn.ModuleDict([(k, _Rec(a)) for k, a in c['dec']])
    for leaf, shape in c['leaves'].items():
        setattr(net.model, leaf, _Rec(weight=shape) if shape is not None else None)
    return net
