"""ORACLE tooling: record what the adapters read from a REAL reference ``EDMPrecond`` as a data fixture
(``tests/golden/ref_structure.json.gz``), so that the tests of ``engine.spec_from_module`` and of ``tests/_ref_like.py`` run where the
reference is absent.  Run where the reference tree is present:

    python oracle/gen_ref_structure.py --ref DIR        # DIR: root of the reference tree (or DS_REFERENCE_DIR)

Per named configuration (``arch.NAMED_CONFIGS``) and ``use_fp16`` setting, built on the meta device (no weights): the attributes
``sample.py`` reads, every ``state_dict`` entry (key, shape, dtype, in order), the ``enc`` / ``dec`` block keys with the
``in_channels / out_channels / num_heads`` each block carries, and the weight shapes of the embedding layers.  Also the names of the
functions defined in the reference ``solver_utils.py``.  Only names, shapes and numbers are stored: no reference code.
"""
import argparse
import ast
import gzip
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'ref_structure.json.gz')
sys.path.insert(0, ROOT)

NAMES = ('cifar10', 'ffhq', 'imagenet64', 'tiny_song', 'tiny_song_cond', 'tiny_adm', 'tiny_song_amed')
ATTRS = ('img_resolution', 'img_channels', 'label_dim', 'use_fp16', 'sigma_min', 'sigma_max', 'sigma_data')
BLOCK_ATTRS = ('in_channels', 'out_channels', 'num_heads')
LEAVES = ('map_layer0', 'map_layer1', 'map_label', 'map_augment')


def record(net):
    m = net.model
    return dict(
        attrs={a: getattr(net, a) for a in ATTRS},
        state_dict=[[k, list(v.shape), str(v.dtype).replace('torch.', '')] for k, v in net.state_dict().items()],
        enc=[[k, {a: getattr(b, a) for a in BLOCK_ATTRS if hasattr(b, a)}] for k, b in m.enc.items()],
        dec=[[k, {a: getattr(b, a) for a in BLOCK_ATTRS if hasattr(b, a)}] for k, b in m.dec.items()],
        leaves={l: (list(getattr(m, l).weight.shape) if getattr(m, l, None) is not None else None) for l in LEAVES})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', default=os.environ.get('DS_REFERENCE_DIR'), help='root of the reference tree (holds diff-solvers-main/)')
    args = ap.parse_args()
    if not args.ref:
        ap.error('--ref (or DS_REFERENCE_DIR) must name the reference tree')
    solvers_dir = os.path.join(args.ref, 'diff-solvers-main')
    sys.path.insert(0, solvers_dir)
    from models.networks_edm import EDMPrecond
    import diff_sampler_amd.arch as arch
    cases = {}
    for name in NAMES:
        for use_fp16 in (False, True):
            kw = dict(arch.NAMED_CONFIGS[name], use_fp16=use_fp16)
            with torch.device('meta'):
                cases[f'{name}/use_fp16={int(use_fp16)}'] = record(EDMPrecond(**kw))
    with open(os.path.join(solvers_dir, 'solver_utils.py')) as fh:
        fns = [n.name for n in ast.parse(fh.read()).body if isinstance(n, ast.FunctionDef)]
    text = json.dumps(dict(source='diff-solvers-main/models/networks_edm.py EDMPrecond, built on the meta device', cases=cases,
                           solver_utils_functions=fns), separators=(',', ':'))
    with open(OUT, 'wb') as fh:
        fh.write(gzip.compress(text.encode(), mtime=0))
    print(OUT, os.path.getsize(OUT), 'bytes,', len(cases), 'cases')


if __name__ == '__main__':
    main()
