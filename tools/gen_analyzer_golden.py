"""Regenerate tests/golden/analyzer_small.npz from the REFERENCE (diff-analyzer-main), on the CPU.

    python tools/gen_analyzer_golden.py --reference /path/to/diff-analyzer-main

Neither utils.py (it imports torchvision, IPython and the training code at the top) nor a notebook can be imported.  Both are parsed at
generation time -- utils.py as Python, main_extend.ipynb as JSON whose code cells are parsed one by one -- the FunctionDef of
``cal_deviation`` and of ``cal_curv_tors`` is compiled on its own into a namespace holding ``torch`` / ``np``, and run as it is.  Nothing of
the reference's text is copied into this repository: the golden holds inputs and recorded results only.

Recorded:
  dev_*   ``cal_deviation`` on a [7, 3, 3, 4, 4] fp32 random walk (its own fp32 arithmetic), and the same function on the input cast to fp64
  curv_*  ``cal_curv_tors`` (with the arc length, computed here as the notebook's cell computes it) on two 3-D curves of T = 61 points,
          window_size 11: a helix, and a non-planar curve sampled at non-uniform parameter values
"""
import argparse
import ast
import json
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def function_from_source(text, name, ns, filename):
    try:
        tree = ast.parse(text, filename=filename)
    except SyntaxError:
        return None
    defs = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name == name]
    if not defs:
        return None
    exec(compile(ast.Module(body=defs[:1], type_ignores=[]), filename, 'exec'), ns)
    return ns[name]


def reference_functions(ref_dir):
    path = os.path.join(ref_dir, 'utils.py')
    with open(path, 'r', encoding='utf-8') as fh:
        dev = function_from_source(fh.read(), 'cal_deviation', dict(torch=torch), path)
    assert dev is not None, 'cal_deviation not found in ' + path
    path = os.path.join(ref_dir, 'main_extend.ipynb')
    with open(path, 'r', encoding='utf-8') as fh:
        nb = json.load(fh)
    curv = None
    for cell in nb['cells']:
        if cell['cell_type'] == 'code' and curv is None:
            curv = function_from_source(''.join(cell['source']), 'cal_curv_tors', dict(np=np), path)
    assert curv is not None, 'cal_curv_tors not found in ' + path
    return dev, curv


def random_walk(seed=0, shape=(7, 3, 3, 4, 4)):
    g = torch.Generator().manual_seed(seed)
    return 3 * torch.cumsum(torch.randn(shape, generator=g), dim=0)


def curves(T=61):
    """xs, ys, zs [T, 2]: column 0 a helix, column 1 a twisted cubic-like curve at non-uniformly spaced parameter values."""
    u = np.linspace(0.0, 3.0, T)
    w = 2.0 * (np.linspace(0.0, 1.0, T) ** 1.7) + 0.2
    xs = np.stack([2.0 * np.cos(u), w], axis=1)
    ys = np.stack([2.0 * np.sin(u), 0.5 * w ** 2 + 0.3 * np.sin(2 * w)], axis=1)
    zs = np.stack([0.7 * u, 0.2 * w ** 3 - 0.4 * w], axis=1)
    return xs, ys, zs


def polygon_length(xs, ys, zs):
    p = np.stack([xs, ys, zs], axis=1)
    seg = np.linalg.norm(p[1:] - p[:-1], axis=1)
    return np.cumsum(np.concatenate((np.zeros((1, seg.shape[1])), seg), axis=0), axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='directory of the reference diff-analyzer-main')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'analyzer_small.npz'))
    args = ap.parse_args()
    cal_deviation, cal_curv_tors = reference_functions(args.reference)
    out = {}
    traj = random_walk()
    n, B, ch, r = traj.shape[0], traj.shape[1], traj.shape[2], traj.shape[3]
    out['dev_traj'] = traj.numpy()
    out['dev_f32'] = cal_deviation(traj, ch, r, B).numpy()                            # [B, n - 2]
    out['dev_f64'] = cal_deviation(traj.to(torch.float64), ch, r, B).numpy()
    xs, ys, zs = curves()
    s = polygon_length(xs, ys, zs)
    window = 11
    curvatures, torsions = cal_curv_tors(xs, ys, zs, s, window)
    assert np.isfinite(curvatures).all() and np.isfinite(torsions).all()
    out.update(curv_xs=xs, curv_ys=ys, curv_zs=zs, curv_s=s, curv_window=np.int64(window), curv_curvatures=curvatures, curv_torsions=torsions)
    np.savez_compressed(args.out, **out)
    print('deviation fp32 vs fp64: %.2e relative' % float(np.abs(out['dev_f32'] - out['dev_f64']).max() / np.abs(out['dev_f64']).max()))
    print('helix curvature %.6f .. %.6f (2 / 4.49 = %.6f), torsion %.6f .. %.6f' % (curvatures[:, 0].min(), curvatures[:, 0].max(), 2 / 4.49,
                                                                                   torsions[:, 0].min(), torsions[:, 0].max()))
    print('wrote', args.out, os.path.getsize(args.out), 'bytes')


if __name__ == '__main__':
    main()
