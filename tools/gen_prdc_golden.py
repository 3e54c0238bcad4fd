"""Regenerate tests/golden/prdc_small.npz from the REFERENCE implementation (sfd-main/prdc.py), on the CPU.

    python tools/gen_prdc_golden.py --reference /path/to/sfd-main/prdc.py

The reference module cannot be imported as it stands (it imports torchvision-era training code at the top); its four pure functions --
compute_pairwise_distance, get_kth_value, compute_nearest_neighbour_distances, compute_prdc -- need numpy and sklearn only.  The file is
parsed at generation time, those four FunctionDefs are compiled on their own into a namespace holding ``np`` and ``sklearn.metrics``, and
run as they are.  Nothing of the reference's text is copied into this repository: the golden holds inputs and recorded results only.

Cases: the correlated-Gaussian generator of tests/test_hip_fid.py with a shifted fake set, fp32 values (handed to the reference as fp64,
as its feature extractor does).  Each case is checked for a decision gap before it is written: no distance that a comparison decides may
lie within 1e-9 (relative) of its radius, so that the four metrics are the same numbers in any summation order.
"""
import argparse
import ast
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WANTED = ('compute_pairwise_distance', 'get_kth_value', 'compute_nearest_neighbour_distances', 'compute_prdc')
CASES = (dict(name='a', n_real=300, n_fake=257, dim=64, k=5, seed=11, shift=0.15),
         dict(name='b', n_real=37, n_fake=41, dim=7, k=5, seed=12, shift=0.3),
         dict(name='c', n_real=200, n_fake=180, dim=32, k=3, seed=13, shift=0.1))


def features(n, d, seed, shift=0.0):
    g = np.random.RandomState(seed)
    a = g.randn(d, d) / np.sqrt(d)
    return (g.randn(n, d) @ a + shift + 0.3 * g.randn(d)).astype(np.float32)


def reference_functions(path):
    import sklearn.metrics
    with open(path, 'r', encoding='utf-8') as fh:
        tree = ast.parse(fh.read(), filename=path)
    defs = [node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name in WANTED]
    assert sorted(d.name for d in defs) == sorted(WANTED), [d.name for d in defs]
    ns = dict(np=np, sklearn=__import__('sklearn'))
    ns['sklearn'].metrics = sklearn.metrics
    exec(compile(ast.Module(body=defs, type_ignores=[]), path, 'exec'), ns)
    return ns


def decision_gap(ref, real, fake, k):
    """Smallest relative distance between a compared value and its radius, over every comparison compute_prdc makes."""
    rr = ref['compute_nearest_neighbour_distances'](real, k)
    rf = ref['compute_nearest_neighbour_distances'](fake, k)
    d = ref['compute_pairwise_distance'](real, fake)
    gaps = [np.abs(d - rr[:, None]) / rr[:, None], np.abs(d - rf[None, :]) / rf[None, :], (np.abs(d.min(1) - rr) / rr)[:, None]]
    return min(float(g.min()) for g in gaps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reference', required=True, help='path of the reference prdc.py')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'prdc_small.npz'))
    args = ap.parse_args()
    ref = reference_functions(args.reference)
    out = {'cases': np.array([c['name'] for c in CASES])}
    for c in CASES:
        real = features(c['n_real'], c['dim'], c['seed'])
        fake = features(c['n_fake'], c['dim'], c['seed'] + 1000, shift=c['shift'])
        r64, f64 = real.astype(np.float64), fake.astype(np.float64)
        gap = decision_gap(ref, r64, f64, c['k'])
        assert gap >= 1e-9, (c, gap)
        res = ref['compute_prdc'](r64, f64, c['k'], realism=True)
        p = c['name'] + '_'
        out[p + 'real'], out[p + 'fake'], out[p + 'k'] = real, fake, np.int64(c['k'])
        out[p + 'radii_real'] = ref['compute_nearest_neighbour_distances'](r64, c['k'])
        out[p + 'radii_fake'] = ref['compute_nearest_neighbour_distances'](f64, c['k'])
        for key in ('precision', 'recall', 'density', 'coverage', 'realism'):
            out[p + key] = np.asarray(res[key], dtype=np.float64)
        print(c['name'], {k: float(res[k]) for k in ('precision', 'recall', 'density', 'coverage')}, 'decision gap %.2e' % gap)
    np.savez_compressed(args.out, **out)
    print('wrote', args.out, os.path.getsize(args.out), 'bytes')


if __name__ == '__main__':
    main()
