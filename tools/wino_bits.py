"""sha256 of the output and of the statistics of the Winograd convolution (csrc/conv3x3_wino.hip) on the 40 cases of tests/_conv_randn.py
(WINO_GROUPS, built by its wino_args): a change to the kernel that claims bit identity is run once from each tree and the two listings
compared.  Each line carries the label under which profiles/wino_*_ab.txt recorded the case (the test file that held its group then).

    python tools/wino_bits.py [--root TREE] [--out FILE]

--root: the tree whose diff_sampler_amd (and built library) is measured -- default this one; the cases always come from this tree's tests,
so a tree from before a case existed can be measured on the same inputs."""
import argparse
import ctypes as C
import hashlib
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABELS = {'pipe': 'test_hip_wino_pipe', 'base': 'test_hip_wino', 'pipe2': 'test_hip_wino_pipe2', 'kloop': 'test_hip_wino_kloop',
          'persist': 'test_hip_wino_persist'}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=HERE)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, os.path.join(HERE, 'tests'))
    sys.path.insert(0, root)
    import torch
    import diff_sampler_amd
    from diff_sampler_amd import _lib
    import _conv_randn as R
    assert os.path.dirname(os.path.dirname(os.path.abspath(diff_sampler_amd.__file__))) == root
    lib = _lib.load()
    lines = [f'# tree {os.path.relpath(root, HERE)}  library {os.path.relpath(_lib.LIB_PATH, root)}']
    for group, label in LABELS.items():
        for name, row in R.WINO_GROUPS[group].items():
            args, out, stats, keep = R.wino_args(row, 'cuda')
            rc = lib.ds_conv2d_nhwc(C.byref(args), _lib.stream_ptr())
            torch.cuda.synchronize()
            assert rc == 0, lib.ds_error_string(rc)
            h = [hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for t in (out, stats)]
            lines.append(f'{label}::{name}  {tuple(row[1:8])}  out {h[0]}  stats {h[1]}')
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
