"""sha256 of the output and of the statistics of the Winograd convolution (csrc/conv3x3_wino.hip) on the cases of tests/test_hip_wino_pipe.py,
tests/test_hip_wino.py, tests/test_hip_wino_pipe2.py, tests/test_hip_wino_kloop.py and tests/test_hip_wino_persist.py (launches of more
tiles than compute units): a change to the kernel that claims bit identity is run once from each tree and the two listings compared.

    python tools/wino_bits.py [--root TREE] [--out FILE]

--root: the tree whose diff_sampler_amd (and built library) is measured -- default this one; the cases always come from this tree's tests,
so a tree from before tests/test_hip_wino_pipe.py existed can be measured on the same inputs."""
import argparse
import ctypes as C
import hashlib
import importlib.util
import os
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(path):
    spec = importlib.util.spec_from_file_location(os.path.basename(path)[:-3], path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--root', default=HERE)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import torch
    import diff_sampler_amd
    from diff_sampler_amd import _lib
    assert os.path.dirname(os.path.dirname(os.path.abspath(diff_sampler_amd.__file__))) == root
    lib = _lib.load()
    lines = [f'# tree {os.path.relpath(root, HERE)}  library {os.path.relpath(_lib.LIB_PATH, root)}']
    for fname, builder in (('test_hip_wino_pipe.py', 'conv_args'), ('test_hip_wino.py', '_args'), ('test_hip_wino_pipe2.py', 'conv_args'),
                           ('test_hip_wino_kloop.py', 'conv_args'), ('test_hip_wino_persist.py', 'conv_args')):
        mod = _load(os.path.join(HERE, 'tests', fname))
        for name in mod.CASES:
            args, out, stats, keep = getattr(mod, builder)(name)
            rc = lib.ds_conv2d_nhwc(C.byref(args), _lib.stream_ptr())
            torch.cuda.synchronize()
            assert rc == 0, lib.ds_error_string(rc)
            h = [hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for t in (out, stats)]
            lines.append(f'{fname[:-3]}::{name}  {tuple(mod.CASES[name][:7])}  out {h[0]}  stats {h[1]}')
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or '.', exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
