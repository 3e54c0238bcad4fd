"""GPU: ordering bugs between the waves of a workgroup made DETERMINISTIC.

Round 5 shipped -- through a green suite -- a kernel in which wave 0 fetched GroupNorm coefficient rows by LDS-DMA and waves 1 - 7 read them
with no barrier in between (docs/HISTORY.md G.5); it failed once, on a cold box.  Bit-equality tests on warm processes cannot see that class.
Two guards live here:

  1. the RACE-STRESS libraries (csrc/ds_common.h DS_RACE_SKEW; diff_sampler_amd/build.py VARIANTS): the same kernels with the waves of a mask
     put to sleep ~2 us right before they produce shared LDS contents (every LDS-DMA issue, every staging ds_write of the hand-scheduled
     kernels, the staging stores of the compiler-scheduled ones).  Mask 0x21 delays waves 0 and 5 -- the single-wave producers arrive late:
     a consumer without wait + barrier reads before the data landed; mask 0xDE delays all the others -- the producers run ahead: an overwrite
     without a barrier hits data still being read.  The kernel suites must pass UNCHANGED against both libraries (a correct kernel's results
     do not depend on timing).  The round-5 bug, re-introduced, fails `test_conv_f16_activations_fused_input_normalisation...` on the first
     case under mask 0x21: `test_the_stress_build_catches_the_round5_race_when_it_is_reintroduced` below asserts exactly that against
     libdsamd_stress_g5.so, on every run of the suite (profiles/r6_race_stress.txt).
  2. the COLD-START comparison: three fresh processes, each building the ImageNet-64 fp16 plans (pass / 'auto' / all-fused normalisation) at the
     benchmark batch and comparing the FIRST evaluation of each -- nothing warmed, no earlier launch of the same kernels in the process.

`DS_STRESS_FULL=1` runs the whole of tests/test_hip_kernels.py + tests/test_hip_fp16.py under both libraries (what profiles/r6_race_stress.txt
records: 362 passed / 41 skipped under each mask); the default selection keeps the driver's suite short: the tests of every kernel with
hand-placed waits and raw barriers."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

# the default selection: every test of the kernels that order their own LDS traffic with raw s_barrier + counted waits (conv3x3_f16dma incl. its
# fused normalisation and split-K, gemm_f16dma incl. the gather form, conv3x3_halo2 split mode, gemm_f16) and of the fp16 attention staging
HAND_SCHEDULED = ('f16_activations or f16_operands or split_fp16 or gather_kernel or fused_input_normalisation or without_the_lds_transpose '
                  'or fp16_residual or geglu_fused or fused_attention_f16 or fused_attention_reads or two_query_blocks or channel_split')


def _run_suite(lib, args, timeout):
    env = dict(os.environ, DS_LIB_PATH=lib, DS_AUTOTUNE='0')          # no tile measurement launches: every launch is a product launch
    cmd = [sys.executable, '-m', 'pytest', '-x', '-q', '-m', 'gpu', '-p', 'no:cacheprovider'] + args
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    tail = (r.stdout or '')[-3000:] + (r.stderr or '')[-1500:]
    assert r.returncode == 0, f'{os.path.basename(lib)}: {" ".join(args)}\n{tail}'
    return r.stdout.strip().splitlines()[-1]


@pytest.mark.parametrize('tag', ['stress_a', 'stress_b'])
def test_kernel_suites_pass_against_the_race_stress_library(tag):
    from diff_sampler_amd import build
    lib = build.variant_lib(tag)
    assert os.path.exists(lib), f'{lib} is missing: __graft_entry__.build() / python -m diff_sampler_amd.build --variants builds it'
    flags = ctypes.CDLL(lib).ds_build_experiments()
    assert flags & 2, 'not a DS_RACE_STRESS build'
    from diff_sampler_amd import _lib
    assert not _lib.load().ds_build_experiments() & 2, 'the product library must not carry the delays'
    if os.environ.get('DS_STRESS_FULL') == '1':
        summary = _run_suite(lib, ['tests/test_hip_kernels.py', 'tests/test_hip_fp16.py'], timeout=3000)
    else:
        summary = _run_suite(lib, ['tests/test_hip_kernels.py', '-k', HAND_SCHEDULED], timeout=1500)
    os.makedirs(os.path.join(ROOT, 'gpurun_out'), exist_ok=True)
    with open(os.path.join(ROOT, 'gpurun_out', f'race_stress_{tag}.txt'), 'w') as f:
        f.write(summary + '\n')
    assert 'passed' in summary and 'failed' not in summary, summary


# seconds.  The four children this one replaces took 17.8 s together on a warm box (profiles/wino_tests_merge.txt) under limits that summed
# to 2700 s: 300 s is 17 times the former and a ninth of the latter, so that a cold box passes and a hung child costs five minutes
WINO_CHILD_TIMEOUT = 300


@pytest.mark.parametrize('tag', ['stress_a', 'stress_b'])
def test_winograd_suite_passes_against_the_race_stress_library(tag):
    """The whole of tests/test_hip_wino.py, unchanged, against a library whose LDS-producing waves are delayed (two complementary wave
    masks): every producer of shared LDS contents in csrc/conv3x3_wino.hip is a DS_RACE_SKEW site."""
    from diff_sampler_amd import build
    lib = build.variant_lib(tag)
    assert os.path.exists(lib), f'{lib} is missing: __graft_entry__.build() / python -m diff_sampler_amd.build --variants builds it'
    assert ctypes.CDLL(lib).ds_build_experiments() & 2, 'not a DS_RACE_STRESS build'
    summary = _run_suite(lib, ['tests/test_hip_wino.py'], timeout=WINO_CHILD_TIMEOUT)
    assert 'passed' in summary and 'failed' not in summary and 'skipped' not in summary, summary


def test_the_stress_build_catches_the_round5_race_when_it_is_reintroduced():
    """The detector detects: libdsamd_stress_g5.so = the mask-0x21 stress library with conv3x3_f16dma.hip's prologue barrier compiled OUT
    (-DDS_TEST_DROP_G5_BARRIER: exactly the round-5 bug -- coefficient rows fetched by wave 0, read by every wave).  Round 5's suite passed
    over that code; against this library the fused-normalisation kernel test must FAIL, on every run."""
    from diff_sampler_amd import build
    lib = build.variant_lib('stress_g5')
    assert os.path.exists(lib) and ctypes.CDLL(lib).ds_build_experiments() & 2
    env = dict(os.environ, DS_LIB_PATH=lib, DS_AUTOTUNE='0')
    cmd = [sys.executable, '-m', 'pytest', '-x', '-q', '-m', 'gpu', '-p', 'no:cacheprovider', 'tests/test_hip_kernels.py', '-k', 'fused_input_normalisation']
    for attempt in range(2):                                        # deterministic, not "once per cold box"
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 1 and ' failed' in r.stdout, (attempt, r.stdout[-1500:], r.stderr[-500:])


_COLD = r'''
import hashlib, sys, torch
sys.path.insert(0, %(root)r)
from diff_sampler_amd.engine import EDMDenoiser
order = %(order)r
B = 64
net = EDMDenoiser.from_config('imagenet64', seed=62, use_fp16=True)
g = torch.Generator().manual_seed(3)
x = (torch.randn(B, 3, 64, 64, generator=g) * 0.7).cuda()
sig = torch.full((B,), 0.7); sig[::7] = 1.3
sig = sig.cuda()
lab = torch.eye(1000)[torch.randint(1000, (B,), generator=g)].cuda()
for mode in order:
    net.engine.fuse_norm16 = mode
    o = net(x, sig, class_labels=lab)                 # the FIRST evaluation of this plan (and, for order[0], of the process)
    torch.cuda.synchronize()
    assert torch.isfinite(o).all(), mode
    print('HASH', mode, hashlib.sha256(o.cpu().numpy().tobytes()).hexdigest(), flush=True)
'''


def test_first_evaluation_after_a_plan_build_is_bit_identical_in_fresh_processes():
    """tools/diag_fuse_norm.py as a test: ImageNet-64 `use_fp16` at the benchmark batch (64 images, per-sample sigma, labels); the plan with
    ds_norm_act passes, the default 'auto' plan and the all-fused plan compute the same bits (tests/test_hip_fp16.py shows it warm).  Here each
    of three FRESH processes runs the three plans in a rotated order and hashes the first output of each: every plan is once the very first
    thing its process launches.  One hash overall -- across plans, across processes."""
    modes = [False, 'auto', True]
    seen = {}
    for rot in range(3):
        order = modes[rot:] + modes[:rot]
        r = subprocess.run([sys.executable, '-c', _COLD % dict(root=ROOT, order=order)], cwd=ROOT, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        for line in r.stdout.splitlines():
            if line.startswith('HASH '):
                _, mode, h = line.split()
                seen[(rot, mode)] = h
    assert len(seen) == 9, seen
    assert len(set(seen.values())) == 1, seen
