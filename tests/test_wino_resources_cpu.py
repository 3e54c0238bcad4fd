"""No GPU: the Winograd convolution (csrc/conv3x3_wino.hip) compiled for gfx950, and the compiler's resource remarks of every instantiation of
conv3x3_wino_kernel.  The kernel is built around one wave per SIMD with the whole register file (256 accumulator registers per wave, the
MFMA block of a slab pinned slot by slot); a change that pushes a value of the K loop or of the skip-slab loop into scratch, or that lets
the compiler settle for fewer registers and a second wave, changes what profiles/ measured.  The bounds are the figures of the kernel
before the skip-slab loop was pipelined (profiles/wino_pipe_isa.txt): one wave per SIMD, 256 + 256 registers, 24 bytes of scratch per lane."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PARENT_WAVES_PER_SIMD = 1
PARENT_REGISTERS = 512          # 256 VGPR + 256 AGPR
PARENT_SCRATCH_BYTES = 24       # 5 spilled VGPRs, all outside the loops


def test_winograd_kernel_keeps_one_wave_per_simd_and_the_parents_scratch():
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    src = os.path.join(ROOT, 'diff_sampler_amd', 'csrc', 'conv3x3_wino.hip')
    r = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '--cuda-device-only', '-c', src, '-o', os.devnull,
                        '-Rpass-analysis=kernel-resource-usage'], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    found = re.findall(r'Function Name: (\S*conv3x3_wino_kernelILi0ELi(\d)ELi(\d)E\S*).*?VGPRs: (\d+).*?AGPRs: (\d+).*?'
                       r'ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)', r.stderr, flags=re.S)
    # normalisation none / affine / affine + SiLU x 3 or 4 halo slots
    assert sorted((int(n), int(s)) for _, n, s, *_ in found) == [(n, s) for n in (0, 1, 2) for s in (3, 4)], r.stderr[-1500:]
    for name, norm, nsl, vgpr, agpr, scratch, waves in found:
        print(f'conv3x3_wino_kernel<0, {norm}, {nsl}>: {vgpr} VGPR + {agpr} AGPR, {scratch} bytes of scratch, {waves} wave(s) per SIMD')
        assert int(waves) == PARENT_WAVES_PER_SIMD, name
        assert int(vgpr) + int(agpr) <= PARENT_REGISTERS, name
        assert int(scratch) <= PARENT_SCRATCH_BYTES, name
