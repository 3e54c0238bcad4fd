"""No GPU: the Winograd convolution (csrc/conv3x3_wino.hip) compiled ONCE for gfx950, and the compiler's resource remarks and assembly of every
instantiation of its three kernels.

conv3x3_wino_kernel and wino_n128_kernel are built around one wave per SIMD with the whole register file (256 accumulator registers per
wave, the MFMA block of a slab pinned slot by slot); a change that pushes a value of the K loop or of the skip-slab loop into scratch, or
that lets the compiler settle for fewer registers and a second wave, changes what profiles/ measured (profiles/wino_pipe_isa.txt: one wave
per SIMD, 256 + 256 registers, 24 bytes of scratch per lane, the figures of the first kernel before the skip-slab loop was pipelined;
profiles/wino_n128_ab.txt).  wino_w8_kernel exists to put TWO waves on every SIMD (eight waves of at most 256 registers, 128 of them
accumulators); a ninth register over 256 halves that to one wave with half the work each (profiles/wino_w8_ab.txt).  For the two 32 x 128
kernels the assembly is parsed too: no scratch instruction in any loop, and exactly two loops (the K loop and the skip-slab loop)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PARENT_WAVES_PER_SIMD = 1
PARENT_REGISTERS = 512          # 256 VGPR + 256 AGPR
PARENT_SCRATCH_BYTES = 24       # 5 spilled VGPRs, all outside the loops


@pytest.fixture(scope='module')
def compiled(tmp_path_factory):
    """(the compiler's remarks, the assembly) of csrc/conv3x3_wino.hip"""
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    src = os.path.join(ROOT, 'diff_sampler_amd', 'csrc', 'conv3x3_wino.hip')
    asm = str(tmp_path_factory.mktemp('wino') / 'conv3x3_wino.s')
    r = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '--cuda-device-only', '-S', src, '-o', asm,
                        '-Rpass-analysis=kernel-resource-usage'], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    with open(asm) as fh:
        return r.stderr, fh.read()


def _loops(text, name):
    """(loops, MFMAs in loops, scratch instructions in loops) of one kernel's assembly"""
    body = re.search(r'^%s:.*?^\s*s_endpgm' % re.escape(name), text, flags=re.S | re.M)
    assert body, name
    # basic blocks as the assembler prints them: a label's comment says whether the block lies in a loop
    in_loop, loops, mfma_in_loops, scratch_in_loops = False, 0, 0, []
    for line in body.group(0).split('\n'):
        if re.match(r'^\.LBB\d+_\d+:', line):
            in_loop = 'Loop' in line
            loops += 'Loop Header' in line
        elif in_loop:
            ins = line.strip()
            mfma_in_loops += ins.startswith('v_mfma_f32_32x32x2_f32')
            if ins.startswith('scratch_'):
                scratch_in_loops.append(ins)
    return loops, mfma_in_loops, scratch_in_loops


def test_winograd_kernel_keeps_one_wave_per_simd_and_the_parents_scratch(compiled):
    remarks, _ = compiled
    found = re.findall(r'Function Name: (\S*conv3x3_wino_kernelILi0ELi(\d)ELi(\d)E\S*).*?VGPRs: (\d+).*?AGPRs: (\d+).*?'
                       r'ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)', remarks, flags=re.S)
    # normalisation none / affine / affine + SiLU x 3 or 4 halo slots
    assert sorted((int(n), int(s)) for _, n, s, *_ in found) == [(n, s) for n in (0, 1, 2) for s in (3, 4)], remarks[-1500:]
    for name, norm, nsl, vgpr, agpr, scratch, waves in found:
        print(f'conv3x3_wino_kernel<0, {norm}, {nsl}>: {vgpr} VGPR + {agpr} AGPR, {scratch} bytes of scratch, {waves} wave(s) per SIMD')
        assert int(waves) == PARENT_WAVES_PER_SIMD, name
        assert int(vgpr) + int(agpr) <= PARENT_REGISTERS, name
        assert int(scratch) <= PARENT_SCRATCH_BYTES, name


def test_n128_kernel_keeps_one_wave_per_simd_and_no_scratch_in_its_loops(compiled):
    remarks, text = compiled
    found = re.findall(r'Function Name: (\S*wino_n128_kernelILi(\d)ELi(\d)EE\S*).*?VGPRs: (\d+).*?AGPRs: (\d+).*?'
                       r'ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)', remarks, flags=re.S)
    # normalisation none / affine / affine + SiLU x 2 or 3 halo slots
    assert sorted((int(n), int(s)) for _, n, s, *_ in found) == [(n, s) for n in (0, 1, 2) for s in (2, 3)], remarks[-1500:]
    for name, norm, nsl, vgpr, agpr, scratch, waves in found:
        loops, mfma_in_loops, scratch_in_loops = _loops(text, name)
        print(f'wino_n128_kernel<{norm}, {nsl}>: {vgpr} VGPR + {agpr} AGPR, {scratch} bytes of scratch, {waves} wave(s) per SIMD, '
              f'{loops} loops with {mfma_in_loops} MFMAs and {len(scratch_in_loops)} scratch instructions')
        assert int(waves) == 1, name
        assert int(vgpr) + int(agpr) <= 512, name              # 256 VGPR + 256 AGPR
        assert int(scratch) <= 24, name                        # the bytes per lane the project allows the first kernel
        assert loops == 2 and mfma_in_loops == 128, name       # the K loop and the skip-slab loop, 64 MFMAs per slab each: the parse saw them
        assert not scratch_in_loops, (name, scratch_in_loops[:4])


def test_w8_kernel_keeps_two_waves_per_simd_and_no_scratch_in_its_loops(compiled):
    remarks, text = compiled
    found = re.findall(r'Function Name: (\S*wino_w8_kernelILi(\d)EE\S*).*?VGPRs: (\d+).*?AGPRs: (\d+).*?'
                       r'ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)', remarks, flags=re.S)
    # normalisation none / affine / affine + SiLU; one halo slot per thread (the kernel is built for 16- and 32-column images only: at 64
    # columns, the width that needs a second slot, it was measured no faster than wino_n128_kernel)
    assert sorted(int(n) for _, n, *_ in found) == [0, 1, 2], remarks[-1500:]
    for name, norm, vgpr, agpr, scratch, waves in found:
        loops, mfma_in_loops, scratch_in_loops = _loops(text, name)
        print(f'wino_w8_kernel<{norm}>: {vgpr} VGPR + {agpr} AGPR, {scratch} bytes of scratch, {waves} wave(s) per SIMD, '
              f'{loops} loops with {mfma_in_loops} MFMAs and {len(scratch_in_loops)} scratch instructions')
        assert int(waves) == 2, name
        assert int(vgpr) + int(agpr) <= 256, name              # VGPR + AGPR
        assert int(scratch) <= 24, name                        # the bytes per lane the project allows the other two kernels
        assert loops == 2 and mfma_in_loops == 64, name        # the K loop and the skip-slab loop, 32 MFMAs per slab and wave each
        assert not scratch_in_loops, (name, scratch_in_loops[:4])
