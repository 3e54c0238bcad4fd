"""No GPU: the 32-tile x 128-channel Winograd kernel (wino_n128_kernel in csrc/conv3x3_wino.hip) compiled for gfx950, in the manner of
tests/test_wino_resources_cpu.py: the compiler's resource remarks of every instantiation, and its assembly.  The kernel is built like the
first one -- one wave per SIMD with the whole register file, 256 accumulator registers per wave, the MFMA block of a slab pinned slot by
slot -- so a second wave per SIMD, or a value of the K loop or of the skip-slab loop pushed into scratch, changes what
profiles/wino_n128_ab.txt measured.  Bounds: one wave per SIMD, at most 512 registers, at most the 24 bytes of scratch per lane the
project allows the first kernel, and no scratch instruction in any loop (the kernel's only loops are the K loop and the skip-slab loop)."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WAVES_PER_SIMD = 1
REGISTERS = 512                 # 256 VGPR + 256 AGPR
SCRATCH_BYTES = 24


def test_n128_kernel_keeps_one_wave_per_simd_and_no_scratch_in_its_loops(tmp_path):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    src = os.path.join(ROOT, 'diff_sampler_amd', 'csrc', 'conv3x3_wino.hip')
    asm = str(tmp_path / 'conv3x3_wino.s')
    r = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '--cuda-device-only', '-S', src, '-o', asm,
                        '-Rpass-analysis=kernel-resource-usage'], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    found = re.findall(r'Function Name: (\S*wino_n128_kernelILi(\d)ELi(\d)EE\S*).*?VGPRs: (\d+).*?AGPRs: (\d+).*?'
                       r'ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)', r.stderr, flags=re.S)
    # normalisation none / affine / affine + SiLU x 2 or 3 halo slots
    assert sorted((int(n), int(s)) for _, n, s, *_ in found) == [(n, s) for n in (0, 1, 2) for s in (2, 3)], r.stderr[-1500:]
    with open(asm) as fh:
        text = fh.read()
    for name, norm, nsl, vgpr, agpr, scratch, waves in found:
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
        print(f'wino_n128_kernel<{norm}, {nsl}>: {vgpr} VGPR + {agpr} AGPR, {scratch} bytes of scratch, {waves} wave(s) per SIMD, '
              f'{loops} loops with {mfma_in_loops} MFMAs and {len(scratch_in_loops)} scratch instructions')
        assert int(waves) == WAVES_PER_SIMD, name
        assert int(vgpr) + int(agpr) <= REGISTERS, name
        assert int(scratch) <= SCRATCH_BYTES, name
        assert loops == 2 and mfma_in_loops == 128, name       # the K loop and the skip-slab loop, 64 MFMAs per slab each: the parse saw them
        assert not scratch_in_loops, (name, scratch_in_loops[:4])
