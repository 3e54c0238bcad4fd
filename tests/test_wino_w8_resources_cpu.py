"""No GPU: the eight-wave Winograd kernel (wino_w8_kernel in csrc/conv3x3_wino.hip) compiled for gfx950, in the manner of
tests/test_wino_n128_resources_cpu.py: the compiler's resource remarks of every instantiation, and its assembly.  The kernel exists to
put TWO waves on every SIMD (eight waves of at most 256 registers, 128 of them accumulators); a ninth register over 256 halves that to
one wave with half the work each, and a value of the K loop or of the skip-slab loop pushed into scratch changes what
profiles/wino_w8_ab.txt measured.  Bounds: two waves per SIMD, at most 256 registers, at most the 24 bytes of scratch per lane the project
allows the other two kernels, no scratch instruction in any loop, and exactly two loops (the K loop and the skip-slab loop) with 32 MFMAs
per slab and wave each."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WAVES_PER_SIMD = 2
REGISTERS = 256                 # VGPR + AGPR
SCRATCH_BYTES = 24


def test_w8_kernel_keeps_two_waves_per_simd_and_no_scratch_in_its_loops(tmp_path):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    src = os.path.join(ROOT, 'diff_sampler_amd', 'csrc', 'conv3x3_wino.hip')
    asm = str(tmp_path / 'conv3x3_wino.s')
    r = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '--cuda-device-only', '-S', src, '-o', asm,
                        '-Rpass-analysis=kernel-resource-usage'], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    found = re.findall(r'Function Name: (\S*wino_w8_kernelILi(\d)EE\S*).*?VGPRs: (\d+).*?AGPRs: (\d+).*?'
                       r'ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)', r.stderr, flags=re.S)
    # normalisation none / affine / affine + SiLU; one halo slot per thread (the kernel is built for 16- and 32-column images only: at 64
    # columns, the width that needs a second slot, it was measured no faster than wino_n128_kernel)
    assert sorted(int(n) for _, n, *_ in found) == [0, 1, 2], r.stderr[-1500:]
    with open(asm) as fh:
        text = fh.read()
    for name, norm, vgpr, agpr, scratch, waves in found:
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
        print(f'wino_w8_kernel<{norm}>: {vgpr} VGPR + {agpr} AGPR, {scratch} bytes of scratch, {waves} wave(s) per SIMD, '
              f'{loops} loops with {mfma_in_loops} MFMAs and {len(scratch_in_loops)} scratch instructions')
        assert int(waves) == WAVES_PER_SIMD, name
        assert int(vgpr) + int(agpr) <= REGISTERS, name
        assert int(scratch) <= SCRATCH_BYTES, name
        assert loops == 2 and mfma_in_loops == 64, name        # the K loop and the skip-slab loop, 32 MFMAs per slab and wave each
        assert not scratch_in_loops, (name, scratch_in_loops[:4])
