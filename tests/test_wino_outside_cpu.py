"""No GPU: the structure of wino_w8_kernel (csrc/conv3x3_wino.hip) OUTSIDE its K loop, read off the assembly the compiler makes for gfx950
(the compile, the remarks and the block parse of tests/test_wino_resources_cpu.py).  A workgroup of this kernel holds a whole compute unit,
so nothing overlaps what it does outside the loops, and the fp32 MFMA shares the VALU: profiles/wino_outside_isa.txt counts what was taken
out there.  Structure only, no measurement -- for each of the three instantiations:
  * the first halo request stands in front of the first LDS write: the loads of halo 0 and 1 are on their way while the rest of the set-up
    (LDS cells, zero cells, transform and fragment indices) runs;
  * no accumulator is zeroed with moves in front of the K loop: the peeled first slab takes the constant 0 as the C operand of its first K
    step (the parent zeroed eight accumulators with 128 v_mov_b32: one of the
    constant 0 and 127 copies of it);
  * no v_cndmask_b32 between the K loop's exit and the skip-slab loop: the exchange branches on the wave's half as a scalar (the parent
    selected 64 registers per lane) and the tail's early requests select their source without one."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_wino_resources_cpu import compiled  # noqa: F401  (the module-scoped fixture: one compile of conv3x3_wino.hip)


def _instructions(text, name):
    """[(opcode, operands, loop)] of one kernel in layout order; loop = 0 for the blocks of the first loop the layout meets (the K loop), 1
    for the second (the skip-slab loop), -1 outside.  A block belongs to the loop whose header its label's comment names."""
    body = re.search(r'^%s:.*?^\s*s_endpgm' % re.escape(name), text, flags=re.S | re.M)
    assert body, name
    out, cur, ids = [], -1, {}
    for line in body.group(0).split('\n')[1:]:
        m = re.match(r'^(?:\.L(BB\d+_\d+)|; %bb\.\d+):(.*)', line)
        if m:
            h = re.search(r'Header=(BB\d+_\d+)', m.group(2))
            cur = ids.setdefault(m.group(1), len(ids)) if 'Loop Header' in m.group(2) else ids.setdefault(h.group(1), len(ids)) if h else -1
            continue
        ins = line.split(';')[0].strip()
        if ins and not ins.startswith('.') and not ins.endswith(':'):
            op, _, rest = ins.partition('\t') if '\t' in ins else ins.partition(' ')
            out.append((op, rest.strip(), cur))
    return out


@pytest.fixture(scope='module')
def w8_kernels(compiled):  # noqa: F811
    remarks, text = compiled
    names = sorted(set(re.findall(r'Function Name: (\S*wino_w8_kernelILi\dEE\S*)', remarks)))
    assert len(names) == 3, names
    return {name: _instructions(text, name) for name in names}


def _regions(ins):
    k = [i for i, x in enumerate(ins) if x[2] == 0]
    s = [i for i, x in enumerate(ins) if x[2] == 1]
    assert k and s and max(k) < min(s), 'the K loop and, behind it, the skip-slab loop'
    assert sum(x[0].startswith('v_mfma') for x in ins[min(k):max(k) + 1]) == 32 and sum(x[0].startswith('v_mfma') for x in ins[min(s):max(s) + 1]) == 32
    return min(k), max(k), min(s)


def test_first_halo_request_stands_in_front_of_the_first_lds_write(w8_kernels):
    for name, ins in w8_kernels.items():
        load = next(i for i, x in enumerate(ins) if x[0].startswith('global_load'))
        write = next(i for i, x in enumerate(ins) if x[0].startswith('ds_write'))
        print(f'{name}: first global_load is instruction {load}, first ds_write {write}')
        assert load < write, name


def test_no_accumulator_is_zeroed_with_moves_in_front_of_the_k_loop(w8_kernels):
    for name, ins in w8_kernels.items():
        k0, _, _ = _regions(ins)
        # the parent zeroed with ONE v_mov_b32 v, 0 and 127 copies of that register, so every 32-bit register move counts
        moves = [x for x in ins[:k0] if x[0].startswith('v_mov_b32')]
        # the peeled slab's MFMAs are there, and their first K steps take the inline constant
        first = [x for x in ins[:k0] if x[0].startswith('v_mfma')]
        print(f'{name}: {len(moves)} v_mov_b32 in front of the K loop, {len(first)} MFMAs of the peeled slab, '
              f'{sum(x[1].endswith(", 0") for x in first)} with the constant 0 as C')
        assert len(moves) < 16, name                         # one accumulator is 16 registers
        assert len(first) == 32 and sum(x[1].endswith(', 0') for x in first) == 8, name


def test_no_select_between_the_k_loop_and_the_skip_slab_loop(w8_kernels):
    for name, ins in w8_kernels.items():
        _, k1, s0 = _regions(ins)
        cnd = [x for x in ins[k1 + 1:s0] if x[0].startswith('v_cndmask_b32')]
        print(f'{name}: {s0 - k1 - 1} instructions between the K loop and the skip-slab loop, {len(cnd)} v_cndmask_b32')
        assert not cnd, (name, cnd[:4])
