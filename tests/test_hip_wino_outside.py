"""GPU: what wino_w8_kernel (csrc/conv3x3_wino.hip, the default at 16 and 32 columns) does OUTSIDE its K loop.  Slab 0 is peeled in front
of the loop and takes the constant 0 as the C operand of its first K step (no accumulator is zeroed); halo 0 and 1 and the first weight
fragments are requested before the rest of the set-up; behind the K loop's last barrier the skip loop's weights of slab 0 and pixels of
slabs 0 and 1, the column bias, the image's cbias row and the eight residual quads of the wave's patch row are requested in front of the
exchange; the exchange and the epilogue branch on the wave's half, p.cbias, p.res and p.act as scalars; the epilogue's and the residual's
addresses are a scalar row base plus one lane offset.  None of it may change a bit: each case runs on the default route, on
ds_conv_tune.variant bit 15 (wino_n128_kernel) and on bit 10 (conv3x3_wino_kernel) and must give THE SAME BITS of the output and of the
statistics, on top of the fp64 bound of tests/_conv_randn.py (2e-5 of the absmax), the GroupNorm statistics ds_gn_finalize makes of the
column sums, NaN margins left alone and a second launch with the same bits.

The cases are the smallest at which that code can go wrong (a K slab is 8 input channels, a skip slab 32 channels of the appended 1x1
projection; an M tile is 128 pixels of one image; cout = 256 throughout):
  one slab                        the peeled slab is the whole K loop: the loop is not entered
  two slabs                       the loop runs once
  8 + 8 channels                  the a0 | a1 boundary right behind the peeled slab
  three slabs                     odd count, the look-ahead clamped in the loop's last round
  two images, cbias and res       the second image's tiles take their own cbias row and their own residual rows in the early requests
  one skip slab                   the early skip requests with nextra = 1: slab 1's request is slab 0's again
  two skip slabs e0 | e1          nextra = 2 behind one K slab: the second early request reads the other source
  32x32, res + SiLU + statistics  the other width of the shifts and of the scalar row bases, the whole epilogue
Two slabs, the two images and the two skip slabs run under every instantiation: normalisation none, affine, affine + SiLU."""
import ctypes as C
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import _conv_randn as R  # noqa: E402

pytestmark = pytest.mark.gpu

# ds_conv_tune.variant: bit 15 = wino_n128_kernel (four waves on the same tile), bit 10 = the 64-tile x 64-channel workgroups; the first
# entry is the default route, wino_w8_kernel at these widths
SHAPES = (('default', 0), ('n128', 32768), ('64x64', 1024))
NORMS = {0: (), 1: ('norm', 'noact'), 2: ('norm',)}          # WinoHalo's NORM -> the features that select it

# name: (seed, B, H, c0, c1, cout, ec0, ec1, features besides the normalisation, NORMs it runs under)
BASE = {
    'one_slab_the_peeled_slab_is_the_whole_k_loop': (7600, 1, 16, 8, 0, 256, 0, 0, (), (2,)),
    'two_slabs': (7601, 1, 16, 16, 0, 256, 0, 0, (), (0, 1, 2)),
    'source_boundary_behind_the_peeled_slab': (7602, 1, 16, 8, 8, 256, 0, 0, (), (2,)),
    'three_slabs_odd_count_clamped_look_ahead': (7603, 1, 16, 24, 0, 256, 0, 0, (), (2,)),
    'two_images_cbias_and_res_per_image': (7604, 2, 16, 16, 0, 256, 0, 0, ('cbias', 'res'), (0, 1, 2)),
    'one_skip_slab': (7605, 1, 16, 8, 0, 256, 32, 0, ('bias',), (2,)),
    'two_skip_slabs_two_sources_behind_one_k_slab': (7606, 1, 16, 8, 0, 256, 32, 32, ('bias',), (0, 1, 2)),
    'res_silu_and_statistics_on_32_columns': (7607, 1, 32, 16, 0, 256, 0, 0, ('res', 'silu'), (2,)),
}
CASES = {f'{name}-norm{n}': row[:8] + (NORMS[n] + row[8],) for name, row in BASE.items() for n in row[9]}


def _launch(lib, row, variant_bits):
    """Route assertion and one launch into fresh NaN-filled guarded buffers, on the kernel `variant_bits` selects."""
    from diff_sampler_amd import _lib
    a, out, stats, keep = R.wino_args(row, 'cuda')
    a.tune.variant |= variant_bits
    info = _lib.ConvRouteInfo()
    rc = lib.ds_conv_route(C.byref(a), C.byref(info))
    assert rc == 0 and info.wino == 1 and info.kernel_id == 2565 and info.splits == 1, (rc, info.wino, info.kernel_id, info.splits)
    rc = lib.ds_conv2d_nhwc(C.byref(a), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib.ds_error_string(rc)
    return out, stats, keep['out_buf'], keep['stats_buf']


@pytest.mark.parametrize('name', list(CASES))
def test_three_kernels_give_the_same_bits_within_the_fp64_bound(name):
    from diff_sampler_amd import _lib
    row = CASES[name]
    seed, B, H, c0, c1, cout, ec0, ec1, feats = row
    lib = _lib.load()
    bufs = {}
    for label, bits in SHAPES:
        out, stats, out_buf, stats_buf = _launch(lib, row, bits)
        err, per, e_s, e_q = R.compare(row, out.cpu(), stats.cpu(), out_buf.cpu(), stats_buf.cpu())
        print(f'wino {label} {name} {row[1:8]}: {(c0 + c1) // 8} slabs + {(ec0 + ec1) // 32} skip slabs, rel err vs fp64 {err:.3e} '
              f'(worst image {per.index(max(per))}), column sums rel err {e_s:.3e} / {e_q:.3e}')
        R.finalize_check(lib, stats, R.make_layer(*row)['ref'], B, H * H, cout)
        again = _launch(lib, row, bits)[2:]              # launch independence: fresh buffers, the same bits, margins included
        assert torch.equal(out_buf.view(torch.int32), again[0].view(torch.int32)), label
        assert torch.equal(stats_buf.view(torch.int32), again[1].view(torch.int32)), label
        bufs[label] = (out_buf, stats_buf)
    for label in ('n128', '64x64'):
        assert torch.equal(bufs['default'][0].view(torch.int32), bufs[label][0].view(torch.int32)), f'out differs between the default and {label}'
        assert torch.equal(bufs['default'][1].view(torch.int32), bufs[label][1].view(torch.int32)), f'stats differ between the default and {label}'
