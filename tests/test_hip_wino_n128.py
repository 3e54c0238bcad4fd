"""GPU: the two tile shapes of the Winograd F(2x2, 3x3) convolution (csrc/conv3x3_wino.hip) against each other.  The 32-tile x 128-channel
workgroup (wino_n128_kernel, the default) keeps every chain of arithmetic of the 64-tile x 64-channel one (conv3x3_wino_kernel, reached
through bit 10 of ds_conv_tune.variant): slab order, K step order, the skip loop's order, the halo chain, the epilogue and the column-sum
shuffles.  So each case runs on both shapes and must give THE SAME BITS of the output and of the statistics, on top of the fp64 bound of
tests/_conv_randn.py, the GroupNorm statistics ds_gn_finalize makes of the column sums, NaN margins left alone and a second launch with the
same bits.

The cases are the smallest at which the new tile can go wrong (a K slab is 8 input channels, a skip slab 32 channels of the appended 1x1
projection; an M tile is 128 pixels of one image, an N tile 128 columns):
  one 16x16 image, one slab      two M tiles that split the image: an in-image halo row at the inner edge, an out-of-image row at the outer;
                                 every look-ahead of the K loop clamped to slab 0
  one 32x32 image, two slabs     eight M tiles, six of them interior (no vertical border); each buffer used once
  one 64x64 image                two rows per tile, three halo slots per thread
  three 16x16 images             neighbouring M tiles belong to different images: per-image cbias row and normalisation coefficients
  five slabs on two sources      the a0 | a1 switch between slabs 2 and 3, first seen by the load three ahead; affine without SiLU, residual,
                                 512 columns = four N tiles (a wave's weight run lies in the 64-column image 2 nt + (wave >> 1))
  three slabs, switch after the first, no normalisation
  one skip slab from e0; three skip slabs from e0 | e1 behind two K slabs with the full epilogue on 512 columns."""
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

OLD_TILE = 1024           # ds_conv_tune.variant bit 10: the 64-tile x 64-channel workgroups

# name: (seed, B, H, c0, c1, cout, ec0, ec1, features)
CASES = {
    'one_16x16_image_one_slab': (7400, 1, 16, 8, 0, 256, 0, 0, ('norm',)),
    'one_32x32_image_two_slabs_interior_tiles': (7401, 1, 32, 16, 0, 256, 0, 0, ('norm',)),
    'one_64x64_image_three_halo_slots': (7402, 1, 64, 8, 0, 256, 0, 0, ('norm',)),
    'three_images_cbias_and_coefficients_per_image': (7403, 3, 16, 24, 0, 256, 0, 0, ('norm', 'cbias')),
    'five_slabs_two_sources_affine_only_res_512_columns': (7404, 1, 16, 16, 24, 512, 0, 0, ('norm', 'noact', 'res')),
    'three_slabs_source_switch_after_the_first_no_normalisation': (7405, 1, 16, 8, 16, 256, 0, 0, ()),
    'one_skip_slab_from_e0': (7406, 1, 16, 8, 0, 256, 32, 0, ('bias',)),
    'three_skip_slabs_e0_e1_full_epilogue_512_columns': (7407, 2, 16, 16, 0, 512, 32, 64, R.FULL),
}


def _launch(lib, row, variant_bits):
    """Route assertion and one launch into fresh NaN-filled guarded buffers, on the tile shape `variant_bits` selects."""
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
def test_both_tile_shapes_give_the_same_bits_within_the_fp64_bound(name):
    from diff_sampler_amd import _lib
    row = CASES[name]
    seed, B, H, c0, c1, cout, ec0, ec1, feats = row
    lib = _lib.load()
    bufs = {}
    for label, bits in (('32x128', 0), ('64x64', OLD_TILE)):
        out, stats, out_buf, stats_buf = _launch(lib, row, bits)
        err, per, e_s, e_q = R.compare(row, out.cpu(), stats.cpu(), out_buf.cpu(), stats_buf.cpu())
        print(f'wino {label} {name} {row[1:8]}: {(c0 + c1) // 8} slabs + {(ec0 + ec1) // 32} skip slabs, rel err vs fp64 {err:.3e} '
              f'(worst image {per.index(max(per))}), column sums rel err {e_s:.3e} / {e_q:.3e}')
        R.finalize_check(lib, stats, R.make_layer(*row)['ref'], B, H * H, cout)
        again = _launch(lib, row, bits)[2:]              # launch independence: fresh buffers, the same bits, margins included
        assert torch.equal(out_buf.view(torch.int32), again[0].view(torch.int32)), label
        assert torch.equal(stats_buf.view(torch.int32), again[1].view(torch.int32)), label
        bufs[label] = (out_buf, stats_buf)
    assert torch.equal(bufs['32x128'][0].view(torch.int32), bufs['64x64'][0].view(torch.int32)), 'out differs between the tile shapes'
    assert torch.equal(bufs['32x128'][1].view(torch.int32), bufs['64x64'][1].view(torch.int32)), 'stats differ between the tile shapes'
