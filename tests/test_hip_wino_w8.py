"""GPU: the three kernels of the Winograd F(2x2, 3x3) convolution (csrc/conv3x3_wino.hip) against each other.  wino_w8_kernel (the default
at 16 and 32 columns) covers wino_n128_kernel's 32-tile x 128-channel workgroup with EIGHT waves, two per SIMD: a wave owns 32 channels
and half of the 16 positions of the transformed patch, the pair exchanges four accumulators through the LDS behind the K loop, and each
wave then owns one patch row -- its skip slabs, its epilogue and its 64-pixel statistics block.  It keeps every chain of arithmetic of
wino_n128_kernel (ds_conv_tune.variant bit 15) and of the 64-tile x 64-channel conv3x3_wino_kernel (bit 10).  So each case runs on the
default route, on bit 15 and on bit 10 and must give THE SAME BITS of the output and of the statistics, on top of the fp64 bound of
tests/_conv_randn.py, the GroupNorm statistics ds_gn_finalize makes of the column sums, NaN margins left alone and a second launch with
the same bits.

The cases are the smallest at which the eight-wave kernel can go wrong (a K slab is 8 input channels, a skip slab 32 channels of the
appended 1x1 projection; an M tile is 128 pixels of one image, an N tile 128 columns):
  one 16x16 image, one slab      both M tiles at an image edge; every look-ahead of the K loop clamped to slab 0
  one 32x32 image, two slabs     interior tiles (no vertical border); each buffer used once
  one 64x64 image                the width at which the default stays wino_n128_kernel (the eight-wave kernel gains nothing there and has
                                 no instantiation with the second halo slot 64 columns need).  The default and bit 15 take the SAME kernel
                                 here, so their comparison says nothing about wino_w8_kernel: the case checks that the route by width
                                 sends a width the eight-wave kernel cannot stage (NP x 2 = 528 > 512 halo slots) to a kernel that can --
                                 a default launch of wino_w8_kernel there would leave 16 halo cells unwritten and miss the fp64 bound
  three 16x16 images             neighbouring M tiles belong to different images: per-image cbias row and normalisation coefficients
  five slabs on two sources      the a0 | a1 switch between slabs 2 and 3, first seen by the load three ahead; affine without SiLU, residual,
                                 512 columns = four N tiles, so each pair's weight run (image 2 nt + (channel group >> 1))
  three slabs, switch after the first, no normalisation
  one skip slab from e0 with bias
  three skip slabs e0 | e1       skip slabs on two pixel accumulators per wave, the full epilogue on both waves of a pair
  residual + cbias + SiLU with statistics on one image, cout = 256: the exchange and both patch rows' statistics blocks."""
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

# ds_conv_tune.variant: bit 15 = wino_n128_kernel (four waves on the same tile), bit 10 = the 64-tile x 64-channel workgroups.  The first
# entry is the default route: wino_w8_kernel at 16 and 32 columns, wino_n128_kernel at every other width (there bit 15 changes nothing)
SHAPES = (('default', 0), ('n128', 32768), ('64x64', 1024))


def default_kernel(H):
    """What launch_conv3x3_wino takes by default at image width H (the cases are square)."""
    return 'wino_w8_kernel' if H in (16, 32) else 'wino_n128_kernel'


# name: (seed, B, H, c0, c1, cout, ec0, ec1, features)
CASES = {
    'one_16x16_image_one_slab': (7500, 1, 16, 8, 0, 256, 0, 0, ('norm',)),
    'one_32x32_image_two_slabs_interior_tiles': (7501, 1, 32, 16, 0, 256, 0, 0, ('norm',)),
    'one_64x64_image_default_stays_the_four_wave_kernel': (7502, 1, 64, 8, 0, 256, 0, 0, ('norm',)),
    'three_images_cbias_and_coefficients_per_image': (7503, 3, 16, 24, 0, 256, 0, 0, ('norm', 'cbias')),
    'five_slabs_two_sources_affine_only_res_512_columns': (7504, 1, 16, 16, 24, 512, 0, 0, ('norm', 'noact', 'res')),
    'three_slabs_source_switch_after_the_first_no_normalisation': (7505, 1, 16, 8, 16, 256, 0, 0, ()),
    'one_skip_slab_from_e0_with_bias': (7506, 1, 16, 8, 0, 256, 32, 0, ('bias',)),
    'three_skip_slabs_e0_e1_full_epilogue_512_columns': (7507, 2, 16, 16, 0, 512, 32, 64, R.FULL),
    'res_cbias_silu_and_statistics_one_image': (7508, 1, 16, 16, 0, 256, 0, 0, ('norm', 'res', 'cbias', 'silu')),
}


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
        kernel = default_kernel(H) if label == 'default' else {'n128': 'wino_n128_kernel', '64x64': 'conv3x3_wino_kernel'}[label]
        print(f'wino {label} ({kernel}) {name} {row[1:8]}: {(c0 + c1) // 8} slabs + {(ec0 + ec1) // 32} skip slabs, rel err vs fp64 {err:.3e} '
              f'(worst image {per.index(max(per))}), column sums rel err {e_s:.3e} / {e_q:.3e}')
        R.finalize_check(lib, stats, R.make_layer(*row)['ref'], B, H * H, cout)
        again = _launch(lib, row, bits)[2:]              # launch independence: fresh buffers, the same bits, margins included
        assert torch.equal(out_buf.view(torch.int32), again[0].view(torch.int32)), label
        assert torch.equal(stats_buf.view(torch.int32), again[1].view(torch.int32)), label
        bufs[label] = (out_buf, stats_buf)
    for label in ('n128', '64x64'):
        assert torch.equal(bufs['default'][0].view(torch.int32), bufs[label][0].view(torch.int32)), f'out differs between the default and {label}'
        assert torch.equal(bufs['default'][1].view(torch.int32), bufs[label][1].view(torch.int32)), f'stats differ between the default and {label}'
