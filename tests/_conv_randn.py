"""The "randn comparison" of the 3x3 convolution kernels (DESIGN.md section 2 keeps this family at 2e-5 of the absmax): random inputs, an fp64
reference of the layer and its whole epilogue, the column sums the kernel writes for the consumer's GroupNorm and the statistics
ds_gn_finalize makes of them.  One builder, one argument builder, one checker and the case table of the Winograd F(2x2, 3x3) kernel
(csrc/conv3x3_wino.hip), shared by tests/test_hip_wino.py, tests/test_hip_upconv.py, tests/test_conv_randn_cpu.py and tools/wino_bits.py.

Tolerance: the per-kernel bound of tests/test_hip_kernels.py, 2e-5 of the reference absmax.  An all-fp32 CPU simulation of F(2x2, 3x3) (pad,
4x4 unfold, B^T d B, per-position channel sums, A^T m A) against an fp64 direct convolution measured 5.8e-7 ... 6.2e-7 at 256 / 512 input
channels (the direct fp32 form: 2.5e-7 ... 3.2e-7): the transforms have entries 0, +-1, +-1/2 only.  Column sums 1e-5, mean and rstd of
ds_gn_finalize rtol 1e-4 / atol 1e-5."""
import ctypes as C
import functools

import torch
import torch.nn.functional as F

TOL = 2e-5
SCALE = 0.7071
FULL = ('norm', 'bias', 'cbias', 'res', 'scale', 'silu')


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


def nhwc(x):      # [B,C,H,W] -> [B*H*W, C]
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).contiguous()


@functools.lru_cache(maxsize=None)
def make_layer(seed, B, H, c0, c1, cout, ec0, ec1, feats):
    """Inputs (NCHW, CPU) and the fp64 reference d['ref'] (NHWC rows) of one layer: conv3x3 of x0 | x1, optionally behind a fused
    normalisation ('norm'; 'noact': without its SiLU), plus the appended 1x1 projection of e0 | e1, then bias, per-image bias, residual,
    scale, SiLU.  Computed once per case and never written to."""
    g = torch.Generator().manual_seed(seed)
    cin = c0 + c1
    d = dict(x0=torch.randn(B, c0, H, H, generator=g), x1=torch.randn(B, c1, H, H, generator=g) if c1 else None,
             w=torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5)
    xin = torch.cat([t for t in (d['x0'], d['x1']) if t is not None], 1).double()
    if 'norm' in feats:          # planes {mu, A, B} per image; B != 0: an activated border pixel differs from a zero one
        d['coefs'] = torch.stack([torch.randn(B, cin, generator=g), 0.5 + torch.rand(B, cin, generator=g), 0.5 + torch.randn(B, cin, generator=g)], 1)
        mu, A_, B_ = (d['coefs'][:, i].double()[:, :, None, None] for i in range(3))
        xin = (xin - mu) * A_ + B_
        if 'noact' not in feats:
            xin = F.silu(xin)
    ref = F.conv2d(xin, d['w'].double(), padding=1)
    if ec0:
        d['e0'] = torch.randn(B, ec0, H, H, generator=g)
        d['e1'] = torch.randn(B, ec1, H, H, generator=g) if ec1 else None
        d['ws'] = torch.randn(cout, ec0 + ec1, 1, 1, generator=g) / (ec0 + ec1) ** 0.5
        ref = ref + F.conv2d(torch.cat([t for t in (d['e0'], d['e1']) if t is not None], 1).double(), d['ws'].double())
    if 'bias' in feats:
        d['bias'] = torch.randn(cout, generator=g)
        ref = ref + d['bias'].double()[None, :, None, None]
    if 'cbias' in feats:
        d['cb'] = torch.randn(B, cout, generator=g)
        ref = ref + d['cb'].double()[:, :, None, None]
    if 'res' in feats:
        d['res'] = torch.randn(B, cout, H, H, generator=g)
        ref = ref + d['res'].double()
    if 'scale' in feats:
        ref = ref * SCALE
    if 'silu' in feats:
        ref = F.silu(ref)
    d['ref'] = nhwc(ref)
    return d


def device_cus():
    """Compute units of device 0 (256 where there is no device: the case table is then only collected, never run)."""
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def tiles_per_workgroup(B, H, cout, cus):
    """(valid tiles of every sequence b, b + G, ..., padded indices) of a launch: grid_1d and decode_tile in Python."""
    mtiles, ntiles = B * H * H // 256, cout // 64
    swapped = mtiles < 8 and ntiles > mtiles
    total = (ntiles + 7) // 8 * 8 * mtiles if swapped else (mtiles + 7) // 8 * 8 * ntiles
    nwg = min(total, cus // 8 * 8)

    def valid(b):
        if swapped:
            g, r = divmod(b, 8 * mtiles)
            return g * 8 + (r & 7) < ntiles
        g, r = divmod(b, 8 * ntiles)
        return g * 8 + (r & 7) < mtiles
    counts = [sum(valid(b) for b in range(w, total, nwg)) for w in range(nwg)]
    return counts, total - sum(counts)


# what tiles_per_workgroup() must give for a case of the 'persist' group, at any compute-unit count: (max tiles of a workgroup, min)
PERSIST_TILES = {
    'one_slab_a_few_workgroups_run_two_tiles': (2, 1),
    'padded_grid_has_invalid_indices': (2, 1),
    'three_tiles_of_three_slabs': (3, 2),
    'two_sources_full_epilogue_second_tile_is_another_image': (2, 1),
    'two_skip_slabs_behind_three_k_slabs_two_tiles': (2, 1),
    'two_tiles_on_32_columns': (2, 1),
    'two_tiles_on_64_columns_four_halo_slots': (2, 1),
}


def wino_groups(cus):
    """group -> {name: (seed, B, H, c0, c1, cout, ec0, ec1, features)}: the smallest shapes at which the Winograd kernel can still go wrong.
    A K slab is 8 input channels, a skip slab 32 channels of the appended 1x1 projection; cout = 256 throughout (four N tiles)."""
    return {
        # The software pipeline of the K loop (weight DMA of slab s+1 and loads of slab s+2 between the MFMAs of slab s, branch-free halo
        # store of slab s+1, s+1 / s+2 clamped to the last slab): one, two and three slabs, the a0 | a1 boundary seen first by the store and
        # first by the s+2 load, two images adjacent in memory (the row above image 1 is zeros AFTER the activation, not image 0's last row;
        # the normalisation's B plane is != 0, so an activated zero differs from a zero), TH = 4, every instantiation of the normalisation
        # (none / affine / affine + SiLU), and the hand-over from the last K slab into one and into three appended 1x1 slabs.
        'pipe': {
            'one_slab': (7000, 1, 16, 8, 0, 256, 0, 0, ('norm',)),
            'two_slabs': (7001, 2, 16, 16, 0, 256, 0, 0, ('norm',)),
            'three_slabs_source_boundary_after_the_first': (7002, 2, 16, 8, 16, 256, 0, 0, ('norm',)),
            'source_boundary_first_seen_by_the_load_two_ahead': (7003, 1, 32, 16, 8, 256, 0, 0, ('norm',)),
            'four_tiles_per_image_two_adjacent_images': (7004, 2, 32, 24, 0, 256, 0, 0, ('norm',)),
            'four_rows_per_tile': (7005, 1, 64, 24, 0, 256, 0, 0, ('norm',)),
            'no_normalisation': (7006, 1, 16, 24, 0, 256, 0, 0, ()),
            'normalisation_without_activation': (7007, 1, 16, 24, 0, 256, 0, 0, ('norm', 'noact')),
            'one_slab_into_one_skip_slab': (7008, 1, 16, 8, 0, 256, 32, 0, ('bias',)),
            'three_skip_slabs_two_sources_full_epilogue': (7009, 2, 16, 24, 0, 256, 32, 64, ('bias', 'res', 'silu', 'scale', 'cbias')),
        },
        # The first kernel's cases, all of >= 4 slabs: one image per tile, four tiles per image (a top border, none, a bottom border), the
        # appended skip slabs, the 64-column geometry of FFHQ.  Seed: B * 1000 + H * 10 + c0 + c1 + cout + ec0.
        'base': {
            'one_image_per_tile_full_epilogue': (3448, 3, 16, 32, 0, 256, 0, 0, ('bias', 'cbias', 'scale', 'silu', 'res')),
            'four_tiles_per_image_two_sources_norm': (2672, 2, 32, 64, 32, 256, 0, 0, ('norm',)),
            'appended_skip_slabs': (2544, 2, 16, 64, 0, 256, 64, 32, ('bias',)),
            'ffhq64_geometry': (1928, 1, 64, 32, 0, 256, 0, 0, ()),
        },
        # The pipelined skip-slab loop (one barrier per slab on two pixel and two weight buffers; weight DMA of slab es+1, pixel store of
        # slab es+1 and pixel loads of slab es+2 between the MFMAs of slab es, es+1 / es+2 clamped to the last slab): the buffers' parity
        # and the look-ahead of two slabs.  Two skip slabs (each buffer used once), four with the e0 | e1 boundary after the first (first
        # seen by the load two ahead), five behind an even number of K slabs on two images adjacent in memory, two behind an odd (one,
        # three) and behind an even number of K slabs (the hand-over from the K loop, whose last slab leaves a redundant DMA and store
        # behind), and skip slabs on 32- and 64-column images (the pixel -> (patch pixel, tile) mapping of the store depends on the width).
        'pipe2': {
            'two_skip_slabs_behind_one_k_slab': (7100, 1, 16, 8, 0, 256, 64, 0, ('bias',)),
            'four_skip_slabs_source_boundary_after_the_first': (7101, 1, 16, 8, 0, 256, 32, 96, ('bias',)),
            'five_skip_slabs_behind_two_k_slabs_two_adjacent_images': (7102, 2, 16, 16, 0, 256, 96, 64, ('norm', 'bias', 'res', 'silu', 'scale', 'cbias')),
            'two_skip_slabs_behind_two_k_slabs': (7103, 1, 16, 16, 0, 256, 64, 0, ('bias',)),
            'two_skip_slabs_behind_three_k_slabs_two_sources': (7104, 1, 16, 24, 0, 256, 32, 32, ('norm', 'bias')),
            'skip_slabs_on_32_columns': (7105, 1, 32, 8, 0, 256, 64, 0, ('bias',)),
            'skip_slabs_on_64_columns_two_sources': (7106, 1, 64, 8, 0, 256, 32, 32, ('norm', 'bias')),
        },
        # The one-barrier K loop (Vs and Hs doubled like Us; between barrier s-1 and barrier s the MFMAs of slab s run on Vs / Us[s & 1]
        # while the transform of slab s+1 goes Hs[(s+1) & 1] -> Vs[(s+1) & 1], the halo of slab s+2 is stored into Hs[s & 1], the weights of
        # slab s+1 stream into Us[(s+1) & 1] and the halo and coefficients of slab s+3 are loaded; s+1 / s+2 / s+3 clamped to the last
        # slab): the buffers' parity, the look-ahead of three slabs and the hand-over to the skip loop and the epilogue.  One slab (every
        # look-ahead clamped to slab 0), two and three (each buffer used once; an odd count), four (the load three ahead reaches exactly
        # the last slab), five on two sources with the boundary after the second (first seen by the load three ahead), seven on two
        # sources and two images adjacent in memory with the full epilogue and statistics, the other two instantiations of the
        # normalisation (affine only, none), 32- and 64-column images (3 and 4 halo slots per thread; the width-dependent halo and tile
        # mapping in both Hs buffers), and skip slabs behind three and behind four K slabs (the hand-over from either buffer parity, with
        # the last slab's redundant transform and halo store behind it).
        'kloop': {
            'one_slab_every_look_ahead_clamped': (7200, 1, 16, 8, 0, 256, 0, 0, ('norm',)),
            'two_slabs_each_buffer_used_once': (7201, 1, 16, 16, 0, 256, 0, 0, ('norm',)),
            'three_slabs_odd_count': (7202, 1, 16, 24, 0, 256, 0, 0, ('norm',)),
            'four_slabs_load_three_ahead_reaches_the_last': (7203, 1, 16, 32, 0, 256, 0, 0, ('norm',)),
            'five_slabs_source_boundary_after_the_second': (7204, 1, 16, 16, 24, 256, 0, 0, ('norm',)),
            'seven_slabs_two_sources_two_adjacent_images_full_epilogue': (7205, 2, 16, 24, 32, 256, 0, 0, FULL),
            'three_slabs_normalisation_without_activation': (7206, 1, 16, 24, 0, 256, 0, 0, ('norm', 'noact')),
            'three_slabs_no_normalisation': (7207, 1, 16, 24, 0, 256, 0, 0, ()),
            'three_slabs_on_32_columns': (7208, 1, 32, 24, 0, 256, 0, 0, ('norm',)),
            'three_slabs_on_64_columns_two_sources': (7209, 1, 64, 16, 8, 256, 0, 0, ('norm',)),
            'two_skip_slabs_behind_three_k_slabs': (7210, 1, 16, 24, 0, 256, 64, 0, ('norm', 'bias')),
            'two_skip_slabs_two_sources_behind_four_k_slabs': (7211, 1, 16, 32, 0, 256, 32, 32, ('norm', 'bias')),
        },
        # Launches of MORE TILES THAN COMPUTE UNITS, sized for a persistent form of the kernel (at most one workgroup per compute unit,
        # workgroup b running the tiles b, b + G, ... of decode_tile's order).  That form was measured and is not the kernel
        # (profiles/wino_persist_ab.txt); its cases stay: a workgroup holds a whole compute unit's LDS (156 KB of 160), so the workgroups
        # of the second and third round start on the LDS another tile's workgroup left behind -- and the kernel writes the zeros of a
        # tile's out-of-image halo cells ONCE, in front of the K loop, into both Hs buffers, where an earlier tile of another image row may
        # have left in-image pixels.  One 16x16 image is one M tile and cout = 256 four N tiles, so n images are 4 n tiles, padded by
        # grid_1d to a multiple of 32; a 32x32 image is four M tiles, a 64x64 image sixteen.  The image counts follow the compute-unit
        # count and every case must give the PERSIST_TILES it is named after: tiles_per_workgroup() deals the indices b, b + G, ... (G =
        # the compute units, rounded down to a multiple of 8) -- with one workgroup per tile the number of workgroups that use a compute
        # unit's LDS in turn.  With four N tiles the padded indices all lie in the last group of 32, at the END of such a sequence.
        'persist': {
            'one_slab_a_few_workgroups_run_two_tiles': (7300, cus // 4 + 1, 16, 8, 0, 256, 0, 0, ('norm',)),
            'padded_grid_has_invalid_indices': (7301, cus // 4 + 2, 16, 8, 0, 256, 0, 0, ('norm',)),
            'three_tiles_of_three_slabs': (7302, cus // 2 + 1, 16, 24, 0, 256, 0, 0, ('norm',)),
            'two_sources_full_epilogue_second_tile_is_another_image': (7303, cus // 4 + 1, 16, 16, 8, 256, 0, 0, FULL),
            'two_skip_slabs_behind_three_k_slabs_two_tiles': (7304, cus // 4 + 1, 16, 24, 0, 256, 64, 0, ('norm', 'bias')),
            'two_tiles_on_32_columns': (7305, cus // 16 + 1, 32, 8, 0, 256, 0, 0, ('norm',)),
            'two_tiles_on_64_columns_four_halo_slots': (7306, cus // 64 + 1, 64, 8, 0, 256, 0, 0, ('norm',)),
        },
    }


WINO_GROUPS = wino_groups(device_cus())


def wino_args(case, dev, guard=4096):
    """(ConvArgs, out, stats, keep-alive) of a row of the case table, forced onto the 256 x 256 class (kernel id 2565) in the Winograd form.
    out and stats are the interiors of NaN-filled buffers (keep['out_buf'], keep['stats_buf']: `guard` floats on either side)."""
    from diff_sampler_amd import _lib, ops
    seed, B, H, c0, c1, cout, ec0, ec1, feats = case
    d = make_layer(*case)
    keep = {k: (nhwc(v).to(dev) if isinstance(v, torch.Tensor) and v.dim() == 4 and k not in ('w', 'ws') else v) for k, v in d.items()}
    keep['wp'] = ops.pack_conv_weight_wino(d['w'].to(dev), extra=d['ws'].to(dev)) if ec0 else ops.pack_conv_weight_wino(d['w'].to(dev))
    for k in ('bias', 'cb', 'coefs'):
        if k in d:
            keep[k] = d[k].to(dev).contiguous()
    n_out, n_st = B * H * H * cout, B * H * H // 64 * 2 * cout
    keep['out_buf'] = torch.full((n_out + 2 * guard,), float('nan'), device=dev)
    keep['stats_buf'] = torch.full((n_st + 2 * guard,), float('nan'), device=dev)
    out = keep['out_buf'][guard:guard + n_out].view(B * H * H, cout)
    stats = keep['stats_buf'][guard:guard + n_st]
    p = lambda k: keep[k].data_ptr() if keep.get(k) is not None else None
    norm_act = _lib.DS_ACT_SILU if 'norm' in feats and 'noact' not in feats else _lib.DS_ACT_NONE
    a = _lib.ConvArgs(p('x0'), p('x1'), c0, c1, c0, c1, B, H, H, 9, keep['wp'].data_ptr(), cout, p('bias'), p('cb'), cout if 'cb' in keep else 0,
                      B if 'cb' in keep else 1, p('res'), cout if 'res' in keep else 0, SCALE if 'scale' in feats else 1.0,
                      _lib.DS_ACT_SILU if 'silu' in feats else _lib.DS_ACT_NONE, out.data_ptr(), cout,
                      p('coefs'), norm_act, p('e0'), p('e1'), ec0, ec1, ec0, ec1)
    a.wino = 1
    a.stats_out = stats.data_ptr()
    a.tune.mode, a.tune.variant = 256, 6
    return a, out, stats, keep


def column_sum_errors(got, stats, B, hw, cout):
    """The kernel's per-64-row column sums and sums of squares against the output's own: an image's hw / 64 blocks are contiguous and add
    up to the image's sums."""
    st = stats.reshape(B, hw // 64, 2, cout).double()
    img = got.double().reshape(B, hw, cout)
    return rel(st[:, :, 0].sum(1), img.sum(1)), rel(st[:, :, 1].sum(1), (img ** 2).sum(1))


def compare(case_row, got, stats, out_buf, stats_buf):
    """CPU: a launch's output and statistics (the interiors of out_buf and stats_buf) against the case's fp64 reference.  Returns
    (error, per-image errors, column-sum error, column-square-sum error), all relative."""
    seed, B, H, c0, c1, cout = case_row[:6]
    want = make_layer(*case_row)['ref']
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(stats).all())
    err = rel(got.double(), want)
    assert err < TOL, f'{err:.3e}'
    # every image against its own reference: a tile that took another tile's image, coefficients or cbias row fails here by name
    per = ((got.double() - want).abs().reshape(B, -1).amax(1) / want.abs().max()).tolist()
    assert max(per) < TOL, f'image {per.index(max(per))}: {max(per):.3e}'
    e_s, e_q = column_sum_errors(got, stats, B, H * H, cout)
    assert e_s < 1e-5 and e_q < 1e-5, (e_s, e_q)
    for buf, n in ((out_buf, got.numel()), (stats_buf, stats.numel())):        # nothing outside the tensors is written
        guard = (buf.numel() - n) // 2
        assert guard > 0 and bool(torch.isnan(buf[:guard]).all()) and bool(torch.isnan(buf[guard + n:]).all())
    return err, per, e_s, e_q


def finalize_check(lib, stats, want, B, hw, cout):
    """GPU: ds_gn_finalize makes the consumer's GroupNorm statistics (32 groups) of the column sums `stats`; against the fp64 reference."""
    from diff_sampler_amd import _lib
    G_ = 32
    dev = stats.device
    mean, rstd = torch.empty(B * G_, device=dev), torch.empty(B * G_, device=dev)
    coefs = torch.empty(B * 3 * cout, device=dev)
    gamma, beta = torch.ones(cout, device=dev), torch.zeros(cout, device=dev)
    f = _lib.GnFinalizeArgs(stats.data_ptr(), None, cout, 0, B, hw, G_, 1e-5, gamma.data_ptr(), beta.data_ptr(), None, None, 0, 1,
                            mean.data_ptr(), rstd.data_ptr(), coefs.data_ptr())
    assert lib.ds_gn_finalize(C.byref(f), _lib.stream_ptr()) == 0
    torch.cuda.synchronize()
    r = want.reshape(B, hw, G_, cout // G_).permute(0, 2, 1, 3).reshape(B, G_, -1)
    assert torch.allclose(mean.cpu(), r.mean(-1).float().reshape(-1), rtol=1e-4, atol=1e-5)
    assert torch.allclose(rstd.cpu(), (1.0 / (r.var(-1, unbiased=False) + 1e-5).sqrt()).float().reshape(-1), rtol=1e-4, atol=1e-5)
