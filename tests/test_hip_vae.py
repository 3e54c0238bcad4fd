"""GPU: the AutoencoderKL decoder (diff_sampler_amd/vae_engine.py) and the kernels it added -- the fp16-activation 3x3 convolution on
4 x 64 patches for images wider than 64 pixels (csrc/conv3x3_f16wide.hip, kernel id 2575) and the 512-channel attention head.
Goldens come from the real reference classes (tools/gen_vae_golden.py); nothing here reads the reference tree."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
G = os.path.join(ROOT, 'tests', 'golden')

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


# n, h, w, cin, cout, forced nb, fp16 rows out, residual, column sums
WIDE_CASES = [
    (3, 128, 128, 128, 192, 0, True, True, True),       # 192-column tiles, store-from-accumulators epilogue with fp16 residual and column sums
    (1, 256, 256, 64, 128, 0, False, False, True),      # fp32 rows out: the staged epilogue, column sums
    (1, 512, 512, 64, 64, 0, True, False, False),       # 64-column tiles (four-deep weight ring)
    (1, 128, 128, 192, 320, 0, True, True, True),       # two column groups: 192 + 128
    (3, 8, 128, 64, 64, 0, False, True, False),         # H != W: two patch rows per image, fp32 rows with an fp16 residual
    (1, 128, 128, 64, 256, 1, True, False, True),       # forced 64-column tiles
]


@pytest.mark.parametrize('n,h,w,cin,cout,nb,out16,res,stats', WIDE_CASES)
def test_wide_conv_matches_fp64_sums_of_fp16_operands(n, h, w, cin, cout, nb, out16, res, stats):
    """The new kernel alone against the same arithmetic on the CPU (fp16 operands, fp64 sums): 2e-5 of the output scale for fp32 rows, one fp16
    ulp (1.5e-3) for fp16 rows -- the per-kernel bounds of DESIGN.md section 2 -- on every pixel, and separately on the pixels next to a patch
    border (rows 4k - 1 | 4k, columns 64k - 1 | 64k) and on the image border, where the halo comes from a neighbouring patch or is zero
    padding.  Column sums: against sums formed on the CPU from the stored output, 1e-5 (the bound of the epilogue-statistics tests)."""
    from diff_sampler_amd import _lib, ops
    lib = _lib.load()
    dev = 'cuda'
    g = torch.Generator().manual_seed(n * 7 + h + w + cin + cout)
    rows = n * h * w
    x = torch.randn(rows, cin, generator=g).to(torch.float16)
    wt = torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5
    bias = torch.randn(cout, generator=g)
    res16 = torch.randn(rows, cout, generator=g).to(torch.float16) if res else None
    y = F.conv2d(x.double().reshape(n, h, w, cin).permute(0, 3, 1, 2), wt.to(torch.float16).double(), padding=1)
    y = y.permute(0, 2, 3, 1).reshape(rows, cout) + bias.double()
    if res:
        y = y + res16.double()
    ref = y.float().to(torch.float16).float() if out16 else y.float()
    wp = ops.pack_conv_weight_f16(wt.to(dev))
    out = torch.full((rows, cout), float('nan'), dtype=torch.float16 if out16 else torch.float32, device=dev)
    st = torch.full((rows // 64 * 2 * cout,), float('nan'), device=dev) if stats else None
    xd, bd_ = x.to(dev), bias.to(dev)
    rd = res16.to(dev) if res else None
    a = _lib.ConvArgs(xd.data_ptr(), None, cin, 0, cin, 0, n, h, w, 9, wp.data_ptr(), cout, bd_.data_ptr(), None, 0, 1,
                      rd.data_ptr() if res else None, cout if res else 0, 1.0, 0, out.data_ptr(), cout)
    a.wgt_f16, a.in_f16, a.out_f16, a.res_f16 = 1, 1, int(out16), int(res)
    if stats:
        a.stats_out = st.data_ptr()
    a.tune.f16dma_nb = nb
    assert lib.ds_conv_kernel_id(C.byref(a)) == 2575
    rc = lib.ds_conv2d_nhwc(C.byref(a), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, lib.ds_error_string(rc)
    got = out.float().cpu()
    assert torch.isfinite(got).all()
    bound = 1.5e-3 if out16 else 2e-5
    err = (got.double() - ref.double()).abs().reshape(n, h, w, cout) / float(ref.abs().max())
    yy, xx = torch.arange(h), torch.arange(w)
    tile_edge = ((yy % 4 == 0) | (yy % 4 == 3))[:, None] | ((xx % 64 == 0) | (xx % 64 == 63))[None, :]
    img_edge = ((yy == 0) | (yy == h - 1))[:, None] | ((xx == 0) | (xx == w - 1))[None, :]
    figures = dict(all=float(err.max()), tile_border=float(err[:, tile_edge].max()), image_border=float(err[:, img_edge].max()))
    print('wide conv', (n, h, w, cin, cout, nb, out16, res, stats), figures, 'bound', bound)
    assert figures['all'] < bound and figures['tile_border'] < bound and figures['image_border'] < bound, figures
    if stats:
        s = st.cpu().reshape(-1, 2, cout)
        assert _rel(s[:, 0], got.reshape(-1, 64, cout).sum(1)) < 1e-5 and _rel(s[:, 1], (got * got).reshape(-1, 64, cout).sum(1)) < 1e-5


def test_wide_conv_rejects_what_it_does_not_cover():
    """Widths that are not powers of two and appended 1x1 slabs have no fp16-activation route above 64 pixels: DS_E_SHAPE, never another kernel."""
    from diff_sampler_amd import _lib
    lib = _lib.load()
    x = torch.zeros(192 * 192, 64, dtype=torch.float16, device='cuda')
    wgt = torch.zeros(128, 9 * 64 // 2, device='cuda')
    out = torch.zeros(192 * 192, 64, dtype=torch.float16, device='cuda')
    a = _lib.ConvArgs(x.data_ptr(), None, 64, 0, 64, 0, 1, 192, 192, 9, wgt.data_ptr(), 64, None, None, 0, 1, None, 0, 1.0, 0, out.data_ptr(), 64)
    a.wgt_f16, a.in_f16, a.out_f16 = 1, 1, 1
    assert lib.ds_conv_kernel_id(C.byref(a)) == -3 and lib.ds_conv2d_nhwc(C.byref(a), _lib.stream_ptr()) == -3


def test_attention_with_one_512_channel_head():
    """ds_attention at d = 512 (the decoder's mid-block AttnBlock: the channel-split block with its epilogue patches aliased onto the K tile)
    against softmax(q k^T * scale) v in fp64, ragged lengths included."""
    from diff_sampler_amd import ops, _lib
    assert _lib.load().ds_attention_supported(512)
    for bz, sq, skv in ((2, 200, 333), (1, 1024, 1024)):
        g = torch.Generator().manual_seed(sq)
        d = 512
        qkv = torch.randn(bz, sq, 3 * d, generator=g)
        kv = torch.randn(bz, skv, 2 * d, generator=g) * 1.5
        qd, kvd = qkv.cuda(), kv.cuda()
        out = torch.full((bz, sq, d), float('nan'), device='cuda')
        ops.attention(qd, kvd, kvd[:, :, d:], out, batch=bz, heads=1, sq=sq, skv=skv, d=d, ldq=3 * d, ldk=2 * d, ldv=2 * d, ldo=d,
                      q_bs=sq * 3 * d, k_bs=skv * 2 * d, v_bs=skv * 2 * d, o_bs=sq * d, scale=d ** -0.5)
        torch.cuda.synchronize()
        w = (torch.einsum('bqd,bkd->bqk', qkv[:, :, :d].double(), kv[:, :, :d].double()) * d ** -0.5).softmax(-1)
        ref = torch.einsum('bqk,bkd->bqd', w, kv[:, :, d:].double()).float()
        assert _rel(out.cpu(), ref) < 2e-5, (bz, sq, skv)


def _golden(name):
    z = np.load(os.path.join(G, name))
    return z, str(z['config']), int(z['seed'])


def _u8(img):
    from diff_sampler_amd import ops
    B, Cc, H, W = img.shape
    u8 = torch.empty(B, H, W, Cc, dtype=torch.uint8, device=img.device)
    ops.quantize_u8_nhwc(img.contiguous(), u8, B, Cc, H, W)
    return u8.cpu().numpy()


@pytest.mark.parametrize('gold', ['vae_tiny.npz', 'vae_sd15_16.npz', 'vae_sd15.npz'])
def test_decoder_fp32_matches_the_real_reference(gold):
    """Whole decoder, fp32 mode, against the real Decoder + post_quant_conv (golden): the per-evaluation bound 2e-4 of the output scale; the
    uint8 images differ from the golden's quantisation by at most one level anywhere."""
    from diff_sampler_amd.vae_engine import VAEDecoder
    z, name, seed = _golden(gold)
    dec = VAEDecoder.from_config(name, seed=seed)
    img = dec(torch.from_numpy(z['z']).cuda())
    torch.cuda.synchronize()
    got, u8 = img.cpu(), _u8(img)
    if 'rows' in z.files:
        rows = torch.from_numpy(z['rows'])
        got, u8 = got[:, :, rows, :], u8[:, z['rows']]
    r = _rel(got, z['out'])
    lv = int(np.abs(u8.astype(np.int16) - z['u8'].astype(np.int16)).max())
    print(gold, 'fp32 rel', r, 'u8 levels', lv)
    assert tuple(got.shape) == z['out'].shape and r < 2e-4 and lv <= 1


@pytest.mark.parametrize('gold', ['vae_tiny.npz', 'vae_sd15_16.npz', 'vae_sd15.npz'])
def test_decoder_fp16_stays_within_the_recorded_autocast_distance(gold):
    """Whole decoder, fp16 mode, against the fp32 golden.  Bound: the larger of the per-evaluation fp16 bound 5e-3 and TWICE the distance the
    golden records for the real reference with every convolution's weights, input and output rounded to fp16 (``f16_dist``; twice: the engine
    and that emulation round the same tensors but sum in another order) -- DESIGN.md section 2."""
    from diff_sampler_amd.vae_engine import VAEDecoder, KERNEL_ID_F16WIDE
    z, name, seed = _golden(gold)
    dec = VAEDecoder.from_config(name, seed=seed, use_fp16=True)
    img, plan = dec.raw(torch.from_numpy(z['z']).cuda())
    torch.cuda.synchronize()
    got = img.cpu()
    if 'rows' in z.files:
        got = got[:, :, torch.from_numpy(z['rows']), :]
    bound = max(5e-3, 2 * float(z['f16_dist']))
    r = _rel(got, z['out'])
    print(gold, 'fp16 rel', r, 'recorded f16_dist', float(z['f16_dist']), 'bound', bound)
    assert r < bound
    if dec.spec.img_resolution > 64 and dec.spec.ch % 64 == 0:
        assert KERNEL_ID_F16WIDE in plan.kernel_ids.values()


@pytest.mark.parametrize('fp16', [False, True])
def test_decoder_graph_replay_and_batch_invariance(fp16):
    """Eager == hipGraph replay bit for bit; with batch_invariant=True the B = 1 output equals the same row of a B = 3 decode bit for bit."""
    from diff_sampler_amd.vae_engine import VAEDecoder
    z, name, seed = _golden('vae_sd15_16.npz')
    g = torch.Generator().manual_seed(5)
    lat = torch.cat([torch.from_numpy(z['z']), torch.randn(1, 4, 16, 16, generator=g) * 0.7]).cuda()
    dec = VAEDecoder.from_config(name, seed=seed, use_fp16=fp16, batch_invariant=True)
    out, plan = dec.raw(lat)
    torch.cuda.synchronize()
    eager = out.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sp = C.c_void_p(side.cuda_stream)
        plan.run(sp)
        side.synchronize()
        plan.graph_capture(sp)
        plan.bufs['out'].zero_()
        plan.graph_launch(sp)
        side.synchronize()
    assert torch.equal(plan.bufs['out'], eager)
    for i in range(3):
        one = dec(lat[i:i + 1])
        torch.cuda.synchronize()
        assert torch.equal(one[0], eager[i]), i


def test_cli_decode_latents_writes_the_decoded_pngs(tmp_path):
    """`--dataset_name ms_coco --random_init True --decode_latents True --seeds 0-1`: two 512 x 512 PNGs, equal to VAEDecoder(sampler output)
    quantised in-process; without the flag the same run still writes the latents."""
    import PIL.Image
    from diff_sampler_amd import sample
    from diff_sampler_amd.vae_engine import VAEDecoder
    kw = dict(max_batch_size=2, seeds='0-1', solver='dpmpp', max_order=2, num_steps=3, predict_x0=False, lower_order_final=True,
              schedule_type='discrete', schedule_rho=1, guidance_type='cfg', guidance_rate=7.5, random_init=True)
    lat_dir, n = sample.run('ms_coco', outdir=str(tmp_path / 'lat'), **kw)
    png_dir, m = sample.run('ms_coco', outdir=str(tmp_path / 'png'), decode_latents=True, **kw)
    assert n == m == 2
    lat = np.stack([np.load(os.path.join(lat_dir, '000000', f'{s:06d}.npy')) for s in (0, 1)])
    want = _u8(VAEDecoder.from_config('sd15', seed=0)(torch.from_numpy(lat).cuda()))
    for s in (0, 1):
        png = np.asarray(PIL.Image.open(os.path.join(png_dir, '000000', f'{s:06d}.png')))
        assert png.shape == (512, 512, 3) and np.array_equal(png, want[s]), s
    assert not any(f.endswith('.npy') for _, _, fs in os.walk(png_dir) for f in fs)
