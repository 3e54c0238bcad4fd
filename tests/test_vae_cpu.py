"""CPU: the AutoencoderKL decoder's host side -- the restatement the GPU tests compare with (tests/_vae_ref.py) against the real
reference's goldens, the launch plans and their routing (built on the CPU: nothing runs), the checkpoint route and the CLI flag."""
import collections
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
G = os.path.join(ROOT, 'tests', 'golden')


@pytest.mark.parametrize('gold', ['vae_tiny.npz', 'vae_sd15_16.npz'])
def test_restatement_equals_the_real_decoder(gold):
    """tests/_vae_ref.py == the real Decoder + post_quant_conv (recorded by tools/gen_vae_golden.py) to fp32 rounding: 1e-5 of the output scale
    (some sixty fp32 layers whose sums another thread count may order differently; on the recording machine the difference is 0)."""
    import _vae_ref
    from diff_sampler_amd import vae_arch as va
    z = np.load(os.path.join(G, gold))
    spec = va.vae_decoder_spec(**va.NAMED_VAE_CONFIGS[str(z['config'])])
    out = _vae_ref.decode(spec, va.init_vae_params(spec, seed=int(z['seed'])), torch.from_numpy(z['z']))
    ref = torch.from_numpy(z['out'])
    assert out.shape == ref.shape
    assert float((out - ref).abs().max() / ref.abs().max()) < 1e-5
    u8 = _vae_ref.quantize_u8(out).numpy()
    assert int(np.abs(u8.astype(np.int16) - z['u8'].astype(np.int16)).max()) <= 1
    assert 0 < float(z['f16_dist']) < 5e-2


def test_goldens_are_small_data_files():
    biggest = max(os.path.getsize(os.path.join(G, f)) for f in os.listdir(G) if not f.startswith('vae_'))
    for f in ('vae_tiny.npz', 'vae_sd15_16.npz', 'vae_sd15.npz'):
        assert os.path.getsize(os.path.join(G, f)) <= min(biggest, 1 << 20), f


def test_spec_follows_v1_inference_yaml_and_refuses_everything_else():
    from diff_sampler_amd import vae_arch as va
    spec = va.vae_decoder_spec(**va.NAMED_VAE_CONFIGS['sd15'])
    assert spec.img_resolution == 512
    kinds = [l.kind for l in spec.layers]
    assert kinds.count('res') == 2 + 4 * 3 and kinds.count('up') == 3 and kinds.count('attn') == 1
    assert [(l.cin, l.cout, l.res_out) for l in spec.layers if l.kind == 'up'] == [(512, 512, 128), (512, 512, 256), (256, 256, 512)]
    assert [l.key for l in spec.layers if l.kind == 'res' and l.cin != l.cout] == ['decoder.up.1.block.0', 'decoder.up.0.block.0']
    # the issue's hand count: ~2.5 TFLOP per image, 91 % of it above 64 pixels
    fl = dict(va.vae_layer_flops(spec))
    total = va.vae_flops_per_image(spec)
    assert total == sum(fl.values()) == 2514518933504.0
    wide = sum(v for k, v in fl.items() if any(k.startswith(l.key) for l in spec.layers if l.res_out > 64 and l.kind != 'conv_out'))
    assert 0.89 < wide / total < 0.93
    for bad in (dict(attn_resolutions=(32,)), dict(tanh_out=True), dict(give_pre_end=True), dict(use_linear_attn=True), dict(first_stage='vq'),
                dict(attn_type='linear'), dict(resamp_with_conv=False)):
        with pytest.raises(NotImplementedError):
            va.vae_decoder_spec(**dict(va.NAMED_VAE_CONFIGS['sd15'], **bad))


@pytest.mark.parametrize('B', [1, 3, 16])
def test_fp16_plan_routes_every_wide_convolution_to_the_patch_kernel(B):
    """Host logic: the sd15 plans at B = 1, 3, 16.  Every 3x3 convolution wider than 64 pixels reports the new kernel id from
    ds_conv_kernel_id, no launch is refused, the launch count does not depend on the batch, and the FLOPs of the convolution launches add up
    to the spec's count."""
    from diff_sampler_amd import _lib, vae_arch as va
    from diff_sampler_amd.vae_engine import VAEDecoder, KERNEL_ID_F16WIDE
    lib = _lib.load()
    dec = VAEDecoder.from_config('sd15', seed=0, device='cpu', use_fp16=True)
    P = dec.plan(B)
    assert len(P.ops) == 101
    convs = [op for op in P.ops if op.fn is lib.ds_conv2d_nhwc]
    wide = [op for op in convs if op.keep[0].taps == 9 and op.keep[0].w > 64 and op.keep[0].cout > 4]
    assert len(wide) == 21
    for op in convs:
        a = op.keep[0]
        kid = lib.ds_conv_kernel_id(C.byref(a))
        assert kid >= 0 and kid == P.kernel_ids[op.name], (op.name, kid)
        if op in wide:
            assert a.in_f16 and kid == KERNEL_ID_F16WIDE, (op.name, kid)
            info = _lib.ConvRouteInfo()
            assert lib.ds_conv_route(C.byref(a), C.byref(info)) == 0
            widths = list(info.f16_widths)[:info.f16_groups]
            assert info.kernel_id == KERNEL_ID_F16WIDE and info.splits == 1
            assert widths == {128: [2], 256: [2], 512: [3, 2]}[a.cout], (op.name, widths)
        else:
            assert kid != KERNEL_ID_F16WIDE
    assert collections.Counter(P.kernel_ids.values()) == {2564: 2, 2566: 10, 2567: 3, 2575: 21, 2570: 1}
    assert P.kernel_ids['decoder.conv_out'] == 2570 and convs[-1].keep[0].out_nchw == 1          # norm_out + swish + conv_out: one thin-kernel launch
    # FLOPs: the spec's table, launch by launch (conv_in runs on the K-padded im2col GEMM and carries post_quant_conv: counted by the table only)
    table = dict(va.vae_layer_flops(dec.spec))
    for op in convs:
        a = op.keep[0]
        if op.name in table and op.name != 'decoder.conv_in':
            assert 2.0 * a.h * a.w * a.taps * a.c0 * a.cout == table[op.name], op.name
    assert dec.flops(B) == B * sum(table.values()) == B * va.vae_flops_per_image(dec.spec)
    # workspaces are recycled: far less than one tensor per layer (a full-resolution 128-channel fp16 tensor is 64 MiB per image)
    kept = sum(t.numel() * t.element_size() for t in P.keep) / 2 ** 20
    assert kept < 256 + 64 + 800 * B, kept


def test_fp32_plan_uses_existing_routes_only():
    from diff_sampler_amd.vae_engine import VAEDecoder, KERNEL_ID_F16WIDE
    dec = VAEDecoder.from_config('sd15', seed=0, device='cpu')
    for B in (1, 3, 16):
        P = dec.plan(B)
        assert len(P.ops) == 91 and min(P.kernel_ids.values()) >= 0 and KERNEL_ID_F16WIDE not in P.kernel_ids.values()
        assert P.kernel_ids['decoder.conv_out'] == 2570


def test_wide_kernel_is_reached_only_where_no_route_existed():
    """ds_conv_kernel_id: the patch kernel takes in_f16 3x3 layers wider than 64 pixels with power-of-two sides; narrower images keep
    conv3x3_f16dma's ids, other widths and appended 1x1 slabs stay DS_E_SHAPE."""
    from diff_sampler_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(64, dtype=torch.float32)

    def kid(h, w, cin=64, cout=64, ec0=0, norm=False):
        a = _lib.ConvArgs(buf.data_ptr(), None, cin, 0, cin, 0, 1, h, w, 9, buf.data_ptr(), cout, None, None, 0, 1, None, 0, 1.0, 0, buf.data_ptr(), cout)
        a.wgt_f16, a.in_f16, a.out_f16 = 1, 1, 1
        if ec0:
            a.e0, a.ec0, a.eld0 = buf.data_ptr(), ec0, ec0
        if norm:
            a.norm_coefs = buf.data_ptr()
        return lib.ds_conv_kernel_id(C.byref(a))
    assert [kid(s, s) for s in (8, 16, 32, 64)] == [2566] * 4
    assert [kid(s, s) for s in (128, 256, 512, 1024)] == [2575] * 4
    assert kid(4, 128) == 2575 and kid(2, 128) == -3
    assert kid(192, 192) == -3 and kid(128, 96) == -3
    assert kid(128, 128, cin=96) == -3 and kid(128, 128, cout=96) < 0
    assert kid(128, 128, ec0=64) == -3 and kid(128, 128, norm=True) == -3


def test_state_dict_round_trip_with_the_real_key_names():
    """A synthetic SD-1.5 state_dict (real key names and shapes: U-Net, first stage with its encoder, text encoder) splits into the U-Net's and
    the decoder's tensors; VAEDecoder.from_state_dict packs the same weights as the parameters it was made from."""
    from diff_sampler_amd import sample, vae_arch as va
    from diff_sampler_amd.vae_engine import VAEDecoder
    spec = va.vae_decoder_spec(**va.NAMED_VAE_CONFIGS['sd15_16'])
    params = va.init_vae_params(spec, seed=7)
    assert params['decoder.mid.attn_1.q.weight'].shape == (512, 512, 1, 1) and params['post_quant_conv.weight'].shape == (4, 4, 1, 1)
    assert params['decoder.up.1.block.0.nin_shortcut.weight'].shape == (256, 512, 1, 1) and 'decoder.up.0.upsample.conv.weight' not in params
    assert params['decoder.up.3.upsample.conv.weight'].shape == (512, 512, 3, 3) and params['decoder.norm_out.weight'].shape == (128,)
    sd = {'first_stage_model.' + k: v.half() for k, v in params.items()}
    sd.update({'first_stage_model.encoder.conv_in.weight': torch.zeros(128, 3, 3, 3), 'first_stage_model.quant_conv.weight': torch.zeros(8, 8, 1, 1),
               'model.diffusion_model.time_embed.0.weight': torch.ones(1280, 320), 'cond_stage_model.transformer.x': torch.zeros(1),
               'model_ema.decay': torch.zeros(())})
    unet, vae = sample.split_sd_checkpoint(sd)
    assert list(unet) == ['time_embed.0.weight'] and set(vae) == set(params) and all(v.dtype == torch.float32 for v in vae.values())
    a = VAEDecoder.from_state_dict(sd, 'sd15_16', device='cpu')
    b = VAEDecoder(spec, {k: v.half().float() for k, v in params.items()}, device='cpu')
    assert set(a.w) == set(b.w) and all(torch.equal(a.w[k], b.w[k]) for k in a.w if isinstance(a.w[k], torch.Tensor))
    del sd['first_stage_model.decoder.conv_out.bias']
    with pytest.raises(KeyError):
        VAEDecoder.from_state_dict(sd, 'sd15_16', device='cpu')
    sd['first_stage_model.decoder.conv_out.bias'] = torch.zeros(4)
    with pytest.raises(ValueError):
        VAEDecoder.from_state_dict(sd, 'sd15_16', device='cpu')


def test_conv_in_weight_composes_post_quant_conv_exactly():
    """The composed conv_in matrix over the im2col of [z | 1] (vae_engine._pack) reproduces conv_in(post_quant_conv(z / scale_factor)),
    zero padding included, in plain torch on the CPU."""
    import torch.nn.functional as F
    from diff_sampler_amd import vae_arch as va
    from diff_sampler_amd.vae_engine import VAEDecoder
    spec = va.vae_decoder_spec(**va.NAMED_VAE_CONFIGS['tiny_vae'])
    p = va.init_vae_params(spec, seed=3)
    dec = VAEDecoder(spec, p, device='cpu')
    z = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(1))
    want = F.conv2d(F.conv2d(z / spec.scale_factor, p['post_quant_conv.weight'], p['post_quant_conv.bias']), p['decoder.conv_in.weight'],
                    p['decoder.conv_in.bias'], padding=1)
    x5 = torch.cat([z, torch.ones(2, 1, 8, 8)], 1)
    col = F.unfold(x5, 3, padding=1).reshape(2, 5, 9, 64).permute(0, 3, 2, 1).reshape(2 * 64, 45)          # K = tap * 5 + c
    W = dec.w['decoder.conv_in.w']
    got = (col @ W[:128, :45].t() + p['decoder.conv_in.bias']).reshape(2, 64, 128).permute(0, 2, 1).reshape(2, 128, 8, 8)
    assert W.shape == (128, 64) and float(W[:, 45:].abs().max()) == 0
    assert float((got - want).abs().max() / want.abs().max()) < 1e-5


def test_cli_parses_decode_latents_and_the_stub_mode_writes_what_it_wrote(tmp_path):
    import PIL.Image
    from click.testing import CliRunner
    from diff_sampler_amd import sample
    outs = []
    for i, extra in enumerate(([], ['--decode_latents', 'true'])):
        out = tmp_path / f'o{i}'
        r = CliRunner().invoke(sample.main, ['--stub', 'true', '--dataset_name', 'cifar10', '--solver', 'ipndm', '--num_steps', '6', '--batch', '4',
                                             '--seeds', '0-5', '--outdir', str(out)] + extra)
        assert r.exit_code == 0, r.output
        files = sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)
        outs.append((files, [np.asarray(PIL.Image.open(out / f)).tobytes() for f in files]))
    assert outs[0] == outs[1] and len(outs[0][0]) == 6
    assert CliRunner().invoke(sample.main, ['--decode_latents', 'maybe']).exit_code != 0
