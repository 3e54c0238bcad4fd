"""CPU-only: the fp16x3 mode of the CLIP score (dsm_gemm_split, ops.pack_linear_weight_split, ``dtype='fp16x3'`` of the towers).

The packing reconstructs the scaled weights and has the kernel's layout; both towers' plans build without a GPU with the four projections of
every layer on dsm_gemm_split, no GELU launch, and an fp32 plan that the argument leaves alone; the entry point rejects bad arguments on the
host and agrees with dsm_gemm_split_supported; gemm_split.hip compiles for gfx950 without scratch."""
import ctypes as C
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diff_sampler_amd import clip_score_arch as A  # noqa: E402


@pytest.fixture(scope='module')
def libs():
    from diff_sampler_amd import build, _lib, _metrics_lib
    build.build_metrics_lib(verbose=False)
    return _lib.load(), _metrics_lib.load()


# ------------------------------------------------------------------------------------------------------------------ packing
def _halves(packed):
    return packed.view(torch.float16)


@pytest.mark.parametrize('cout,k,scale', [(96, 64, 0.03), (352, 352, 0.03), (130, 32, 40.0), (32, 96, 3e-6)])
def test_packing_reconstructs_the_scaled_weights(cout, k, scale):
    from diff_sampler_amd.ops import pack_linear_weight_split
    g = torch.Generator().manual_seed(cout + k)
    w = torch.randn(cout, k, generator=g) * scale
    w[0, 0] = 0.0
    packed, shift = pack_linear_weight_split(w)
    rows = -(-cout // 128) * 128
    assert packed.dtype == torch.float32 and tuple(packed.shape) == (rows, k)                # a float-typed view of [rows][2 k] halves
    h = _halves(packed)
    assert tuple(h.shape) == (rows, 2 * k) and float(h[cout:].abs().max() if rows > cout else 0.0) == 0.0       # rows padded to 128 with zeros
    wmax = float(w.abs().max())
    assert 0 <= shift <= 24 and (2.0 ** 13 <= wmax * 2.0 ** shift < 2.0 ** 14 or shift in (0, 24))
    blocks = h[:cout].reshape(cout, k // 32, 64)
    hi, lo = blocks[:, :, :32].reshape(cout, k), blocks[:, :, 32:].reshape(cout, k)           # [hi | lo] per 32-column block
    ws = w.double() * 2.0 ** shift
    assert torch.equal(hi, ws.float().to(torch.float16))                                      # hi = fp16(w 2^shift)
    assert torch.equal(lo, (ws.float() - hi.float()).to(torch.float16))
    err = (hi.double() + lo.double() - ws).abs()
    normal = lo.float().abs() >= 2.0 ** -14                                                   # lo is a normal fp16 number
    assert bool(normal.any()) and bool((err[normal] <= 2.0 ** -22 * ws.abs()[normal]).all())
    assert bool((err <= 2.0 ** -25).logical_or(normal).all())                                 # elsewhere: half a subnormal quantum


def test_packing_edge_cases():
    from diff_sampler_amd.ops import pack_linear_weight_split
    packed, shift = pack_linear_weight_split(torch.zeros(32, 32))
    assert shift == 0 and tuple(packed.shape) == (128, 32) and float(packed.abs().max()) == 0.0
    packed, shift = pack_linear_weight_split(torch.full((32, 32), 3.0e4))                     # inside the fp16 range with shift 0
    assert shift == 0 and float(_halves(packed)[0, 0]) == float(torch.tensor(3.0e4).to(torch.float16))
    for bad in (65504.0, 1e6, float('inf'), float('nan')):
        w = torch.zeros(32, 32)
        w[3, 5] = -bad
        with pytest.raises(ValueError):
            pack_linear_weight_split(w)
    with pytest.raises(ValueError):
        pack_linear_weight_split(torch.zeros(32, 48))                                         # K is not a multiple of 32
    packed, _ = pack_linear_weight_split(torch.ones(32, 32), row_pad=256)
    assert tuple(packed.shape) == (256, 32)


# ------------------------------------------------------------------------------------------------------------------ plans
PROJ = ('qkv', 'out_proj', 'fc1', 'fc2')


@pytest.mark.parametrize('name', ['tiny_clip_score', 'vit_g_14_2l'])
def test_plans_build_on_the_cpu_with_the_projections_on_the_split_gemm(libs, name):
    from diff_sampler_amd.clip_score_engine import ClipImageEncoder, ClipPooledTextEncoder
    from diff_sampler_amd._metrics_lib import DSM_ACT_GELU, DSM_ACT_NONE
    lib, mlib = libs
    spec = A.named_spec(name)
    p = A.init_clip_score_params(spec, 0)
    for cls, t, tag in ((ClipImageEncoder, spec.vision, 'vision'), (ClipPooledTextEncoder, spec.text, 'text')):
        plain = cls(spec, p, device='cpu').plan(2)
        fp32 = cls(spec, p, device='cpu', dtype='fp32').plan(2)
        split = cls(spec, p, device='cpu', dtype='fp16x3').plan(2)
        # the default plan is untouched by the argument: same names, same functions
        assert [(o.name, o.fn) for o in plain.ops] == [(o.name, o.fn) for o in fp32.ops]
        assert any(o.name.endswith('.gelu') for o in plain.ops)
        names = [o.name for o in split.ops]
        assert not [n for n in names if n.endswith('.gelu') or n.endswith('.quick_gelu')]                   # fc1 carries it
        assert len(names) == len(plain.ops) - t.layers
        assert [n for n in names] == [o.name for o in plain.ops if not o.name.endswith('.gelu')]
        by = {o.name: o for o in split.ops}
        for i in range(t.layers):
            for x in PROJ:
                assert by[f'{tag}.layers.{i}.{x}'].fn is mlib.dsm_gemm_split, (i, x)
            a = {x: by[f'{tag}.layers.{i}.{x}'].keep[0] for x in PROJ}
            assert a['fc1'].act == DSM_ACT_GELU and not a['fc1'].res and a['qkv'].act == DSM_ACT_NONE and not a['qkv'].res
            assert a['out_proj'].res and a['fc2'].res and a['out_proj'].act == a['fc2'].act == DSM_ACT_NONE
            assert (a['qkv'].k, a['qkv'].cout, a['fc1'].cout, a['fc2'].k, a['fc2'].cout) == (t.width, 3 * t.width, t.ffn, t.ffn, t.width)
            assert all(v.bias and v.rows == plain.bufs['hidden'].shape[0] and list(v.reserved) == [0, 0, 0] for v in a.values())
        # everything else stays where the fp32 plan has it
        for o, q in zip(split.ops, [o for o in plain.ops if not o.name.endswith('.gelu')]):
            if o.name.split('.')[-1] not in PROJ:
                assert o.fn is q.fn, o.name
        head = 'visual_projection' if tag == 'vision' else 'text_projection'
        assert by[head].fn is lib.ds_conv2d_nhwc
        if tag == 'vision':
            assert by['patch_embedding'].fn is lib.ds_conv2d_nhwc
        assert tuple(split.bufs['out'].shape) == (2, spec.embed) and split.bufs['hidden'].shape == plain.bufs['hidden'].shape


def test_quick_gelu_rides_in_fc1_and_bad_arguments_are_refused(libs):
    from diff_sampler_amd.clip_score_engine import ClipImageEncoder, ClipPooledTextEncoder
    from diff_sampler_amd.clip_score import ClipScorer
    from diff_sampler_amd._metrics_lib import DSM_ACT_QUICK_GELU
    _, mlib = libs
    cfg = dict(A.NAMED_CLIP_SCORE_CONFIGS['tiny_clip_score'], act='quick_gelu')
    spec = A.clip_score_spec(**cfg)
    p = A.init_clip_score_params(spec, 0)
    P = ClipPooledTextEncoder(spec, p, device='cpu', dtype='fp16x3').plan(1)
    by = {o.name: o for o in P.ops}
    assert by['text.layers.0.fc1'].fn is mlib.dsm_gemm_split and by['text.layers.0.fc1'].keep[0].act == DSM_ACT_QUICK_GELU
    assert not [o for o in P.ops if 'gelu' in o.name]
    with pytest.raises(ValueError):
        ClipImageEncoder(spec, p, device='cpu', dtype='fp16')
    sc = ClipScorer(spec, p, device='cpu', dtype='fp16x3')
    assert sc.dtype == 'fp16x3' and sc.image.dtype == sc.text.dtype == 'fp16x3' and ClipScorer(spec, p, device='cpu').image.dtype == 'fp32'
    assert ClipScorer.from_config('tiny_clip_score', device='cpu', dtype='fp16x3').text.split


def test_geometry_the_split_gemm_refuses_is_an_error_at_build_time(libs):
    """ffn 520 is a multiple of 4 (enough for the fp32 kernels' row operations) but not of 32: fp16x3 refuses it, never falls back."""
    from diff_sampler_amd.clip_score_engine import _Tower
    import types
    _, mlib = libs
    t = types.SimpleNamespace(width=352, ffn=520)
    fake = types.SimpleNamespace(split=True, mlib=mlib)
    with pytest.raises(NotImplementedError, match='fp16x3'):
        _Tower._split_ok(fake, t, 'image')
    _Tower._split_ok(types.SimpleNamespace(split=False, mlib=mlib), t, 'image')               # fp32: not asked
    _Tower._split_ok(fake, types.SimpleNamespace(width=352, ffn=1536), 'image')


def test_cli_has_the_dtype_switch():
    from click.testing import CliRunner
    from diff_sampler_amd import clip_score as CS
    r = CliRunner().invoke(CS.main, ['calc', '--help'])
    assert r.exit_code == 0 and '--dtype' in r.output and 'fp16x3' in r.output
    opt = [o for o in CS.calc.params if o.name == 'dtype'][0]
    assert opt.default == 'fp32' and list(opt.type.choices) == ['fp32', 'fp16x3']


# ------------------------------------------------------------------------------------------------------------------ library surface
def test_gemm_split_rejects_bad_arguments_on_the_host(libs):
    """Every rejection comes back before any launch: no GPU is needed for them."""
    from diff_sampler_amd._metrics_lib import DS_E_ALIGN, DS_E_ARG, DS_E_SHAPE, DsmGemmSplitArgs, DSM_VERSION
    _, m = libs
    assert m.dsm_version() == DSM_VERSION == 2
    buf = (C.c_float * 8192)()
    base = (C.addressof(buf) + 63) & ~63
    other = base + 4096

    def call(**kw):
        a = dict(x=base, ldx=64, rows=5, k=64, w_split=base, shift=3, cout=96, bias=base, res=None, res_ld=0, act=0, out=other, out_ld=96)
        reserved = kw.pop('reserved', (0, 0, 0))
        a.update(kw)
        s = DsmGemmSplitArgs(**a)
        s.reserved[:] = reserved
        return m.dsm_gemm_split(C.byref(s), None)

    assert m.dsm_gemm_split(None, None) == DS_E_ARG
    assert call(x=None) == call(w_split=None) == call(out=None) == DS_E_ARG                   # NULL pointers (bias and res may be NULL)
    assert call(ldx=60) == call(out_ld=92) == call(res=base, res_ld=92) == DS_E_ARG           # a leading dimension below its columns
    assert call(res=other, res_ld=96) == DS_E_ARG                                             # res == out
    assert call(res=base, res_ld=96, act=1) == DS_E_ARG                                       # an activation and a residual exclude each other
    assert call(act=3) == call(act=-1) == DS_E_ARG                                            # unknown activation
    assert call(reserved=(1, 0, 0)) == call(reserved=(0, 0, 7)) == DS_E_ARG
    assert call(shift=-1) == call(shift=127) == DS_E_ARG
    assert call(x=base + 4) == call(out=other + 8) == call(w_split=base + 2) == call(bias=base + 4) == call(res=base + 4, res_ld=96) == DS_E_ALIGN
    assert call(ldx=66) == call(out_ld=98) == call(res=base, res_ld=98) == DS_E_ALIGN         # leading dimensions: multiples of 4
    for rows, k, cout in ((5, 48, 96), (5, 64, 40), (0, 64, 96), (-1, 64, 96), (5, 0, 96), (5, 64, 0), (5, 16, 96), (5, 64, 16), (5, 1416, 96)):
        assert call(rows=rows, k=k, cout=cout, ldx=max(k, 4) + 4 - max(k, 4) % 4, out_ld=max(cout, 4) + 4 - max(cout, 4) % 4) == DS_E_SHAPE, (rows, k, cout)
        assert m.dsm_gemm_split_supported(rows, k, cout) == 0
    for rows, k, cout in ((1, 32, 32), (77, 352, 352), (257, 1408, 1056), (16448, 1408, 4224), (1 << 33, 6144, 1408)):
        assert m.dsm_gemm_split_supported(rows, k, cout) == 1
    assert m.dsm_gemm_split_supported(1 << 41, 32, 32) == 0                                   # more workgroups than a grid holds


def test_gemm_split_kernel_needs_no_scratch():
    """64 accumulator registers, 16 of staged operands and 32 of fragments per lane: no private memory in any of the three activations'
    instantiations, and registers for the two workgroups per CU that 64 KB of LDS each leave room for (512 / 2 = 256)."""
    import shutil
    import subprocess
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    src = os.path.join(ROOT, 'diff_sampler_amd', 'csrc', 'metrics', 'gemm_split.hip')
    r = subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-c', src, '-o', os.devnull, '-Rpass-analysis=kernel-resource-usage'],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    found = re.findall(r'Function Name: (\S*gemm_split_kernel\S*).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)',
                       r.stderr, flags=re.S)
    assert len(found) == 3, r.stderr[-1500:]
    for name, vgpr, agpr, scratch, occ in found:
        print(f'{name}: VGPRs {vgpr}, AGPRs {agpr}, scratch {scratch}, occupancy {occ} waves/SIMD')
        assert int(scratch) == 0 and int(vgpr) + int(agpr) <= 256 and int(occ) >= 2
