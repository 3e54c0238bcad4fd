"""Case table of the U-Net block forms of the wide fp16-activation 3x3 kernel (csrc/conv3x3_f16wide.hip): appended 1x1 columns (kernel id
2576) and the per-image bias row (2575 / 2576), on the families, the data and the argument builder of tests/_conv_refs.py (imported, not
edited).  tests/test_cm_wide_cases_cpu.py proves routes and exactness conditions, tests/test_hip_cm_wide_conv.py runs the cases.

What the table covers: W = 128 with H in {4, 8} (one and two patch rows); one and two images (image borders inside a launch, the cbias row
index); c0 in {64, 128} (c0 = 64: the appended slab is slab 1, staged whole in the prologue); ec0 in {0, 64, 128}; cout in {64, 128, 192}, one
per column-tile width; fp16 and fp32 rows out; with and without residual (fp32 and fp16); statistics at the small magnitudes family A
prescribes for them; the real geometry once (256 x 256, 64 + 64 -> 64); the family-B selector form for the real-valued epilogue."""
import _conv_refs as R

_c = R._c
F16 = dict(kind='f16')
X16 = dict(kind='f16', tune=dict(variant=131072))       # appended slabs above 64 pixels are asked for: ds_conv_tune.variant bit 17

CASES = (
    # ---- appended 1x1 columns (2576)
    _c('cmw_e64', 1, 4, 128, 64, 64, ec0=64, kid=2576, widths=(1,), **X16),
    _c('cmw_e128_cbn_res', 2, 8, 128, 128, 128, ec0=128, cbias=2, res=1, kid=2576, widths=(2,), fam='AB', **X16),
    _c('cmw_e64_192_out16', 2, 4, 128, 64, 192, ec0=64, cbias=2, res=1, res16=1, scale=2.0 ** -8, out16=1, bias=0, kid=2576, widths=(3,), fam='AB', **X16),
    _c('cmw_e128_c64_192', 1, 8, 128, 64, 192, ec0=128, res=1, kid=2576, widths=(3,), **X16),
    _c('cmw_e64_c128_out16', 2, 8, 128, 128, 64, ec0=64, scale=2.0 ** -8, out16=1, kid=2576, widths=(1,), **X16),
    _c('cmw_e64_stats16', 2, 4, 128, 128, 128, ec0=64, stats=1, out16=1, mag='small', kid=2576, widths=(2,), **X16),
    _c('cmw_e64_stats32', 2, 4, 128, 64, 192, ec0=64, stats=1, res=1, mag='small', kid=2576, widths=(3,), **X16),
    _c('cmw_e64_b', 2, 4, 128, 64, 128, ec0=64, cbias=1, res=1, res16=1, scale=R.B_SCALE, act=1, out16=1, kid=2576, widths=(2,), fam='B', **X16),
    _c('cmw_256', 1, 256, 256, 64, 64, ec0=64, cbias=1, kid=2576, widths=(1,), **X16),
    # ---- the per-image bias row without appended columns (2575): conv0 of a non-adaptive block
    _c('cmw_cbn_out16', 2, 8, 128, 128, 128, cbias=2, scale=2.0 ** -8, out16=1, kid=2575, widths=(2,), fam='AB', **F16),
    _c('cmw_cb1', 2, 4, 128, 64, 64, cbias=1, kid=2575, widths=(1,), **F16),
    _c('cmw_cbn_stats16', 2, 4, 128, 64, 192, cbias=2, stats=1, out16=1, mag='small', kid=2575, widths=(3,), **F16),
)
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
RUNS = tuple((c.name, fam) for c in CASES for fam in c.fam)
