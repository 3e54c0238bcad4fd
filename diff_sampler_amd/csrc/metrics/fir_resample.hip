// FIR resampling of the NCSN++ networks (networks_edm.py:56-82, Conv2d.forward with resample_filter = [1,3,3,1]) on fp32 NHWC rows.
//
//   dsm_fir_resample   the depthwise forms of Conv2d.forward for a separable 4-tap filter f (passed as its 1-D taps), one launch with the epilogue
//                      out = (fir + bias[c] + res[m, c]) * out_scale:
//                        down:  out[y, x] = sum_{i, j < 4} f2d[i][j] in[2y + i - pad, 2x + j - pad],  f2d = f (x) f / (sum f)^2, zero outside the
//                               image and NOT renormalised at the border (conv2d's zero padding); pad = 1 is the stand-alone form, pad = 0 the
//                               second half of fused_resample on the (h + 2) x (w + 2) output of the padding-2 convolution.  16 taps per output.
//                        up:    conv_transpose2d with 4 f2d, stride 2, padding 1 (h x w -> 2h x 2w): output row Y receives input rows y with
//                               Y = 2y + i - 1, i.e. two taps per axis -- for [1,3,3,1] the 3/4 | 1/4 phase form.  4 taps per output.
//                      The 2-D weights are formed on the host with the reference's own fp32 expression (f.ger(f) / f.sum().square(), times 4 for up;
//                      exact for [1,1] and [1,3,3,1]) and travel in the kernel arguments.  The sum runs over the taps in a fixed order (i outer, j
//                      inner, taps outside the image skipped) in fp32 FMAs: at most one rounding per tap, three for the epilogue.
//   dsm_zero_border    [outer][h][w][inner] -> [outer][h + 2p][w + 2p][inner] with a ring of zeros: conv2d(x, w, padding = 2) of the fused down
//                      path is the engine's padding-1 3x3 convolution on the zero-ringed input.
//
// Both are memory-bound: a lane moves whole channel quads (16-byte loads and stores; dsm_zero_border falls back to single floats when `inner` is
// not a multiple of 4 -- the channel-planar network input), consecutive lanes consecutive quads of a pixel, the grid is capped at 2048 workgroups
// with a grid-stride loop.  No LDS, no atomics, no scratch: an output element is written once, by one lane.
#include "../ds_common.h"
#include "ds_metrics.h"

namespace {

constexpr int FIR_MAX_BLOCKS = 2048;

struct FirParams {
    const float* x; const float* bias; const float* res; float* out;
    long long total;            // n * ho * wo * (c / 4)
    int ld_x, res_ld, out_ld;
    int h, w, ho, wo, c4, pad;
    float out_scale;
    float w2d[16];              // down: f2d[i][j]; up: 4 f2d[i][j]
};

template <bool UP>
__global__ void __launch_bounds__(256) fir_resample_kernel(const FirParams p) {
    const long long step = (long long)gridDim.x * 256;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < p.total; idx += step) {
        const int q = (int)(idx % p.c4);
        const long long pix = idx / p.c4;
        const int ox = (int)(pix % p.wo);
        const int oy = (int)((pix / p.wo) % p.ho);
        const long long img = pix / ((long long)p.wo * p.ho);
        const float* xi = p.x + img * p.h * p.w * (long long)p.ld_x + 4 * q;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (UP) {
            // Y = 2y + i - 1: even Y takes (i, y) = (1, Y/2), (3, Y/2 - 1); odd Y takes (0, (Y+1)/2), (2, (Y-1)/2).  The loops run over
            // all sixteen (i, j) with the parity as a predicate, so that every weight index is a compile-time constant (kernel arguments
            // indexed per lane would be copied to scratch).
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int y = (oy + 1 - i) >> 1;
                if (((oy + 1 - i) & 1) || (unsigned)y >= (unsigned)p.h) continue;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int x = (ox + 1 - j) >> 1;
                    if (((ox + 1 - j) & 1) || (unsigned)x >= (unsigned)p.w) continue;
                    const f32x4 v = *reinterpret_cast<const f32x4*>(xi + ((long long)y * p.w + x) * p.ld_x);
                    const float wt = p.w2d[i * 4 + j];
                    acc.x = fmaf(wt, v.x, acc.x); acc.y = fmaf(wt, v.y, acc.y); acc.z = fmaf(wt, v.z, acc.z); acc.w = fmaf(wt, v.w, acc.w);
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int y = 2 * oy + i - p.pad;
                if ((unsigned)y >= (unsigned)p.h) continue;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int x = 2 * ox + j - p.pad;
                    if ((unsigned)x >= (unsigned)p.w) continue;
                    const f32x4 v = *reinterpret_cast<const f32x4*>(xi + ((long long)y * p.w + x) * p.ld_x);
                    const float wt = p.w2d[i * 4 + j];
                    acc.x = fmaf(wt, v.x, acc.x); acc.y = fmaf(wt, v.y, acc.y); acc.z = fmaf(wt, v.z, acc.z); acc.w = fmaf(wt, v.w, acc.w);
                }
            }
        }
        if (p.bias) acc += *reinterpret_cast<const f32x4*>(p.bias + 4 * q);
        if (p.res) acc += *reinterpret_cast<const f32x4*>(p.res + pix * p.res_ld + 4 * q);
        acc *= p.out_scale;
        *reinterpret_cast<f32x4*>(p.out + pix * p.out_ld + 4 * q) = acc;
    }
}

template <typename T>
__global__ void __launch_bounds__(256) zero_border_kernel(const T* __restrict__ x, T* __restrict__ out, long long total, int h, int w, int inner,
                                                          int p) {
    const int H = h + 2 * p, W = w + 2 * p;
    const long long step = (long long)gridDim.x * 256;
    for (long long idx = (long long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += step) {
        const int q = (int)(idx % inner);
        const long long pix = idx / inner;
        const int X = (int)(pix % W) - p;
        const int Y = (int)((pix / W) % H) - p;
        const long long o = pix / ((long long)W * H);
        T v = {};
        if ((unsigned)Y < (unsigned)h && (unsigned)X < (unsigned)w) v = x[((o * h + Y) * w + X) * inner + q];
        out[idx] = v;
    }
}

inline unsigned fir_blocks(long long total) {
    const long long b = (total + 255) / 256;
    return (unsigned)(b < FIR_MAX_BLOCKS ? b : FIR_MAX_BLOCKS);
}

inline int fir_out_size(int in, int up, int pad) {
    if (up) return 2 * in;
    const int span = in + 2 * pad - 4;
    return (span < 0 || (span & 1)) ? -1 : span / 2 + 1;
}

}  // namespace

extern "C" int dsm_fir_resample_supported(int up, int pad, int h, int w, int c) {
    if (h <= 0 || w <= 0 || c <= 0 || (c & 3) || (up != 0 && up != 1)) return 0;
    if (up ? pad != 1 : (pad != 0 && pad != 1)) return 0;
    return fir_out_size(h, up, pad) > 0 && fir_out_size(w, up, pad) > 0;
}

extern "C" int dsm_fir_resample(const dsm_fir_args* a, void* stream) {
    if (!a || !a->x || !a->out || a->x == a->out) return DS_E_ARG;
    if (a->reserved[0] || a->reserved[1] || a->reserved[2]) return DS_E_ARG;
    if (a->n <= 0 || a->h <= 0 || a->w <= 0 || a->c <= 0) return DS_E_ARG;
    if ((a->up != 0 && a->up != 1) || (a->up ? a->pad != 1 : (a->pad != 0 && a->pad != 1))) return DS_E_ARG;
    if (a->ld_x < a->c || a->out_ld < a->c || (a->res && a->res_ld < a->c)) return DS_E_ARG;
    if ((a->c & 3) || (a->ld_x & 3) || (a->out_ld & 3) || (a->res && (a->res_ld & 3))) return DS_E_ALIGN;
    if (!ds_aligned16(a->x) || !ds_aligned16(a->out) || (a->bias && !ds_aligned16(a->bias)) || (a->res && !ds_aligned16(a->res))) return DS_E_ALIGN;
    const float fsum = a->taps[0] + a->taps[1] + a->taps[2] + a->taps[3];
    if (!(fsum * fsum > 0.f) || !(fsum * fsum < 3.0e38f)) return DS_E_ARG;           // also refuses NaN taps
    const int ho = fir_out_size(a->h, a->up, a->pad), wo = fir_out_size(a->w, a->up, a->pad);
    if (ho <= 0 || wo <= 0) return DS_E_SHAPE;
    if ((long long)a->n * a->h * a->w > 0x7fffffffLL || (long long)a->n * ho * wo > 0x7fffffffLL) return DS_E_SHAPE;
    FirParams p;
    p.x = a->x; p.bias = a->bias; p.res = a->res; p.out = a->out;
    p.ld_x = a->ld_x; p.res_ld = a->res_ld; p.out_ld = a->out_ld;
    p.h = a->h; p.w = a->w; p.ho = ho; p.wo = wo; p.c4 = a->c >> 2; p.pad = a->pad;
    p.out_scale = a->out_scale;
    p.total = (long long)a->n * ho * wo * p.c4;
    const float den = fsum * fsum;                              // f.sum().square()
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            const float f2d = (a->taps[i] * a->taps[j]) / den;    // f.ger(f) / f.sum().square(), in fp32 like the reference's buffer
            p.w2d[i * 4 + j] = a->up ? f2d * 4.0f : f2d;
        }
    (void)hipGetLastError();
    if (a->up)
        hipLaunchKernelGGL(fir_resample_kernel<true>, dim3(fir_blocks(p.total)), dim3(256), 0, (hipStream_t)stream, p);
    else
        hipLaunchKernelGGL(fir_resample_kernel<false>, dim3(fir_blocks(p.total)), dim3(256), 0, (hipStream_t)stream, p);
    DS_CHECK_LAUNCH();
    return DS_OK;
}

extern "C" int dsm_zero_border(const float* x, float* out, long long outer, int h, int w, int inner, int p, void* stream) {
    if (!x || !out || x == out || outer <= 0 || h <= 0 || w <= 0 || inner <= 0 || p < 0) return DS_E_ARG;
    if (p > 32768 || h > 32768 || w > 32768) return DS_E_SHAPE;
    const long long pixels = outer * (h + 2 * p) * (long long)(w + 2 * p);
    if (pixels > 0x7fffffffLL) return DS_E_SHAPE;
    (void)hipGetLastError();
    if (!(inner & 3)) {
        if (!ds_aligned16(x) || !ds_aligned16(out)) return DS_E_ALIGN;
        const long long total = pixels * (inner >> 2);
        hipLaunchKernelGGL(zero_border_kernel<f32x4>, dim3(fir_blocks(total)), dim3(256), 0, (hipStream_t)stream,
                           reinterpret_cast<const f32x4*>(x), reinterpret_cast<f32x4*>(out), total, h, w, inner >> 2, p);
    } else {
        if ((reinterpret_cast<uintptr_t>(x) & 3u) || (reinterpret_cast<uintptr_t>(out) & 3u)) return DS_E_ALIGN;
        const long long total = pixels * inner;
        hipLaunchKernelGGL(zero_border_kernel<float>, dim3(fir_blocks(total)), dim3(256), 0, (hipStream_t)stream, x, out, total, h, w, inner, p);
    }
    DS_CHECK_LAUNCH();
    return DS_OK;
}
