// Dynamic thresholding of DPM-Solver++ (solver_utils.py:77-86) for samples that do not fit the LDS form of libdsamd's ds_dynamic_threshold
// (more than 38 144 values per sample: images of 128 pixels and above -- the LSUN-256 consistency-model nets):
//
//   dsm_dynamic_threshold_large   out = clamp(x0, -s, s) / s per sample, s = max(quantile_p(|x0|), 1), torch.quantile's linear interpolation.
//
// The same selection as dynamic_threshold_kernel (csrc/solver.hip): an 8-bit-digit radix select over the bit patterns of |x0| finds the order
// statistic at floor(p (n - 1)), one more scan its upper neighbour, at::lerp combines them.  What differs is where the keys live: they are
// recomputed from global memory in each of the four digit passes and in the neighbour scan (a sample of 196 608 values is 768 KB: it stays in
// L2), and LDS holds the 256-bin histogram only.  One workgroup per sample.  ds_dynamic_threshold itself is unchanged and keeps refusing such
// samples; solver_utils.dynamic_thresholding_fn sends them here.
// In place (out == x0) is allowed: a workgroup touches its own sample only and a barrier separates its last read from its first write.
#include "../ds_common.h"
#include "ds_metrics.h"

namespace {

__global__ void __launch_bounds__(512) dynamic_threshold_large_kernel(const float* x0, float* out, int per, float p) {
    __shared__ unsigned hist[256];
    __shared__ unsigned s_cnt;
    __shared__ unsigned s_min;
    const float* x = x0 + (size_t)blockIdx.x * per;
    float* y = out + (size_t)blockIdx.x * per;
    auto key = [x](int i) { return __float_as_uint(fabsf(x[i])); };
    if (threadIdx.x == 0) { s_cnt = 0; s_min = 0xffffffffu; }
    const float rankf = p * (float)(per - 1);       // fp32, as ATen computes it
    const float lo_f = floorf(rankf);
    const float w = rankf - lo_f;
    const unsigned lo = (unsigned)lo_f;
    const unsigned hi = (unsigned)ceilf(rankf);
    // ---- radix select of the order statistic `lo`, most significant digit first ----
    unsigned prefix = 0, mask = 0, rank = lo;
    for (int pass = 3; pass >= 0; --pass) {
        const int shift = pass * 8;
        for (int i = threadIdx.x; i < 256; i += blockDim.x) hist[i] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < per; i += blockDim.x) {
            const unsigned v = key(i);
            if ((v & mask) == prefix) atomicAdd(&hist[(v >> shift) & 255u], 1u);
        }
        __syncthreads();
        unsigned cum = 0, digit = 0, before = 0;     // every thread scans the histogram: a uniform result
        for (int b = 0; b < 256; ++b) {
            const unsigned hcount = hist[b];
            if (cum + hcount > rank) { digit = (unsigned)b; before = cum; break; }
            cum += hcount;
        }
        rank -= before;
        prefix |= digit << shift;
        mask |= 255u << shift;
        __syncthreads();
    }
    const unsigned v_lo = prefix;
    unsigned v_hi = v_lo;
    if (hi != lo) {                                  // (uniform) the next order statistic: v_lo again if it repeats, else the smallest key above it
        unsigned cnt = 0, mn = 0xffffffffu;
        for (int i = threadIdx.x; i < per; i += blockDim.x) {
            const unsigned v = key(i);
            if (v <= v_lo) ++cnt; else mn = min(mn, v);
        }
        atomicAdd(&s_cnt, cnt);
        atomicMin(&s_min, mn);
        __syncthreads();
        v_hi = (s_cnt >= hi + 1) ? v_lo : s_min;
    }
    const float a = __uint_as_float(v_lo), b = __uint_as_float(v_hi);
    float s = (w < 0.5f) ? a + w * (b - a) : b - (b - a) * (1.0f - w);       // at::lerp
    s = fmaxf(s, 1.0f);
    __syncthreads();                                 // every read of the sample precedes the first (possibly in-place) write
    for (int i = threadIdx.x; i < per; i += blockDim.x) {
        const float v = fminf(fmaxf(x[i], -s), s);
        y[i] = v / s;
    }
}

}  // namespace

extern "C" int dsm_dynamic_threshold_large(const float* x0, float* out, int n, int per, float p, void* stream) {
    if (!x0 || !out || n <= 0 || per <= 1 || !(p >= 0.0f && p <= 1.0f)) return DS_E_ARG;
    if (per > (1 << 24)) return DS_E_SHAPE;          // p (n - 1) in fp32, like ATen: exact ranks up to 2^24 values per sample
    (void)hipGetLastError();
    hipLaunchKernelGGL(dynamic_threshold_large_kernel, dim3(n), dim3(512), 0, (hipStream_t)stream, x0, out, per, p);
    DS_CHECK_LAUNCH();
    return DS_OK;
}
