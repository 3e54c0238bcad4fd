// CLIP score (clip_score.py of the four reference repositories) -- the device code both CLIP towers need beyond libdsamd.so's projections,
// LayerNorm, token embedding and causal attention.  fp32 throughout: the reference runs clip_score.py without autocast.
//
//   dsm_attention        bidirectional softmax(scale Q K^T) V at head size 88 (ViT-g-14: 1408 / 16), the formulation of ../attention.hip:
//                        everything transposed so that a query is a lane, v_mfma_f32_32x32x2_f32, online softmax, the P^T registers feed the
//                        P V MFMAs directly, scores never reach memory.  Block = 128 queries of one (image, head), 4 waves x 32 queries, K / V
//                        streamed in 32-key tiles through LDS, one tile ahead in registers.
//                            Q K^T: 88 channels = 11 fragments of 8 (ds_read_b128 of the K tile, pitch 92 floats: 23 odd, conflict free).
//                            P V:   O^T is 3 blocks of 32 rows; the head is staged ZERO-PADDED to 96 channels (pitch 104) and 88 are stored:
//                                   8 of the 96 rows of every P V MFMA column block are wasted = 1 / 12 of the P V work, 1 / 23 of all MFMAs.
//                        LDS: (32 x 92 + 32 x 104 + 32 + 4 x 32 x 33) floats = 42 112 bytes; registers: 44 (Q) + 48 (O^T) + 16 (S^T) + 24 (staged tile).
//                        Keys at or beyond skv are loaded from the clamped row skv - 1 and their scores set to -1e30 before the maximum, so
//                        their weight is exactly 0; query lanes at or beyond sq read the clamped row sq - 1 and store nothing.
//   dsm_gelu_rows        exact erf-GELU over rows (the laion towers' activation; ds_quick_gelu is the OpenAI towers').
//   dsm_vit_patch_rows   uint8 / fp32 NCHW images -> normalised patch rows, the A operand of the patch projection.
//   dsm_vit_tokens       class embedding | patch outputs, + position embedding.
//   dsm_gather_rows      out[i] = x[index[i]]: the class-token row per image, the end-of-text row per prompt.
//   dsm_clip_score       100 cos(a_i, b_i) per pair and their fp64 sum in a fixed order.
#include "../ds_common.h"
#include "ds_metrics.h"

namespace {

constexpr int AD = 88;                   // the head size
constexpr int A_DB = 3;                  // 32-row blocks of O^T
constexpr int A_KLD = AD + 4;            // 92
constexpr int A_VLD = A_DB * 32 + 8;     // 104: rows 4 apart land 32 banks apart
constexpr int A_NQ = AD / 8;             // 11 Q fragments
constexpr int A_D4 = AD / 4;             // 22 float4 per row
constexpr int A_KT = 32;                 // keys per tile
constexpr int A_NLD = (A_KT * A_D4 + 255) / 256;       // 3 float4 of K and of V per thread and tile (704 in all)
constexpr int A_LDS_FLOATS = A_KT * A_KLD + A_KT * A_VLD + 32 + 4 * 32 * 33;

__global__ void __launch_bounds__(256) attn88_kernel(const dsm_attn_args a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Ks = smem;
    float* Vs = smem + A_KT * A_KLD;
    float* Es = smem + A_KT * A_KLD + A_KT * A_VLD + 32;         // epilogue transposition patches, 32 x 33 floats per wave

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hb = lane >> 5, l31 = lane & 31;
    const int h = blockIdx.y, b = blockIdx.z;
    const int q0 = blockIdx.x * 128 + wave * 32;
    const bool active = q0 < a.sq;
    const float* qp = a.q + (size_t)b * a.q_bs + h * AD;
    const float* kp = a.k + (size_t)b * a.k_bs + h * AD;
    const float* vp = a.v + (size_t)b * a.v_bs + h * AD;

    // channels 88 .. 103 of the V tile: zero once (the tile stores below never touch them), so rows 88 .. 95 of O^T are sums of zeros
    for (int i = tid; i < A_KT * (A_VLD - AD); i += 256) Vs[(i / (A_VLD - AD)) * A_VLD + AD + i % (A_VLD - AD)] = 0.f;

    const float sc = a.scale * 1.4426950408889634f;              // exp as exp2: scale * log2(e) folded into Q
    f32x4 qf[A_NQ];
    {
        const int qrow = min(q0 + l31, a.sq - 1);
        const float* qr = qp + (size_t)qrow * a.ldq + 4 * hb;
#pragma unroll
        for (int ks = 0; ks < A_NQ; ++ks) qf[ks] = *reinterpret_cast<const f32x4*>(qr + 8 * ks) * sc;
    }
    f32x16 ot[A_DB];
#pragma unroll
    for (int i = 0; i < A_DB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) ot[i][r] = 0.f;
    float m = -1e30f, l = 0.f;

    f32x4 kr[A_NLD], vr[A_NLD];
    auto gload = [&](int t) {
#pragma unroll
        for (int j = 0; j < A_NLD; ++j) {
            const int idx = tid + 256 * j;
            if (idx < A_KT * A_D4) {
                const int row = idx / A_D4, c4 = idx - row * A_D4;
                const int key = min(t * A_KT + row, a.skv - 1);        // never beyond the tensor
                kr[j] = *reinterpret_cast<const f32x4*>(kp + (size_t)key * a.ldk + c4 * 4);
                vr[j] = *reinterpret_cast<const f32x4*>(vp + (size_t)key * a.ldv + c4 * 4);
            }
        }
    };
    auto sstore = [&]() {
#pragma unroll
        for (int j = 0; j < A_NLD; ++j) {
            const int idx = tid + 256 * j;
            if (idx < A_KT * A_D4) {
                const int row = idx / A_D4, c4 = idx - row * A_D4;
                *reinterpret_cast<f32x4*>(Ks + row * A_KLD + c4 * 4) = kr[j];
                *reinterpret_cast<f32x4*>(Vs + row * A_VLD + c4 * 4) = vr[j];
            }
        }
    };

    const int ntiles = (a.skv + A_KT - 1) / A_KT;
    gload(0);
    const float* kfrag = Ks + l31 * A_KLD + 4 * hb;
    for (int t = 0; t < ntiles; ++t) {
        __syncthreads();                     // every wave is done with the previous tile
        sstore();
        __syncthreads();
        if (t + 1 < ntiles) gload(t + 1);    // in flight during the MFMAs below
        if (!active) continue;

        f32x16 st;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < A_NQ; ++ks) {
            const f32x4 kv = *reinterpret_cast<const f32x4*>(kfrag + 8 * ks);
#pragma unroll
            for (int r = 0; r < 4; ++r) st = __builtin_amdgcn_mfma_f32_32x32x2f32(kv[r], qf[ks][r], st, 0, 0, 0);
        }
        if (t == ntiles - 1) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (t * A_KT + 4 * hb + (r & 3) + 8 * (r >> 2) >= a.skv) st[r] = -1e30f;
        }
        float mx = st[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, st[r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float mn = fmaxf(m, mx);
        const float alpha = __builtin_amdgcn_exp2f(m - mn);
        m = mn;
        float rs = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) { st[r] = __builtin_amdgcn_exp2f(st[r] - mn); rs += st[r]; }
        l = l * alpha + rs;
#pragma unroll
        for (int i = 0; i < A_DB; ++i) ot[i] *= alpha;
#pragma unroll
        for (int i = 0; i < A_DB; ++i) {
            const float* vcol = Vs + (4 * hb) * A_VLD + i * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float vv = vcol[((r & 3) + 8 * (r >> 2)) * A_VLD];
                ot[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(vv, st[r], ot[i], 0, 0, 0);
            }
        }
    }
    if (!active) return;

    const float inv = 1.0f / (l + __shfl_xor(l, 32));
    float* patch = Es + wave * (32 * 33);
    float* op = a.out + (size_t)b * a.o_bs + h * AD;
#pragma unroll
    for (int i = 0; i < A_DB; ++i) {
#pragma unroll
        for (int r = 0; r < 16; ++r) patch[l31 * 33 + (r & 3) + 8 * (r >> 2) + 4 * hb] = ot[i][r] * inv;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const int c4 = (lane & 7) * 4;
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            const int q = pass * 8 + (lane >> 3);
            f32x4 o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = patch[q * 33 + c4 + j];
            if (q0 + q < a.sq && i * 32 + c4 < AD)               // 88 of the 96 staged channels; nothing beyond the head's columns
                *reinterpret_cast<f32x4*>(op + (size_t)(q0 + q) * a.ldo + i * 32 + c4) = o;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// ---- row kernels --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }

__global__ void __launch_bounds__(256) gelu_rows_kernel(const float* __restrict__ x, int ldx, float* __restrict__ y, int ldy, long long rows, int c4s) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * c4s) return;
    const long long r = i / c4s;
    const int c = (int)(i - r * c4s) * 4;
    f32x4 v = *reinterpret_cast<const f32x4*>(x + r * ldx + c);
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = gelu_erf(v[j]);
    *reinterpret_cast<f32x4*>(y + r * ldy + c) = v;
}

struct PatchArgs {
    const void* img; float* out;
    int f32, n, size, patch, ld;
    float mean[3], std[3];
};

// (v - mean) / std as torchvision's Normalize rounds it: a subtraction and a true division, each rounded on its own
__device__ __forceinline__ float pixel_norm(float p, float mean, float std) {
#pragma clang fp contract(off)
    const float d = p - mean;
    return d / std;
}

// one thread per output element: row = (image, gy, gx), column = (channel, py, px); columns [3 P^2, ld) are zeros
__global__ void __launch_bounds__(256) patch_rows_kernel(const PatchArgs a) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int g = a.size / a.patch, pp = a.patch * a.patch;
    const long long total = (long long)a.n * g * g * a.ld;
    if (i >= total) return;
    const long long row = i / a.ld;
    const int col = (int)(i - row * a.ld);
    float v = 0.f;
    if (col < 3 * pp) {
        const int c = col / pp, rem = col - c * pp, py = rem / a.patch, px = rem - py * a.patch;
        const int img = (int)(row / (g * g)), cell = (int)(row - (long long)img * g * g), gy = cell / g, gx = cell - gy * g;
        const size_t at = (((size_t)img * 3 + c) * a.size + (gy * a.patch + py)) * a.size + gx * a.patch + px;
        const float p = a.f32 ? reinterpret_cast<const float*>(a.img)[at] : (float)reinterpret_cast<const unsigned char*>(a.img)[at] / 255.0f;
        v = pixel_norm(p, a.mean[c], a.std[c]);
    }
    a.out[i] = v;
}

// out[(b * tokens + t)][:] = (t == 0 ? cls : patches[b * (tokens - 1) + t - 1]) + pos[t]
__global__ void __launch_bounds__(256) vit_tokens_kernel(const float* __restrict__ patches, int ldp, const float* __restrict__ cls,
                                                         const float* __restrict__ pos, float* __restrict__ out, int ldo, int n, int tokens, int w4) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)n * tokens * w4) return;
    const long long row = i / w4;
    const int c = (int)(i - row * w4) * 4;
    const int b = (int)(row / tokens), t = (int)(row - (long long)b * tokens);
    const f32x4 src = t == 0 ? *reinterpret_cast<const f32x4*>(cls + c)
                             : *reinterpret_cast<const f32x4*>(patches + ((size_t)b * (tokens - 1) + t - 1) * ldp + c);
    *reinterpret_cast<f32x4*>(out + row * ldo + c) = src + *reinterpret_cast<const f32x4*>(pos + (size_t)t * (w4 * 4) + c);
}

__global__ void __launch_bounds__(256) gather_rows_kernel(const float* __restrict__ x, int ldx, long long x_rows, const int* __restrict__ index,
                                                          float* __restrict__ out, int ldo, int n, int c4s) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)n * c4s) return;
    const int r = (int)(i / c4s), c = (int)(i - (long long)r * c4s) * 4;
    long long src = index[r];
    src = src < 0 ? 0 : (src >= x_rows ? x_rows - 1 : src);          // the host validates; the kernel never reads beyond x
    *reinterpret_cast<f32x4*>(out + (size_t)r * ldo + c) = *reinterpret_cast<const f32x4*>(x + (size_t)src * ldx + c);
}

// one workgroup per pair: <a, b>, |a|^2, |b|^2 as per-thread strided partial sums and a fixed tree -- the same bits on every run
__global__ void __launch_bounds__(256) pair_score_kernel(const float* __restrict__ a, int lda, const float* __restrict__ b, int ldb, int dim,
                                                         float* __restrict__ scores) {
    __shared__ float red[3][256];
    const int p = blockIdx.x, t = threadIdx.x;
    const float* ar = a + (size_t)p * lda;
    const float* br = b + (size_t)p * ldb;
    float ab = 0.f, aa = 0.f, bb = 0.f;
    for (int c = t; c < dim; c += 256) {
        const float u = ar[c], v = br[c];
        ab += u * v; aa += u * u; bb += v * v;
    }
    red[0][t] = ab; red[1][t] = aa; red[2][t] = bb;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
            red[0][t] += red[0][t + s]; red[1][t] += red[1][t + s]; red[2][t] += red[2][t + s];
        }
        __syncthreads();
    }
    if (t == 0) scores[p] = 100.0f * (red[0][0] / (sqrtf(red[1][0]) * sqrtf(red[2][0])));
}

// *sum += scores[0] + ... + scores[n - 1] in fp64: thread t adds its contiguous run of pairs in pair order, thread 0 the 256 runs in order
__global__ void __launch_bounds__(256) score_sum_kernel(const float* __restrict__ scores, int n, double* __restrict__ sum) {
    __shared__ double part[256];
    const int t = threadIdx.x, per = (n + 255) / 256;
    double s = 0.0;
    for (int i = t * per; i < min(n, (t + 1) * per); ++i) s += (double)scores[i];
    part[t] = s;
    __syncthreads();
    if (t == 0) {
        double tot = 0.0;
        for (int i = 0; i < 256; ++i) tot += part[i];
        *sum += tot;
    }
}

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
inline bool grid_ok(long long threads) { return (threads + 255) / 256 <= 0x7fffffffLL; }

}  // namespace

extern "C" int dsm_attention_supported(int d) { return d == AD; }

extern "C" int dsm_attention(const dsm_attn_args* a, void* stream) {
    if (!a || !a->q || !a->k || !a->v || !a->out) return DS_E_ARG;
    if (a->reserved[0] || a->reserved[1] || a->reserved[2]) return DS_E_ARG;
    if (a->batch <= 0 || a->heads <= 0 || a->sq <= 0 || a->skv <= 0 || a->batch > 65535 || a->heads > 65535) return DS_E_ARG;
    if (!dsm_attention_supported(a->d)) return DS_E_SHAPE;
    const long long span = (long long)a->heads * a->d;
    if (a->ldq < span || a->ldk < span || a->ldv < span || a->ldo < span) return DS_E_ARG;
    if ((a->ldq & 3) || (a->ldk & 3) || (a->ldv & 3) || (a->ldo & 3) || (a->q_bs & 3) || (a->k_bs & 3) || (a->v_bs & 3) || (a->o_bs & 3))
        return DS_E_ALIGN;
    if (!ds_aligned16(a->q) || !ds_aligned16(a->k) || !ds_aligned16(a->v) || !ds_aligned16(a->out)) return DS_E_ALIGN;
    (void)hipGetLastError();
    constexpr int bytes = A_LDS_FLOATS * (int)sizeof(float);
    DS_ENSURE_DYN_LDS((&attn88_kernel), bytes);
    const dim3 grid((unsigned)((a->sq + 127) / 128), (unsigned)a->heads, (unsigned)a->batch);
    hipLaunchKernelGGL(attn88_kernel, grid, dim3(256), bytes, (hipStream_t)stream, *a);
    DS_CHECK_LAUNCH();
    return DS_OK;
}

extern "C" int dsm_gelu_rows(const float* x, int ldx, float* y, int ldy, long long rows, int cols, void* stream) {
    if (!x || !y || rows <= 0 || cols <= 0 || ldx < cols || ldy < cols) return DS_E_ARG;
    if ((cols & 3) || (ldx & 3) || (ldy & 3) || !ds_aligned16(x) || !ds_aligned16(y)) return DS_E_ALIGN;
    const long long total = rows * (cols >> 2);
    if (!grid_ok(total)) return DS_E_SHAPE;
    (void)hipGetLastError();
    hipLaunchKernelGGL(gelu_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, y, ldy, rows, cols >> 2);
    DS_CHECK_LAUNCH();
    return DS_OK;
}

extern "C" int dsm_vit_patch_rows(const void* images, int images_f32, int n, int size, int patch, const float* mean3, const float* std3,
                                  float* out, int ld, void* stream) {
    if (!images || !out || !mean3 || !std3 || n <= 0 || size <= 0 || patch <= 0) return DS_E_ARG;
    if (images_f32 != 0 && images_f32 != 1) return DS_E_ARG;
    if (size % patch || size > 32768) return DS_E_SHAPE;
    if (ld < 3 * patch * patch) return DS_E_ARG;
    if (std3[0] == 0.f || std3[1] == 0.f || std3[2] == 0.f) return DS_E_ARG;
    if (!ds_aligned16(out) || (images_f32 && !aligned4(images))) return DS_E_ALIGN;
    const long long g = size / patch, total = (long long)n * g * g * ld;
    if (!grid_ok(total) || (long long)n * g * g > 0x7fffffffLL) return DS_E_SHAPE;
    (void)hipGetLastError();
    PatchArgs a = {images, out, images_f32, n, size, patch, ld, {mean3[0], mean3[1], mean3[2]}, {std3[0], std3[1], std3[2]}};
    hipLaunchKernelGGL(patch_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    DS_CHECK_LAUNCH();
    return DS_OK;
}

extern "C" int dsm_vit_tokens(const float* patches, int ldp, const float* cls, const float* pos, float* out, int ldo, int n, int tokens, int width,
                              void* stream) {
    if (!patches || !cls || !pos || !out || n <= 0 || tokens < 2 || width <= 0 || ldp < width || ldo < width) return DS_E_ARG;
    if ((width & 3) || (ldp & 3) || (ldo & 3) || !ds_aligned16(patches) || !ds_aligned16(cls) || !ds_aligned16(pos) || !ds_aligned16(out)) return DS_E_ALIGN;
    const long long total = (long long)n * tokens * (width >> 2);
    if (!grid_ok(total) || (long long)n * tokens > 0x7fffffffLL) return DS_E_SHAPE;
    (void)hipGetLastError();
    hipLaunchKernelGGL(vit_tokens_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, patches, ldp, cls, pos, out, ldo, n,
                       tokens, width >> 2);
    DS_CHECK_LAUNCH();
    return DS_OK;
}

extern "C" int dsm_gather_rows(const float* x, int ldx, long long x_rows, const int* row_index, float* out, int ldo, int n, int cols, void* stream) {
    if (!x || !row_index || !out || x_rows <= 0 || n <= 0 || cols <= 0 || ldx < cols || ldo < cols) return DS_E_ARG;
    if ((cols & 3) || (ldx & 3) || (ldo & 3) || !ds_aligned16(x) || !ds_aligned16(out) || !aligned4(row_index)) return DS_E_ALIGN;
    if (x_rows > 0x7fffffffLL) return DS_E_SHAPE;
    (void)hipGetLastError();
    const long long total = (long long)n * (cols >> 2);
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, x_rows, row_index, out,
                       ldo, n, cols >> 2);
    DS_CHECK_LAUNCH();
    return DS_OK;
}

extern "C" int dsm_clip_score(const float* a, int lda, const float* b, int ldb, int n, int dim, float* scores, double* sum, void* stream) {
    if (!a || !b || !scores || !sum || n <= 0 || dim <= 0 || lda < dim || ldb < dim) return DS_E_ARG;
    if (!aligned4(a) || !aligned4(b) || !aligned4(scores) || (reinterpret_cast<uintptr_t>(sum) & 7u)) return DS_E_ALIGN;
    (void)hipGetLastError();
    hipLaunchKernelGGL(pair_score_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, a, lda, b, ldb, dim, scores);
    DS_CHECK_LAUNCH();
    hipLaunchKernelGGL(score_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, scores, n, sum);
    DS_CHECK_LAUNCH();
    return DS_OK;
}
