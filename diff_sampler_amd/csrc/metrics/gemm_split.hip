// dsm_gemm_split -- a Linear layer with fp32 operands and fp32 results on the fp16 matrix pipe (gfx950):
//
//     out[rows][cout] = act(x[rows][k] . W^T . 2^-shift + bias) + res
//
// Every fp32 operand is two fp16 halves, hi = fp16(v) and lo = fp16(v - hi) (the difference is exact in fp32), and a product is three
// v_mfma_f32_32x32x16_f16 into one fp32 accumulator: hi.hi + hi.lo + lo.hi (lo.lo is below 2^-22 of the product and dropped).  This is
// the split of ../conv3x3_halo2.hip.  The weights are split once on the host (ops.pack_linear_weight_split: scaled by 2^shift so that
// both halves of every weight of any size sit in fp16's normal range, 32 hi halves then 32 lo halves per 32-column K block, rows padded
// to 128); the activations are split while their tile is staged, unscaled: |x| <= 65504, and below 2^-3 the lo half is an fp16
// subnormal (quantum 2^-24).
//
// Tile: one workgroup of 256 threads (4 waves, launch bound 2 workgroups per CU) = 128 rows x 128 output columns, a wave = 64 x 64 =
// 2 x 2 accumulators of 32 x 32 (64 registers).  K advances 32 columns per step.  Both operand tiles have the same LDS image: 128 tile
// rows of 128 bytes = 8 chunks of 16 bytes (chunks 0-3: hi halves of k 0-7 .. 24-31, chunks 4-7: the lo halves), chunk c of row r stored
// at chunk c ^ ((r >> 1) & 7), so that the 16 rows a ds_read_b128 fragment read touches together cover all 64 banks once.  Two such
// image pairs (2 x 32 KB = 64 KB of LDS per workgroup, 128 KB per CU): step kt + 1 is loaded to registers before the MFMAs of step kt,
// split and written to the other pair after them -- ONE barrier per K step.  Per step and wave: 16 ds_read_b128, 24 MFMAs.
//
// The W tile is the A operand and the x tile the B operand of the MFMA, so an accumulator has its x row on the lane and 4 consecutive
// output columns in 4 consecutive registers: the epilogue (exact 2^-shift, bias, activation, residual) works on float4 and stores rows
// directly.  Rows at or beyond `rows` are loaded from the clamped row rows - 1 and never stored; output columns at or beyond cout
// (cout % 32 == 0: whole 32-column blocks) read the packing's zero rows and are never stored.  No split-K, no atomics: a row's bits
// depend on that row and the weights alone.
#include "../ds_common.h"
#include "ds_metrics.h"

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));

constexpr int GS_TM = 128;                    // x rows per workgroup
constexpr int GS_TN = 128;                    // output columns per workgroup
constexpr int GS_TILE_B = 128 * 128;          // bytes of one operand image
constexpr int GS_LDS_B = 4 * GS_TILE_B;       // {x, W} x two stages

struct GsParams {
    const float* x; const _Float16* w; const float* bias; const float* res; float* out;
    long long rows;
    int ldx, k, cout, res_ld, out_ld, nct;
    float scale;
};

__device__ __forceinline__ unsigned gs_at(int row, int chunk) { return (unsigned)(row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4)); }

__device__ __forceinline__ float gs_gelu_erf(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f)); }      // dsm_gelu_rows' form
__device__ __forceinline__ float gs_quick_gelu(float v) { return v * __builtin_amdgcn_rcpf(1.0f + __expf(-1.702f * v)); }    // ds_quick_gelu's form

template <int ACT>
__global__ void __launch_bounds__(256, 2) gemm_split_kernel(const GsParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gs_smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hb = lane >> 5, l31 = lane & 31;
    const int wm = wave & 1, wn = wave >> 1;
    const int ct = (int)(blockIdx.x % (unsigned)p.nct);
    const long long r0 = (long long)(blockIdx.x / (unsigned)p.nct) * GS_TM;
    const int n0 = ct * GS_TN;
    const int nk = p.k >> 5;

    // staging slots: x = 2 x (row, 8-column chunk) per thread, W = 4 x (row, 16-byte chunk) per thread
    const float* xsrc[2];
    unsigned xdst[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int i = tid + 256 * j, row = i >> 2, kc = i & 3;
        long long gr = r0 + row;
        gr = gr < p.rows ? gr : p.rows - 1;                                     // never beyond the tensor
        xsrc[j] = p.x + (size_t)gr * p.ldx + kc * 8;
        xdst[j] = gs_at(row, kc);
    }
    const _Float16* wsrc[4];
    unsigned wdst[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = tid + 256 * j, row = i >> 3, ch = i & 7;
        wsrc[j] = p.w + (size_t)(n0 + row) * (2 * (size_t)p.k) + ch * 8;        // rows exist up to the next multiple of 128
        wdst[j] = GS_TILE_B + gs_at(row, ch);
    }

    f32x4 xr[2][2];
    h8 wr[4];
    auto gload = [&](int kt) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            xr[j][0] = *reinterpret_cast<const f32x4*>(xsrc[j] + (size_t)kt * 32);
            xr[j][1] = *reinterpret_cast<const f32x4*>(xsrc[j] + (size_t)kt * 32 + 4);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) wr[j] = *reinterpret_cast<const h8*>(wsrc[j] + (size_t)kt * 64);
    };
    auto sstore = [&](unsigned char* stage) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            h8 hi, lo;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float v = xr[j][e >> 2][e & 3];
                hi[e] = (_Float16)v;
                lo[e] = (_Float16)(v - (float)hi[e]);                           // the difference is exact in fp32
            }
            *reinterpret_cast<h8*>(stage + xdst[j]) = hi;
            *reinterpret_cast<h8*>(stage + (xdst[j] ^ 64u)) = lo;               // chunk + 4: bit 2 of the chunk index, which the swizzle keeps
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) *reinterpret_cast<h8*>(stage + wdst[j]) = wr[j];
    };

    f32x16 acc[2][2];                                                           // [32 output columns cb][32 rows rb] of the wave's 64 x 64
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    gload(0);
    sstore(gs_smem);
    __syncthreads();

    for (int kt = 0; kt < nk; ++kt) {
        const unsigned char* cur = gs_smem + (kt & 1) * (2 * GS_TILE_B);
        if (kt + 1 < nk) gload(kt + 1);                                         // in flight during the MFMAs below
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            h8 xh[2], xl[2], wh[2], wl[2];
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int xrow = wm * 64 + b * 32 + l31, wrow = wn * 64 + b * 32 + l31;
                xh[b] = *reinterpret_cast<const h8*>(cur + gs_at(xrow, 2 * s + hb));
                xl[b] = *reinterpret_cast<const h8*>(cur + gs_at(xrow, 4 + 2 * s + hb));
                wh[b] = *reinterpret_cast<const h8*>(cur + GS_TILE_B + gs_at(wrow, 2 * s + hb));
                wl[b] = *reinterpret_cast<const h8*>(cur + GS_TILE_B + gs_at(wrow, 4 + 2 * s + hb));
            }
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int rb = 0; rb < 2; ++rb) {
                    acc[cb][rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[cb], xh[rb], acc[cb][rb], 0, 0, 0);
                    acc[cb][rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[cb], xl[rb], acc[cb][rb], 0, 0, 0);
                    acc[cb][rb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[cb], xh[rb], acc[cb][rb], 0, 0, 0);
                }
        }
        if (kt + 1 < nk) sstore(gs_smem + ((kt + 1) & 1) * (2 * GS_TILE_B));    // the stage every wave left before the previous barrier
        __syncthreads();
    }

    // accumulator register r of lane (hb, l31): output column 8 (r >> 2) + 4 hb + (r & 3) of the 32-column block, x row l31 of the 32-row block
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
        const long long row = r0 + wm * 64 + rb * 32 + l31;
        if (row >= p.rows) continue;
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            const int cbase = n0 + wn * 64 + cb * 32;
            if (cbase >= p.cout) continue;                                      // cout % 32 == 0: a 32-column block is inside or outside
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int c = cbase + 8 * g + 4 * hb;
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = acc[cb][rb][4 * g + e] * p.scale;
                if (p.bias) v += *reinterpret_cast<const f32x4*>(p.bias + c);
                if constexpr (ACT == DSM_ACT_GELU) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = gs_gelu_erf(v[e]);
                } else if constexpr (ACT == DSM_ACT_QUICK_GELU) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = gs_quick_gelu(v[e]);
                } else {
                    if (p.res) v += *reinterpret_cast<const f32x4*>(p.res + (size_t)row * p.res_ld + c);
                }
                *reinterpret_cast<f32x4*>(p.out + (size_t)row * p.out_ld + c) = v;
            }
        }
    }
}

template <int ACT>
int gs_launch(const GsParams& p, unsigned blocks, hipStream_t stream) {
    DS_ENSURE_DYN_LDS((&gemm_split_kernel<ACT>), GS_LDS_B);
    hipLaunchKernelGGL((gemm_split_kernel<ACT>), dim3(blocks), dim3(256), GS_LDS_B, stream, p);
    DS_CHECK_LAUNCH();
    return DS_OK;
}

inline long long gs_blocks(long long rows, int cout) { return ((rows + GS_TM - 1) / GS_TM) * ((cout + GS_TN - 1) / GS_TN); }

}  // namespace

extern "C" int dsm_gemm_split_supported(long long rows, int k, int cout) {
    if (rows < 1 || k < 32 || cout < 32 || (k & 31) || (cout & 31)) return 0;
    if (rows > (1LL << 40)) return 0;
    return gs_blocks(rows, cout) <= 0x7fffffffLL;
}

extern "C" int dsm_gemm_split(const dsm_gemm_split_args* a, void* stream) {
    if (!a || !a->x || !a->w_split || !a->out) return DS_E_ARG;
    if (a->reserved[0] || a->reserved[1] || a->reserved[2]) return DS_E_ARG;
    if (a->act != DSM_ACT_NONE && a->act != DSM_ACT_GELU && a->act != DSM_ACT_QUICK_GELU) return DS_E_ARG;
    if (a->shift < 0 || a->shift > 126) return DS_E_ARG;
    if (a->res && (a->act != DSM_ACT_NONE || a->res == a->out)) return DS_E_ARG;
    if (!dsm_gemm_split_supported(a->rows, a->k, a->cout)) return DS_E_SHAPE;
    if (a->ldx < a->k || a->out_ld < a->cout || (a->res && a->res_ld < a->cout)) return DS_E_ARG;
    if ((a->ldx & 3) || (a->out_ld & 3) || (a->res && (a->res_ld & 3))) return DS_E_ALIGN;
    if (!ds_aligned16(a->x) || !ds_aligned16(a->w_split) || !ds_aligned16(a->out) || !ds_aligned16(a->bias) || !ds_aligned16(a->res)) return DS_E_ALIGN;
    (void)hipGetLastError();
    GsParams p;
    p.x = a->x; p.w = reinterpret_cast<const _Float16*>(a->w_split); p.bias = a->bias; p.res = a->res; p.out = a->out;
    p.rows = a->rows; p.ldx = a->ldx; p.k = a->k; p.cout = a->cout; p.res_ld = a->res_ld; p.out_ld = a->out_ld;
    p.nct = (a->cout + GS_TN - 1) / GS_TN;
    p.scale = __builtin_ldexpf(1.0f, -a->shift);
    const unsigned blocks = (unsigned)gs_blocks(a->rows, a->cout);
    switch (a->act) {
        case DSM_ACT_GELU: return gs_launch<DSM_ACT_GELU>(p, blocks, (hipStream_t)stream);
        case DSM_ACT_QUICK_GELU: return gs_launch<DSM_ACT_QUICK_GELU>(p, blocks, (hipStream_t)stream);
        default: return gs_launch<DSM_ACT_NONE>(p, blocks, (hipStream_t)stream);
    }
}
