// 3x3 stride-1 convolution in the Winograd form F(2x2, 3x3) on the exact-fp32 MFMA (gfx950).
//
// The direct LDS-halo kernel (conv3x3_halo.hip) runs at 0.88 of the fp32 matrix peak on the 256 x 256 tile: only removing multiply-adds makes
// those layers faster.  F(2x2, 3x3) computes a 2 x 2 output patch ("tile") from a 4 x 4 input patch with 16 multiplies per (cin, cout) pair
// instead of 36 -- 2.25 x fewer MFMA operations, still in fp32:
//     Y = A^T [ sum_c (G g_c G^T) . (B^T d_c B) ] A          (. = elementwise over the 16 positions; entries of A, B: 0, +-1; of G: 0, +-1, +-1/2)
// i.e. 16 independent [tiles x channels] x [channels x cout] products, one per position of the 4 x 4 transformed patch.
//
//   workgroup = 64 tiles (256 output pixels of ONE image: TH = 256 / W rows x W columns, the 256-pixel M tile of the direct kernel) x 64
//               output channels, four waves (2 x 2), one per SIMD; a wave holds ALL 16 positions of its 32 tiles x 32 channels
//               (16 x f32x16 = 256 accumulator registers), so the output transform is lane-local
//   slab      = 8 input channels.  Per slab: the raw halo (TH+2) x (W+2) pixels x 8 channels goes global -> registers -> LDS `Hs` with the
//               consumer's GroupNorm affine + SiLU applied on the way (norm_coefs; out-of-image pixels are written as zeros AFTER the
//               activation), is transformed to V = B^T d B in LDS `Vs` (16 positions x 64 tiles x 8 channels), and the transformed weights
//               U of the workgroup's 64 columns (ops.pack_conv_weight_wino, already in the LDS image's order) stream global -> LDS by
//               LDS-DMA into a double buffer `Us`.  16 positions x 4 K steps of v_mfma_f32_32x32x2_f32 per wave and slab.
//   LDS image = [position][channel quad kh = 0 / 1][row 0..63][4 floats] for U and V alike: an MFMA fragment read is one ds_read_b128 per
//               lane at (kh = lane >> 5, row = lane & 31), 512 contiguous bytes per 32 lanes -- conflict-free, and the K index of step r is
//               channel 4 kh + r on both operands.  Hs is split into planes [kh][column parity][row][column / 2][4] so that the tiles of a
//               row (pixels two apart) read consecutive 16-byte cells.
//   sum order = slab order, then the channel order inside the MFMA; no split-K, no dependence on batch or grid.
//   epilogue  = the direct kernel's, in its order: acc_scale, bias, per-image cbias, res, out_scale, act, non-temporal stores, and the
//               GroupNorm column sums of 64-pixel blocks (a wave's 32 tiles x one patch row = 64 pixels; an image's HW / 64 blocks stay
//               contiguous, which is all ds_gn_finalize assumes).
//
// Who orders what: barrier A after the transform (Vs published, Hs dead), barrier C after the slab's MFMAs (Vs and the
// weight buffer dead; `s_waitcnt vmcnt(0)` in front of it: the next slab's weights have landed); the weight DMA of slab s+1 and the halo
// store of slab s+1 are issued between A and C.
#include "igemm_common.h"

namespace igemm {
namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

// timing ablations (wrong results on purpose; compiled only with -DDS_CONV_ABLATIONS, selected by tune.variant = 0x10000 + bits)
constexpr int WV_NO_NORM = 2, WV_NO_HALO = 4, WV_NO_DMA = 8, WV_NO_EPI = 16;
constexpr int WINO_K = 8;                         // channels per slab
constexpr int WINO_POS = 2 * 64 * 4;              // floats per position of an LDS image
constexpr int WINO_IMG = 16 * WINO_POS;           // floats per U / V image (8192)
constexpr int WINO_NSH = 4;                       // halo float4 slots per thread: NP * 2 <= 1024
constexpr int WINO_EPI_LD = 36;                   // epilogue staging row: 32 + 4 floats

__device__ float g_zero_page_wino[64];            // zero-initialised

// `s_waitcnt vmcnt(0)` as the BUILTIN (simm16: vmcnt 0, expcnt 7, lgkmcnt 15), not inline asm: the compiler's own wait-count pass sees it, so it
// knows that the halo registers requested a slab ago are there and does not put a second vmcnt(0) -- which would also wait for the weight DMA
// just issued -- in front of the halo store in the middle of the slab's MFMAs.
#define DS_WINO_WAIT_VM0() do { __builtin_amdgcn_s_waitcnt(0x0F70); asm volatile("" ::: "memory"); } while (0)

template <int VAR>
__global__ void __launch_bounds__(256, 1) conv3x3_wino_kernel(const KParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Us = smem;                              // [2][16][2][64][4]
    float* Vs = smem + 2 * WINO_IMG;               // [16][2][64][4]
    float* Hs = Vs + WINO_IMG;                     // [2][2][HP][WP / 2][4]

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    int mt, nt;
    if (!decode_tile(blockIdx.x, p.mtiles, p.ntiles, mt, nt)) return;
    const int m0 = mt * 256, n0 = nt * 64;
    const int img0 = m0 / p.HW;
    const int r0 = (m0 - img0 * p.HW) / p.W;
    const int WPH = p.WP >> 1, Wt = p.W >> 1;
    const int Ctot = p.c0 + p.c1;
    const int nslabs = Ctot / WINO_K;
    const float* zero = g_zero_page_wino;

    // ---- halo slots of this thread: (halo pixel, channel quad), fixed for the whole K loop ------------------------------------------
    const int kh_h = tid & 1;
    int h_pix[WINO_NSH], h_lds[WINO_NSH];
#pragma unroll
    for (int j = 0; j < WINO_NSH; ++j) {
        const int hp = (tid + j * 256) >> 1;
        const int hr = hp / p.WP, hc = hp - hr * p.WP;
        const int y = r0 + hr - 1, x = hc - 1;
        const bool in = hp < p.NP;
        const bool ok = in && (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W;
        h_pix[j] = ok ? (img0 * p.H + y) * p.W + x : -1;
        h_lds[j] = in ? (((kh_h * 2 + (hc & 1)) * p.HP + hr) * WPH + (hc >> 1)) * 4 : -1;
    }
    f32x4 hreg[WINO_NSH];
    auto halo_load = [&](int s) {
        const int c = s * WINO_K;
        const bool first = c < p.c0;
        const float* src = first ? p.a0 + c + kh_h * 4 : p.a1 + (c - p.c0) + kh_h * 4;
        const int ld = first ? p.lda0 : p.lda1;
#pragma unroll
        for (int j = 0; j < WINO_NSH; ++j) {
            const float* ptr = h_pix[j] >= 0 ? src + (size_t)h_pix[j] * ld : zero;
            hreg[j] = *reinterpret_cast<const f32x4*>(ptr);
        }
    };
    // the consumer's GroupNorm affine + SiLU, applied once per element while the halo is written (planes {mu, A, B} of the tile's image)
    const bool norm_on = p.norm != nullptr;
    f32x4 cmu = {0.f, 0.f, 0.f, 0.f}, cga = {1.f, 1.f, 1.f, 1.f}, cbe = {0.f, 0.f, 0.f, 0.f};
    auto coef_load = [&](int s) {
        const float* cp = norm_on ? p.norm + (size_t)img0 * 3 * Ctot + s * WINO_K + kh_h * 4 : zero;
        const int st = norm_on ? Ctot : 0;
        cmu = *reinterpret_cast<const f32x4*>(cp);
        cga = *reinterpret_cast<const f32x4*>(cp + st);
        cbe = *reinterpret_cast<const f32x4*>(cp + 2 * st);
    };
    auto halo_store = [&]() {
        const bool do_norm = norm_on && !(VAR & WV_NO_NORM);
        DS_RACE_SKEW(wave);
#pragma unroll
        for (int j = 0; j < WINO_NSH; ++j) {
            f32x4 v = hreg[j];
            if (do_norm && h_pix[j] >= 0) {
                v = (v - cmu) * cga + cbe;
                if (p.norm_act == DS_ACT_SILU) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = ds_silu(v[e]);
                }
            }
            if (h_lds[j] >= 0) *reinterpret_cast<f32x4*>(Hs + h_lds[j]) = v;
        }
    };

    // ---- input transform: this thread owns (tile t_t, channels 4 kh_t + 2 cpl .. + 1) -----------------------------------------------
    const int t_t = (tid >> 1) & 63, cpl = tid & 1, kh_t = tid >> 7;
    const int t_ty = t_t / Wt, t_tx = t_t - t_ty * Wt;
    const float* h_rd = Hs + ((kh_t * 2 * p.HP + 2 * t_ty) * WPH + t_tx) * 4 + cpl * 2;
    const int h_par = p.HP * WPH * 4;              // odd-column plane
    float* v_wr = Vs + (kh_t * 64 + t_t) * 4 + cpl * 2;
    auto transform = [&]() {
        f32x2 d[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                d[i][j] = *reinterpret_cast<const f32x2*>(h_rd + (j & 1) * h_par + i * WPH * 4 + (j >> 1) * 4);
        DS_RACE_SKEW(wave);
        f32x2 t[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {              // B^T d
            t[0][j] = d[0][j] - d[2][j];
            t[1][j] = d[1][j] + d[2][j];
            t[2][j] = d[2][j] - d[1][j];
            t[3][j] = d[1][j] - d[3][j];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {              // (B^T d) B
            *reinterpret_cast<f32x2*>(v_wr + (i * 4 + 0) * WINO_POS) = t[i][0] - t[i][2];
            *reinterpret_cast<f32x2*>(v_wr + (i * 4 + 1) * WINO_POS) = t[i][1] + t[i][2];
            *reinterpret_cast<f32x2*>(v_wr + (i * 4 + 2) * WINO_POS) = t[i][2] - t[i][1];
            *reinterpret_cast<f32x2*>(v_wr + (i * 4 + 3) * WINO_POS) = t[i][1] - t[i][3];
        }
    };

    // ---- transformed weights of slab s -> buffer buf: 8 LDS-DMA instructions per wave, source already in the LDS image's order --------
    auto u_dma = [&](int s, int buf) {
        const float* src = p.b + ((size_t)nt * nslabs + s) * WINO_IMG + tid * 4;
        DS_RACE_SKEW(wave);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float* dst = Us + buf * WINO_IMG + (i * 256 + wave * 64) * 4;          // wave-uniform base; the DMA writes lane-linear
            typedef const __attribute__((address_space(1))) void* gptr_t;
            typedef __attribute__((address_space(3))) void* lptr_t;
            __builtin_amdgcn_global_load_lds((gptr_t)(src + i * 1024), (lptr_t)(dst), 16, 0, 0);
        }
    };

    f32x16 acc[16];
#pragma unroll
    for (int q = 0; q < 16; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
    const int a_off = ((lane >> 5) * 64 + wr * 32 + (lane & 31)) * 4;
    const int b_off = ((lane >> 5) * 64 + wc * 32 + (lane & 31)) * 4;
    // positions [Q0, Q0 + 4): four independent accumulators per K step
#define DS_WINO_MFMA4(Q0, ub)                                                                                               \
    {                                                                                                                       \
        f32x4 fa[4], fb[4];                                                                                                 \
        _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                                                     \
            fa[q] = *reinterpret_cast<const f32x4*>(Vs + ((Q0) + q) * WINO_POS + a_off);                                    \
            fb[q] = *reinterpret_cast<const f32x4*>((ub) + ((Q0) + q) * WINO_POS + b_off);                                  \
        }                                                                                                                   \
        _Pragma("unroll") for (int r = 0; r < 4; ++r)                                                                       \
            _Pragma("unroll") for (int q = 0; q < 4; ++q)                                                                   \
                acc[(Q0) + q] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q][r], fb[q][r], acc[(Q0) + q], 0, 0, 0);           \
    }

    // ---- prologue --------------------------------------------------------------------------------------------------------------------
    halo_load(0);
    coef_load(0);
    u_dma(0, 0);
    halo_store();
    if (nslabs > 1) { halo_load(1); coef_load(1); }
    DS_WINO_WAIT_VM0();
    __syncthreads();

    for (int s = 0; s < nslabs; ++s) {
        const float* ub = Us + (s & 1) * WINO_IMG;
        transform();                                   // Hs -> Vs (Vs died at barrier C of the previous slab)
        __syncthreads();                               // A: Vs published, Hs dead
        if (s + 1 < nslabs) {
            if (!(VAR & WV_NO_DMA)) u_dma(s + 1, (s + 1) & 1);     // that buffer was last read by the MFMAs of slab s-1 (barrier C passed)
            if (!(VAR & WV_NO_HALO)) {
                halo_store();                          // slab s+1 (its loads were issued a slab ago, landed at barrier C)
                // the loads of slab s+2 go out BEFORE the slab's MFMAs: they must have landed at barrier C (vmcnt(0) for the weight DMA)
                if (s + 2 < nslabs) { halo_load(s + 2); coef_load(s + 2); }
            }
        }
        DS_WINO_MFMA4(0, ub)
        DS_WINO_MFMA4(4, ub)
        DS_WINO_MFMA4(8, ub)
        DS_WINO_MFMA4(12, ub)
        DS_WINO_WAIT_VM0();                            // the LDS-DMA of slab s+1 has landed (hipcc waits only in front of LDS reads it can tie to it)
        __syncthreads();                               // C: Vs, Us[s & 1] dead; Hs and Us[(s+1) & 1] published
    }
#undef DS_WINO_MFMA4

    if constexpr ((VAR & WV_NO_EPI) != 0) {
#pragma unroll
        for (int q = 0; q < 16; ++q) asm volatile("" :: "v"(acc[q]));
        return;
    }

    // ---- output transform Y = A^T M A (lane-local): Y[a * 2 + b] = the wave's 32 tiles x 32 channels at patch pixel (a, b) ---------------
    f32x16 Y[4];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        f32x16 t[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) t[j] = a == 0 ? acc[j] + acc[4 + j] + acc[8 + j] : acc[4 + j] - acc[8 + j] - acc[12 + j];
        Y[a * 2 + 0] = t[0] + t[1] + t[2];
        Y[a * 2 + 1] = t[1] - t[2] - t[3];
    }

    // ---- appended 1x1 slabs (the fused skip projection; e0 | e1, 32 raw channels per slab): four plain MFMA groups on the post-transform
    // accumulators, one per patch pixel.  The slab's 256 pixels x 32 channels go global -> registers -> Vs as [patch pixel][8-channel group]
    // [kh][tile][4], the untransformed weights (behind the U images in `wgt`, already in LDS order [group][kh][row][4]) by LDS-DMA into the
    // two U buffers.  Barriers: E1 after the store (Vs and the weights of this slab published), E2 after the slab's MFMAs (both dead).
    const int nextra = (p.ec0 + p.ec1) / 32;
    if (nextra > 0) {
        const float* wsk = p.b + (size_t)p.ntiles * nslabs * WINO_IMG + (size_t)nt * nextra * 2048 + tid * 4;
        const int e_chunk = tid & 7;                   // channels 4 e_chunk .. + 3 of the slab: group e_chunk >> 1, kh = e_chunk & 1
        int e_lds[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int lp = (tid >> 3) + 32 * j;        // pixel of the tile
            const int yl = lp / p.W, x = lp - yl * p.W;
            const int ph = (yl & 1) * 2 + (x & 1), t = (yl >> 1) * Wt + (x >> 1);
            e_lds[j] = (((ph * 4 + (e_chunk >> 1)) * 2 + (e_chunk & 1)) * 64 + t) * 4;
        }
        f32x4 ereg[8];
        auto e_load = [&](int es) {
            const int c = es * 32;
            const bool first = c < p.ec0;
            const float* src = (first ? p.e0 + c : p.e1 + (c - p.ec0)) + e_chunk * 4;
            const int ld = first ? p.elda0 : p.elda1;
#pragma unroll
            for (int j = 0; j < 8; ++j) ereg[j] = *reinterpret_cast<const f32x4*>(src + (size_t)(m0 + (tid >> 3) + 32 * j) * ld);
        };
        auto w_dma = [&](int es, int buf) {
            DS_RACE_SKEW(wave);
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                float* dst = Us + buf * WINO_IMG + (i * 256 + wave * 64) * 4;
                typedef const __attribute__((address_space(1))) void* gptr_t;
                typedef __attribute__((address_space(3))) void* lptr_t;
                __builtin_amdgcn_global_load_lds((gptr_t)(wsk + (size_t)es * 2048 + i * 1024), (lptr_t)(dst), 16, 0, 0);
            }
        };
        e_load(0);
        w_dma(0, 0);
        for (int es = 0; es < nextra; ++es) {
            DS_RACE_SKEW(wave);
#pragma unroll
            for (int j = 0; j < 8; ++j) *reinterpret_cast<f32x4*>(Vs + e_lds[j]) = ereg[j];
            DS_WINO_WAIT_VM0();
            __syncthreads();                           // E1
            if (es + 1 < nextra) { e_load(es + 1); w_dma(es + 1, (es + 1) & 1); }
            const float* wb = Us + (es & 1) * WINO_IMG;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 fa[4];
                const f32x4 fb = *reinterpret_cast<const f32x4*>(wb + g * WINO_POS + b_off);
#pragma unroll
                for (int ph = 0; ph < 4; ++ph) fa[ph] = *reinterpret_cast<const f32x4*>(Vs + (ph * 4 + g) * WINO_POS + a_off);
#pragma unroll
                for (int r = 0; r < 4; ++r)
#pragma unroll
                    for (int ph = 0; ph < 4; ++ph) Y[ph] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[ph][r], fb[r], Y[ph], 0, 0, 0);
            }
            __syncthreads();                           // E2
        }
    }

    // ---- the fused epilogue, one patch pixel (a, b) at a time ----------------------------------------------------------------------------
    float* stage = smem + wave * 32 * WINO_EPI_LD;     // wave-private rows; every LDS buffer died at the last barrier C
    const int c4 = (lane & 7) * 4;
    const int col = n0 + wc * 32 + c4;
    f32x4 cb = {0.f, 0.f, 0.f, 0.f}, cvu = {0.f, 0.f, 0.f, 0.f};
    if (p.colbias) cb = *reinterpret_cast<const f32x4*>(p.colbias + col);
    if (p.cbias) cvu = *reinterpret_cast<const f32x4*>(p.cbias + (size_t)(p.cbias_bcast ? 0 : img0) * p.cbias_ld + col);
    const float acc_scale = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, p.acc_scale)));
    const float scale = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, p.scale)));
    int e_row[4];                                      // output row of (pass, patch pixel (0, 0)) of this lane
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
        const int tl = wr * 32 + pass * 8 + (lane >> 3);
        const int ty = tl / Wt, tx = tl - ty * Wt;
        e_row[pass] = m0 + 2 * ty * p.W + 2 * tx;
    }
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        f32x4 st_s = {0.f, 0.f, 0.f, 0.f}, st_q = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const f32x16 y = Y[a * 2 + b];
            f32x4 rv[4];
            if (p.res) {
#pragma unroll
                for (int pass = 0; pass < 4; ++pass)
                    rv[pass] = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p.res + (size_t)(e_row[pass] + a * p.W + b) * p.res_ld + col));
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) stage[((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * WINO_EPI_LD + (lane & 31)] = y[r];
#pragma unroll
            for (int pass = 0; pass < 4; ++pass) {
                f32x4 v = *reinterpret_cast<const f32x4*>(stage + (pass * 8 + (lane >> 3)) * WINO_EPI_LD + c4);
                v *= acc_scale;
                v += cb;
                if (p.cbias) v += cvu;
                if (p.res) v += rv[pass];
                v *= scale;
                if (p.act == DS_ACT_SILU) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = ds_silu(v[q]);
                }
                __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(p.out + (size_t)(e_row[pass] + a * p.W + b) * p.ldo + col));
                st_s += v; st_q += v * v;
            }
        }
        if (p.stats) {
            // column sums of the 64 pixels of patch row a of this wave's 32 tiles: the 8 lane groups (lane >> 3) hold disjoint rows
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                st_s[q] += __shfl_xor(st_s[q], 8); st_s[q] += __shfl_xor(st_s[q], 16); st_s[q] += __shfl_xor(st_s[q], 32);
                st_q[q] += __shfl_xor(st_q[q], 8); st_q[q] += __shfl_xor(st_q[q], 16); st_q[q] += __shfl_xor(st_q[q], 32);
            }
            if (lane < 8) {
                float* sp = p.stats + (size_t)((m0 >> 6) + wr * 2 + a) * 2 * p.N + col;
                *reinterpret_cast<f32x4*>(sp) = st_s;
                *reinterpret_cast<f32x4*>(sp + p.N) = st_q;
            }
        }
    }
}

template <int VAR>
int launch_wino(KParams& p, hipStream_t stream) {
    const int smem = (3 * WINO_IMG + p.NP * WINO_K) * (int)sizeof(float);
    DS_ENSURE_DYN_LDS((&conv3x3_wino_kernel<VAR>), 128 * 1024);
    hipLaunchKernelGGL((conv3x3_wino_kernel<VAR>), dim3(grid_1d(p.mtiles, p.ntiles)), dim3(256), smem, stream, p);
    DS_CHECK_LAUNCH();
    return DS_OK;
}

}  // namespace

// The layer as the kernel above takes it: one image per 256-pixel M tile with an even number of rows (16-, 32- and 64-column images),
// whole 64-column tiles, the vector epilogue, no split-K.
bool conv3x3_wino_applicable(const KParams& p) {
    if (p.taps != 9 || p.stride != 1 || p.splits != 1 || (p.ec0 & 31) || (p.ec1 & 31)) return false;
    if ((p.H & 1) || (p.W & 1) || p.W < 4 || p.W > 64 || p.HW % 256 || 256 % p.W || ((256 / p.W) & 1)) return false;
    if ((p.N & 63) || (p.c0 % WINO_K) || (p.c1 % WINO_K) || !p.vec_ok || p.out_planar || p.out_f16 || p.res_f16 || p.rowbias) return false;
    if (p.act != DS_ACT_NONE && p.act != DS_ACT_SILU) return false;
    const int np = (256 / p.W + 2) * (p.W + 2);
    if (np * 2 > WINO_NSH * 256 || (3 * WINO_IMG + np * WINO_K) * (int)sizeof(float) > 128 * 1024) return false;
    return p.M % 256 == 0;
}

int launch_conv3x3_wino(KParams& p, hipStream_t stream) {
    if (!conv3x3_wino_applicable(p)) return DS_E_SHAPE;
    p.TH = 256 / p.W; p.nimg = 1; p.HP = p.TH + 2; p.WP = p.W + 2; p.NP = p.HP * p.WP;
    p.mtiles = p.M / 256; p.ntiles = p.N / 64; p.n_begin = 0;
#ifdef DS_CONV_ABLATIONS
    if (p.t_variant & 0x10000) {                       // timing ablations (wrong results on purpose)
        switch (p.t_variant & 31) {
            case 2: return launch_wino<2>(p, stream);
            case 4: return launch_wino<4>(p, stream);
            case 8: return launch_wino<8>(p, stream);
            case 16: return launch_wino<16>(p, stream);
            case 28: return launch_wino<28>(p, stream);
            default: break;
        }
    }
#endif
    return launch_wino<0>(p, stream);
}

}  // namespace igemm
