// Trajectory analysis (diff-analyzer-main: main_extend.ipynb, main_mp.ipynb) on the fp64 matrix pipe.
//
// dsm_traj_gram: for every sample b of a stacked fp32 sampling trajectory traj [n_pts][batch][per], the Gram matrix of the trajectory's points
// taken relative to its end point,
//     gram[b][t][s] = sum_e (x[t,b,e] - x[n_pts-1,b,e]) (x[s,b,e] - x[n_pts-1,b,e])          [n_pts][n_pts] fp64,
// from which the 3-D projection of the notebook (chord direction + the two leading principal components of the rest) follows on the host
// with n_pts x n_pts work (analyzer.py) -- no per x per projector, no QR of a per x per matrix.  PC1 and PC2 carry 1e-4 and 1e-6 of the
// chord's energy and come out of the difference G - g0 g0^T / G00, so the Gram matrix has to be fp64: the differences are formed in fp64
// (exact from fp32 operands) when a tile is staged, products and sums run on v_mfma_f64_16x16x4_f64.
//
// Tile: as prdc.hip -- a 256-thread workgroup computes one 128 x 128 tile of one sample's matrix, four waves of 64 x 64 = 4 x 4 MFMA blocks
// (128 accumulator VGPRs); a lane's operands are y[i0 + (l & 15)][k0 + (l >> 4)] (A) and y[j0 + (l & 15)][k0 + (l >> 4)] (B).  Both row bands
// are staged 16 features at a time as fp64 in LDS, [128 rows][16 + 2] doubles per operand: with the 18-double pitch the 16 rows x 2 features of
// a ds_read_b64 lane half fall on 32 different bank pairs and the 16 consecutive doubles a 16-lane group writes cover the write banks once.
// Loads are coalesced along the row (16 lanes = 64 contiguous bytes of one trajectory point), unconditional from clamped addresses and zeroed
// by a select when staged; the end point's 16 features are one more load per thread.  The next 16 features are requested before the 64 MFMAs
// of the current ones.  Only tiles on or below the diagonal are computed (grid.y walks them), and only elements with s <= t leave the
// workgroup: each is stored to [t][s] and to [s][t], so the matrix is symmetric bit for bit.
//
// Split: a trajectory of n_pts <= 128 points is ONE tile per sample, so the contraction over `per` is split over grid.x: split q of a tile takes
// the 16-feature chunks [q * chunks / splits, (q + 1) * chunks / splits), writes its partial tile to the workspace, and traj_reduce_kernel adds the
// partials in ascending q.  splits = clamp(32 / lower tiles, 1, chunks / 8) -- a function of (n_pts, per) alone, at least 128 features per
// workgroup, no split from 6 tile rows (n_pts > 640) on.  Neither the tile walk nor the split depends on batch, b0 or nb, and a sample's
// workgroups read that sample's rows only: its matrix is the same bits in any batch and any [b0, b0 + nb) window, and from run to run (no atomics).
//
// By instruction count a chunk is 32 + 16 ds_read_b64 and 17 global dword loads per lane for 64 MFMAs (4 096 matrix cycles) per wave; a trajectory
// of 21 points fills 21 of a tile's 128 rows, so there the matrix pipe works at 3 % of its rows and the kernel should be bound by staging.
// These are ESTIMATES; what was measured is in DESIGN.md section 4 and profiles/analyzer_bench.txt.  226 VGPRs without scratch under
// __launch_bounds__(256, 2): two workgroups per CU cover each other's two barriers per chunk (one per CU: 132 + 128 registers, 20 % slower).
//
// dsm_row_sqdist: out[r] = sum_e (a[r,e] - b[r,e])^2 (b may be NULL: sum a^2), fp64 differences and sums, one workgroup per row: thread i adds
// elements i, i + 256, ... in order, then the 256 sums are added pairwise in a fixed tree.
#include "../ds_common.h"
#include "ds_metrics.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int TM = 128;                 // rows / columns per tile
constexpr int KC = 16;                  // features per staged chunk
constexpr int KP = KC + 2;              // LDS row pitch in doubles
constexpr int TARGET_TILES = 32;        // workgroups per sample the split aims at
constexpr int MIN_CHUNKS = 8;           // fewest chunks (of 16 features) a split takes
constexpr int MAX_PTS = 32768;          // 256 tile rows: 32 896 lower tiles fit grid.y
constexpr int MAX_NB = 65535;           // grid.z

inline int tile_rows(int n_pts) { return (n_pts + TM - 1) / TM; }
inline int lower_tiles(int n_pts) { const int nt = tile_rows(n_pts); return nt * (nt + 1) / 2; }

inline int splits_for(int n_pts, long long per) {
    const long long chunks = (per + KC - 1) / KC;
    long long s = TARGET_TILES / lower_tiles(n_pts);
    if (s > chunks / MIN_CHUNKS) s = chunks / MIN_CHUNKS;
    return s < 1 ? 1 : (int)s;
}

// dst: the sample's [n_pts][n_pts] matrix (mirror: both triangles are written) or the [n_pts][n_pts] partial of (sample, split) (lower only)
__global__ void __launch_bounds__(256, 2) traj_gram_kernel(const float* __restrict__ traj, int n_pts, int batch, long long per, int b0,
                                                        double* __restrict__ dst_base, int mirror) {
    __shared__ double tile[2][TM][KP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = (wave >> 1) * 64, wj = (wave & 1) * 64;
    const int lc = lane & 15, lk = lane >> 4;
    const int sk = tid & (KC - 1), sr = tid >> 4;                 // staging: feature, first row (rows sr, sr + 16, ...)
    int ti = 0;                                                   // blockIdx.y = ti (ti + 1) / 2 + tj, tj <= ti
    while ((ti + 1) * (ti + 2) / 2 <= (int)blockIdx.y) ++ti;
    const int tj = (int)blockIdx.y - ti * (ti + 1) / 2;
    const int i0 = ti * TM, j0 = tj * TM;
    const int splits = (int)gridDim.x, q = (int)blockIdx.x, bl = (int)blockIdx.z;
    const long long chunks = (per + KC - 1) / KC;
    const long long kbeg = (q * chunks / splits) * KC;
    const long long kend = min(((q + 1) * chunks / splits) * KC, per);
    const float* xs = traj + (size_t)(b0 + bl) * per;             // point t of this sample at xs + t * pitch
    const size_t pitch = (size_t)batch * per;
    const float* xl = xs + (size_t)(n_pts - 1) * pitch;
    float pa[TM / 16], pb[TM / 16], pl;
    auto request = [&](long long k0) {
        const long long kc = min(k0 + sk, per - 1);
        pl = xl[kc];
#pragma unroll
        for (int u = 0; u < TM / 16; ++u) {
            pa[u] = xs[(size_t)min(i0 + sr + 16 * u, n_pts - 1) * pitch + kc];
            pb[u] = xs[(size_t)min(j0 + sr + 16 * u, n_pts - 1) * pitch + kc];
        }
    };
    f64x4 acc[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = f64x4{0.0, 0.0, 0.0, 0.0};
    const double* ta = &tile[0][0][0];
    const double* tb = &tile[1][0][0];
    request(kbeg);
    for (long long k0 = kbeg; k0 < kend; k0 += KC) {
        __syncthreads();                                        // the previous chunk's reads are done
        const bool kv = k0 + sk < kend;
        const double last = (double)pl;
#pragma unroll
        for (int u = 0; u < TM / 16; ++u) {
            tile[0][sr + 16 * u][sk] = (kv && i0 + sr + 16 * u < n_pts) ? (double)pa[u] - last : 0.0;
            tile[1][sr + 16 * u][sk] = (kv && j0 + sr + 16 * u < n_pts) ? (double)pb[u] - last : 0.0;
        }
        __syncthreads();
        if (k0 + KC < kend) request(k0 + KC);                    // in flight under this chunk's MFMAs
#pragma unroll
        for (int ks = 0; ks < KC / 4; ++ks) {
            double a[4], b[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) a[m] = ta[(wi + m * 16 + lc) * KP + ks * 4 + lk];
#pragma unroll
            for (int n = 0; n < 4; ++n) b[n] = tb[(wj + n * 16 + lc) * KP + ks * 4 + lk];
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int n = 0; n < 4; ++n) acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], b[n], acc[m][n], 0, 0, 0);
        }
    }
    double* dst = dst_base + ((size_t)bl * splits + q) * ((size_t)n_pts * n_pts);
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = i0 + wi + m * 16 + lk + 4 * r;
#pragma unroll
            for (int n = 0; n < 4; ++n) {
                const int col = j0 + wj + n * 16 + lc;
                if (row < n_pts && col <= row) {                  // col <= row < n_pts
                    dst[(size_t)row * n_pts + col] = acc[m][n][r];
                    if (mirror) dst[(size_t)col * n_pts + row] = acc[m][n][r];
                }
            }
        }
}

// gram[bl][t][s] = gram[bl][s][t] = partial[bl][0][t][s] + partial[bl][1][t][s] + ... for s <= t
__global__ void __launch_bounds__(256) traj_reduce_kernel(const double* __restrict__ partial, int n_pts, int splits, long long total,
                                                          double* __restrict__ gram) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const long long nn = (long long)n_pts * n_pts;
    const long long bl = e / nn, rem = e - bl * nn;
    const int t = (int)(rem / n_pts), s = (int)(rem - (long long)t * n_pts);
    if (s > t) return;
    const double* src = partial + (size_t)bl * splits * nn + rem;
    double v = src[0];
    for (int q = 1; q < splits; ++q) v += src[(size_t)q * nn];
    double* g = gram + (size_t)bl * nn;
    g[rem] = v;
    g[(size_t)s * n_pts + t] = v;
}

__global__ void __launch_bounds__(256) row_sqdist_kernel(const float* __restrict__ a, const float* __restrict__ b, long long per,
                                                         double* __restrict__ out) {
    __shared__ double sh[256];
    const size_t base = (size_t)blockIdx.x * per;
    double acc = 0.0;
    for (long long e = threadIdx.x; e < per; e += 256) {
        const double d = b ? (double)a[base + e] - (double)b[base + e] : (double)a[base + e];
        acc = __builtin_fma(d, d, acc);
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = sh[0];
}

long long gram_bytes(int n_pts, long long per, int nb) {
    const int s = splits_for(n_pts, per);
    return s == 1 ? 0 : (long long)nb * s * n_pts * n_pts * (long long)sizeof(double);
}

}  // namespace

extern "C" int dsm_traj_gram_splits(int n_pts, long long per) {
    if (n_pts < 2 || per < 1) return DS_E_ARG;
    if (n_pts > MAX_PTS) return DS_E_SHAPE;
    return splits_for(n_pts, per);
}

extern "C" long long dsm_traj_gram_workspace_bytes(int n_pts, long long per, int nb) {
    if (n_pts < 2 || per < 1 || nb < 1) return DS_E_ARG;
    if (n_pts > MAX_PTS || nb > MAX_NB) return DS_E_SHAPE;
    return gram_bytes(n_pts, per, nb);
}

extern "C" int dsm_traj_gram(const float* traj, int n_pts, int batch, long long per, int b0, int nb, double* gram, void* workspace,
                             long long workspace_bytes, void* stream) {
    if (!traj || !gram || n_pts < 2 || batch < 1 || per < 1 || b0 < 0 || nb < 1 || (long long)b0 + nb > batch) return DS_E_ARG;
    if (n_pts > MAX_PTS || nb > MAX_NB) return DS_E_SHAPE;
    if (((long long)nb * n_pts * n_pts + 255) / 256 > 0x7fffffffll) return DS_E_SHAPE;
    const long long need = gram_bytes(n_pts, per, nb);
    if (need > 0 && (!workspace || workspace_bytes < need)) return DS_E_ARG;
    if (need > 0 && (reinterpret_cast<uintptr_t>(workspace) & 7u)) return DS_E_ALIGN;
    (void)hipGetLastError();                                    // only now: a rejected call has not touched the runtime
    const int splits = splits_for(n_pts, per);
    const dim3 grid((unsigned)splits, (unsigned)lower_tiles(n_pts), (unsigned)nb);
    hipStream_t s = (hipStream_t)stream;
    if (splits == 1) {
        hipLaunchKernelGGL(traj_gram_kernel, grid, dim3(256), 0, s, traj, n_pts, batch, per, b0, gram, 1);
        DS_CHECK_LAUNCH();
        return DS_OK;
    }
    double* partial = reinterpret_cast<double*>(workspace);     // [nb][splits][n_pts][n_pts], tiles on and below the diagonal written
    hipLaunchKernelGGL(traj_gram_kernel, grid, dim3(256), 0, s, traj, n_pts, batch, per, b0, partial, 0);
    DS_CHECK_LAUNCH();
    const long long total = (long long)nb * n_pts * n_pts;
    hipLaunchKernelGGL(traj_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, partial, n_pts, splits, total, gram);
    DS_CHECK_LAUNCH();
    return DS_OK;
}

extern "C" int dsm_row_sqdist(const float* a, const float* b_or_null, long long rows, long long per, double* out, void* stream) {
    if (!a || !out || rows < 1 || per < 1) return DS_E_ARG;
    if (rows > 0x7fffffffll) return DS_E_SHAPE;
    (void)hipGetLastError();
    hipLaunchKernelGGL(row_sqdist_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, a, b_or_null, per, out);
    DS_CHECK_LAUNCH();
    return DS_OK;
}
