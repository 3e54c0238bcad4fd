// Precision / recall / density / coverage (sfd-main/prdc.py) on the fp64 matrix pipe: squared Euclidean distances of two feature sets in
// sklearn's expanded form
//     d2(i, j) = max(|x_i|^2 + |y_j|^2 - 2 x_i . y_j, 0)
// consumed tile by tile -- the k-nearest-neighbour radii of a set (dsm_knn_radii_sq) and the counts / minima / maxima of the real x fake
// comparison (dsm_prdc_cross) -- so that no n x n matrix ever reaches memory.  n = 10 000, dim = 2048: 3 x 0.41 TFLOP of fp64 against
// 3 x 800 MB that the reference writes, sorts and reads back on the CPU.
//
// Tile: one 256-thread workgroup owns a 128-row band of x and walks a contiguous range of 128-column tiles of y (the columns of a band
// are split over several workgroups: 10 000 rows are only 79 bands for 256 CUs); four waves of 64 x 64 = 4 x 4 blocks of
// v_mfma_f64_16x16x4_f64 (128 accumulator VGPRs), as in fid.hip.  Here the contraction runs along the feature ROWS, so a lane's operands
// are x[i0 + (l & 15)][k0 + (l >> 4)] (A) and y[j0 + (l & 15)][k0 + (l >> 4)] (B).  Both bands are staged 16 features at a time as fp64
// in LDS, [128 rows][16 + 2] doubles per operand: with the 18-double pitch the 16 rows x 2 features of a ds_read_b64 lane half fall on 32
// different bank pairs (18 r mod 32 is even and distinct for r = 0 .. 15), and the 16 consecutive doubles of one row that a 16-lane group
// writes cover the 32 write banks once -- reads and writes are conflict free.  Loads are coalesced along the row (16 lanes = 64 / 128
// contiguous bytes), unconditional from clamped addresses and zeroed by a select when staged (fid.hip: a predicated load costs a branch
// and a full vmcnt(0) each); the next 16 features are requested into registers before the 64 MFMAs of the current ones.
// |x_i|^2 and |y_j|^2 come from the same staged tiles (threads 0 - 127 the x rows, 128 - 255 the y rows; features in a fixed order per
// row position), so a row's norm is the same number in every workgroup that touches it.
//
// Per 16 features a wave issues 32 + 16 ds_read_b64 for 64 MFMAs (4 096 matrix cycles), and the epilogue of a tile is 256 distances per
// lane: by instruction count the loop should be bound by the matrix pipe.  That is an ESTIMATE; what was measured, and what limits it, is in
// DESIGN.md section 4 and profiles/prdc_bench.txt.
#include <type_traits>

#include "../ds_common.h"
#include "ds_metrics.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int TM = 128;                 // rows / columns per tile
constexpr int KC = 16;                  // features per staged chunk
constexpr int KP = KC + 2;              // LDS row pitch in doubles
constexpr int LMAX = DSM_MAX_K + 1;     // longest per-row list of smallest distances
constexpr int MAX_ROWS = 65535 * TM;     // one 128-row band per blockIdx.y
constexpr int TARGET_WG = 512;          // most workgroups a split launch has (two rounds of 256 CUs): fixes the column split as a function of the sizes only

struct Stage {
    double tile[2][TM][KP];             // [operand: 0 = x rows, 1 = y rows][row][feature]
    double nrm[2][TM];                  // squared norms of the staged rows, complete after the last chunk
};

__host__ __device__ inline int ceil_div(int a, int b) { return (a + b - 1) / b; }

inline int splits_for(int n_rows, int n_cols) {
    const int bands = ceil_div(n_rows, TM), tiles = ceil_div(n_cols, TM);
    const int s = bands >= TARGET_WG ? 1 : TARGET_WG / bands;     // rounded DOWN: a launch stays within two rounds of the 256 CUs (one workgroup
    return s < tiles ? s : tiles;                                 // per CU at this register count); 79 bands x 7 = 553 took a third round at 16 % fill
}

__device__ __forceinline__ double d_inf() { return __longlong_as_double(0x7ff0000000000000ll); }

// acc[m][n][r] = x[i0 + wi + 16 m + (lane >> 4) + 4 r] . y[j0 + wj + 16 n + (lane & 15)] over all features, and st.nrm = the squared norms
// of the 128 + 128 rows.  Rows at or beyond nx / ny and features beyond dim are staged as zeros.  Ends with a barrier: st.nrm is readable.
template <bool XF64, bool YF64>
__device__ __forceinline__ void tile_dots(Stage& st, const void* __restrict__ x, int ldx, int nx, int i0, const void* __restrict__ y, int ldy,
                                          int ny, int j0, int dim, f64x4 (&acc)[4][4]) {
    typedef typename std::conditional<XF64, double, float>::type xraw_t;
    typedef typename std::conditional<YF64, double, float>::type yraw_t;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = (wave >> 1) * 64, wj = (wave & 1) * 64;
    const int lc = lane & 15, lk = lane >> 4;
    const int sk = tid & (KC - 1), sr = tid >> 4;                 // staging: feature, first row (rows sr, sr + 16, ...)
    const xraw_t* xs = reinterpret_cast<const xraw_t*>(x);
    const yraw_t* ys = reinterpret_cast<const yraw_t*>(y);
    xraw_t px[TM / 16];
    yraw_t py[TM / 16];
    auto request = [&](int k0) {
        const int kc = min(k0 + sk, dim - 1);
#pragma unroll
        for (int u = 0; u < TM / 16; ++u) {
            px[u] = xs[(size_t)min(i0 + sr + 16 * u, nx - 1) * ldx + kc];
            py[u] = ys[(size_t)min(j0 + sr + 16 * u, ny - 1) * ldy + kc];
        }
    };
    const int no = tid >> 7, nr = tid & (TM - 1), nrot = (nr >> 4) & 1;     // norms: operand, row, first feature (rows r and r + 16 share a bank pair)
    double nsum = 0.0;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = f64x4{0.0, 0.0, 0.0, 0.0};
    const double* ta = &st.tile[0][0][0];
    const double* tb = &st.tile[1][0][0];
    request(0);
    for (int k0 = 0; k0 < dim; k0 += KC) {
        __syncthreads();                                        // the previous chunk's (and the previous tile's epilogue's) reads are done
        const bool kv = k0 + sk < dim;
#pragma unroll
        for (int u = 0; u < TM / 16; ++u) {
            st.tile[0][sr + 16 * u][sk] = (kv && i0 + sr + 16 * u < nx) ? (double)px[u] : 0.0;
            st.tile[1][sr + 16 * u][sk] = (kv && j0 + sr + 16 * u < ny) ? (double)py[u] : 0.0;
        }
        __syncthreads();
        if (k0 + KC < dim) request(k0 + KC);                     // in flight under this chunk's MFMAs
#pragma unroll
        for (int q = 0; q < KC; ++q) {
            const double v = st.tile[no][nr][(q + nrot) & (KC - 1)];
            nsum = __builtin_fma(v, v, nsum);
        }
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
    st.nrm[no][nr] = nsum;
    __syncthreads();
}

// max that keeps a NaN from either side, as numpy's does: radius 0 over distance 0 makes a sample's realism NaN in the reference
__device__ __forceinline__ double nan_max(double a, double b) { return (b > a || b != b) ? b : a; }

__device__ __forceinline__ double dist_sq(double xn, double yn, double dot) { return fmax(xn + yn - 2.0 * dot, 0.0); }

// Sorted insertion of c into the ascending list l[0 .. len): the largest entry drops out.  One lane per list at a time.
typedef volatile __attribute__((address_space(3))) double* lds_list_t;       // LDS address space spelled out: volatile accesses stay ds_read / ds_write

__device__ __forceinline__ void list_insert(lds_list_t l, int len, double c) {
    int p = len - 1;
    while (p > 0) {
        const double q = l[p - 1];
        if (!(q > c)) break;
        l[p] = q;
        --p;
    }
    l[p] = c;
}

// best[] (ascending, LMAX entries) takes c if it is among the LMAX smallest seen; static indices only (registers).
__device__ __forceinline__ void best_take(double (&best)[LMAX], double c) {
    if (!(c < best[LMAX - 1])) return;
    best[LMAX - 1] = c;
#pragma unroll
    for (int p = LMAX - 1; p > 0; --p) {
        const double lo = fmin(best[p - 1], best[p]), hi = fmax(best[p - 1], best[p]);
        best[p - 1] = lo;
        best[p] = hi;
    }
}

// ---- k-nearest-neighbour radii.  Each (row, column half of the tile) keeps the kl = k + 1 smallest squared distances it has seen as a
// sorted list in LDS, owned by ONE wave (rows wi .. wi + 63, columns wj .. wj + 63 of every tile): its last entry is the row's threshold,
// and only candidates below it take the serial insert path -- all 64 of a row in the first tile, a handful per row after a few tiles.  The
// 16 lanes that hold a row's candidates insert one at a time (lowest lane first); the four 16-lane groups of the wave work on four
// different rows.  The result is the kl smallest values as a multiset: it does not depend on the order of insertion.
template <bool F64>
__global__ void __launch_bounds__(256) knn_kernel(const void* __restrict__ x, int ld, int n, int dim, int kl, double* __restrict__ partial) {
    __shared__ Stage st;
    __shared__ double lists[2][TM][LMAX];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = (wave >> 1) * 64, wj = (wave & 1) * 64, half = wave & 1;
    const int lc = lane & 15, lk = lane >> 4;
    const int i0 = blockIdx.y * TM, tiles = ceil_div(n, TM);
    const int t0 = (int)((long long)blockIdx.x * tiles / gridDim.x), t1 = (int)((long long)(blockIdx.x + 1) * tiles / gridDim.x);
    const double inf = d_inf();
    for (int e = tid; e < 2 * TM * LMAX; e += 256) (&lists[0][0][0])[e] = inf;
    __syncthreads();
    f64x4 acc[4][4];
    for (int t = t0; t < t1; ++t) {
        const int j0 = t * TM;
        tile_dots<F64, F64>(st, x, ld, n, i0, x, ld, n, j0, dim, acc);
        double yn[4];
        int jg[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            jg[c] = j0 + wj + c * 16 + lc;
            yn[c] = st.nrm[1][wj + c * 16 + lc];
        }
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = wi + m * 16 + lk + 4 * r, ig = i0 + row;
                const double xn = st.nrm[0][row];
                const lds_list_t l = (lds_list_t)&lists[half][row][0];
                double v[4], vmin = inf;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    double d = dist_sq(xn, yn[c], acc[m][c][r]);
                    d = jg[c] == ig ? 0.0 : d;                  // sklearn zeroes the diagonal of a self-distance matrix
                    d = jg[c] < n ? d : inf;
                    v[c] = d;
                    vmin = fmin(vmin, d);
                }
                if (__builtin_amdgcn_ballot_w64(vmin < l[kl - 1]) == 0) continue;       // wave-uniform: nobody has a candidate
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    double cand = v[c];
                    for (;;) {
                        const bool want = cand < l[kl - 1];
                        const unsigned long long b = __builtin_amdgcn_ballot_w64(want);
                        if (b == 0) break;                      // wave-uniform
                        const unsigned grp = (unsigned)(b >> (lk * 16)) & 0xffffu;
                        if (want && lc == __builtin_ctz(grp)) { // the row's first pending lane; LDS serves a wave's accesses in order
                            list_insert(l, kl, cand);
                            cand = inf;
                        }
                    }
                }
            }
    }
    __syncthreads();
    if (tid < TM && i0 + tid < n) {                             // the two column halves of the row -> the split's kl smallest, ascending
        double best[LMAX];
#pragma unroll
        for (int p = 0; p < LMAX; ++p) best[p] = inf;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int p = 0; p < LMAX; ++p) best_take(best, lists[h][tid][p]);
        double* dst = partial + ((size_t)blockIdx.x * n + i0 + tid) * kl;
#pragma unroll
        for (int p = 0; p < LMAX; ++p)
            if (p < kl) dst[p] = best[p];
    }
}

__global__ void __launch_bounds__(256) knn_merge_kernel(const double* __restrict__ partial, int n, int kl, int splits, double* __restrict__ radii_sq) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double best[LMAX];
#pragma unroll
    for (int p = 0; p < LMAX; ++p) best[p] = d_inf();
    for (int s = 0; s < splits; ++s) {
        const double* src = partial + ((size_t)s * n + i) * kl;
        for (int p = 0; p < kl; ++p) best_take(best, src[p]);
    }
    double out = best[0];
#pragma unroll
    for (int p = 1; p < LMAX; ++p) out = p == kl - 1 ? best[p] : out;
    radii_sq[i] = out;
}

// ---- real x fake.  Row statistics (hits, minimum) stay in registers over the workgroup's column tiles and leave as one partial per
// column split; column statistics (counts, realism maximum) are complete per (band, tile) and leave as one partial per band.  Integer
// sums, fp64 min and max: every reduction is exact in any order, and the partials are combined in a fixed one by cross_reduce_kernel.
template <bool RF64, bool FF64, bool REALISM>
__global__ void __launch_bounds__(256) cross_kernel(const void* __restrict__ real, int ld_r, int n_real, const void* __restrict__ fake, int ld_f,
                                                    int n_fake, int dim, const double* __restrict__ rr, const double* __restrict__ rf,
                                                    const unsigned char* __restrict__ mask, double* __restrict__ min_part,
                                                    double* __restrict__ rls_part, int* __restrict__ hit_part, int* __restrict__ cnt_part) {
    __shared__ Stage st;
    __shared__ int colcnt[TM];
    __shared__ double colmax[2][TM];
    __shared__ double rowmin[2][TM];
    __shared__ int rowhit[2][TM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = (wave >> 1) * 64, wj = (wave & 1) * 64;
    const int lc = lane & 15, lk = lane >> 4;
    const int i0 = blockIdx.y * TM, tiles = ceil_div(n_fake, TM);
    const int t0 = (int)((long long)blockIdx.x * tiles / gridDim.x), t1 = (int)((long long)(blockIdx.x + 1) * tiles / gridDim.x);
    const double inf = d_inf();
    double rmin[4][4];
    int rhit[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            rmin[m][r] = inf;
            rhit[m][r] = 0;
        }
    f64x4 acc[4][4];
    for (int t = t0; t < t1; ++t) {
        const int j0 = t * TM;
        if (tid < TM) colcnt[tid] = 0;                          // ordered before the atomics below by the barriers of tile_dots
        tile_dots<RF64, FF64>(st, real, ld_r, n_real, i0, fake, ld_f, n_fake, j0, dim, acc);
        double yn[4], rfj[4], cmax[4];
        int ccnt[4];
        bool jv[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int j = j0 + wj + c * 16 + lc;
            jv[c] = j < n_fake;
            yn[c] = st.nrm[1][wj + c * 16 + lc];
            rfj[c] = jv[c] ? rf[j] : -1.0;                      // a padded column is never hit (d2 >= 0)
            ccnt[c] = 0;
            cmax[c] = -inf;
        }
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = wi + m * 16 + lk + 4 * r, ig = i0 + row;
                const double xn = st.nrm[0][row];
                const double rri = ig < n_real ? rr[ig] : -1.0; // a padded row covers nothing
                bool mk = false;
                if constexpr (REALISM) mk = ig < n_real && mask[min(ig, n_real - 1)] != 0;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const double d = dist_sq(xn, yn[c], acc[m][c][r]);
                    ccnt[c] += d < rri ? 1 : 0;
                    rhit[m][r] += d < rfj[c] ? 1 : 0;
                    rmin[m][r] = fmin(rmin[m][r], jv[c] ? d : inf);
                    if constexpr (REALISM) {
                        if (mk) cmax[c] = nan_max(cmax[c], rri / d);
                    }
                }
            }
#pragma unroll
        for (int c = 0; c < 4; ++c) {                           // columns: over the wave's four row groups, then over the two row halves
            int cc = ccnt[c];
            cc += __shfl_xor(cc, 16);
            cc += __shfl_xor(cc, 32);
            if (lk == 0 && cc != 0) atomicAdd(&colcnt[wj + c * 16 + lc], cc);
            if constexpr (REALISM) {
                double cm = cmax[c];
                cm = nan_max(cm, __shfl_xor(cm, 16));
                cm = nan_max(cm, __shfl_xor(cm, 32));
                if (lk == 0) colmax[wave >> 1][wj + c * 16 + lc] = cm;
            }
        }
        __syncthreads();
        if (tid < TM && j0 + tid < n_fake) {
            cnt_part[(size_t)blockIdx.y * n_fake + j0 + tid] = colcnt[tid];
            if constexpr (REALISM) rls_part[(size_t)blockIdx.y * n_fake + j0 + tid] = nan_max(colmax[0][tid], colmax[1][tid]);
        }
    }
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {                           // rows: over the 16 lanes of the row, then over the two column halves
            double v = rmin[m][r];
            int h = rhit[m][r];
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) {
                v = fmin(v, __shfl_xor(v, o));
                h += __shfl_xor(h, o);
            }
            if (lc == 0) {
                rowmin[wave & 1][wi + m * 16 + lk + 4 * r] = v;
                rowhit[wave & 1][wi + m * 16 + lk + 4 * r] = h;
            }
        }
    __syncthreads();
    if (tid < TM && i0 + tid < n_real) {
        min_part[(size_t)blockIdx.x * n_real + i0 + tid] = fmin(rowmin[0][tid], rowmin[1][tid]);
        hit_part[(size_t)blockIdx.x * n_real + i0 + tid] = rowhit[0][tid] + rowhit[1][tid];
    }
}

__global__ void __launch_bounds__(256) cross_reduce_kernel(int n_real, int n_fake, int splits, int bands, const double* __restrict__ min_part,
                                                           const double* __restrict__ rls_part, const int* __restrict__ hit_part,
                                                           const int* __restrict__ cnt_part, int* __restrict__ fake_count, int* __restrict__ real_hit,
                                                           double* __restrict__ real_min_sq, double* __restrict__ realism_sq) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < n_real) {
        double v = min_part[e];
        int h = hit_part[e];
        for (int s = 1; s < splits; ++s) {
            v = fmin(v, min_part[(size_t)s * n_real + e]);
            h += hit_part[(size_t)s * n_real + e];
        }
        real_min_sq[e] = v;
        real_hit[e] = h;
    }
    if (e < n_fake) {
        int c = cnt_part[e];
        for (int b = 1; b < bands; ++b) c += cnt_part[(size_t)b * n_fake + e];
        fake_count[e] = c;
        if (realism_sq) {
            double v = rls_part[e];
            for (int b = 1; b < bands; ++b) v = nan_max(v, rls_part[(size_t)b * n_fake + e]);
            realism_sq[e] = v;
        }
    }
}

long long knn_bytes(int n, int k) { return (long long)splits_for(n, n) * n * (k + 1) * (long long)sizeof(double); }

long long cross_bytes(int n_real, int n_fake) {
    const long long s = splits_for(n_real, n_fake), b = ceil_div(n_real, TM);
    return (s * n_real + b * n_fake) * (long long)(sizeof(double) + sizeof(int));
}

template <bool RF64, bool FF64>
void launch_cross(bool realism, dim3 grid, hipStream_t stream, const void* real, int ld_r, int n_real, const void* fake, int ld_f, int n_fake, int dim,
                  const double* rr, const double* rf, const unsigned char* mask, double* min_part, double* rls_part, int* hit_part, int* cnt_part) {
    if (realism)
        hipLaunchKernelGGL((cross_kernel<RF64, FF64, true>), grid, dim3(256), 0, stream, real, ld_r, n_real, fake, ld_f, n_fake, dim, rr, rf, mask,
                           min_part, rls_part, hit_part, cnt_part);
    else
        hipLaunchKernelGGL((cross_kernel<RF64, FF64, false>), grid, dim3(256), 0, stream, real, ld_r, n_real, fake, ld_f, n_fake, dim, rr, rf, mask,
                           min_part, rls_part, hit_part, cnt_part);
}

}  // namespace

extern "C" int dsm_version(void) { return DSM_VERSION; }

extern "C" const char* dsm_error_string(int code) {
    switch (code) {
        case DS_OK: return "ok";
        case DS_E_ARG: return "invalid argument";
        case DS_E_ALIGN: return "misaligned pointer or leading dimension";
        case DS_E_SHAPE: return "unsupported shape";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown error";
    }
}

extern "C" int dsm_prdc_splits(int n_rows, int n_cols) {
    if (n_rows < 1 || n_cols < 1) return DS_E_ARG;
    return splits_for(n_rows, n_cols);
}

extern "C" long long dsm_prdc_workspace_bytes(int n_real, int n_fake, int k) {
    if (n_real < 1 || n_fake < 1 || k < 1) return DS_E_ARG;
    long long b = cross_bytes(n_real, n_fake);
    const long long kr = knn_bytes(n_real, k), kf = knn_bytes(n_fake, k);
    b = kr > b ? kr : b;
    return kf > b ? kf : b;
}

extern "C" int dsm_knn_radii_sq(const void* x, int x_f64, int ld, int n, int dim, int k, double* radii_sq, void* workspace, long long workspace_bytes,
                                void* stream) {
    if (!x || !radii_sq || !workspace || dim <= 0 || ld < dim || k < 1 || n < 1 || (long long)k + 1 > n) return DS_E_ARG;
    if (x_f64 != 0 && x_f64 != 1) return DS_E_ARG;
    if (k > DSM_MAX_K || n > MAX_ROWS) return DS_E_SHAPE;
    if (workspace_bytes < knn_bytes(n, k)) return DS_E_ARG;
    if (reinterpret_cast<uintptr_t>(workspace) & 7u) return DS_E_ALIGN;
    (void)hipGetLastError();                                    // only now: a rejected call has not touched the runtime
    const int splits = splits_for(n, n), kl = k + 1;
    double* partial = reinterpret_cast<double*>(workspace);
    const dim3 grid((unsigned)splits, (unsigned)ceil_div(n, TM));
    if (x_f64) hipLaunchKernelGGL(knn_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, ld, n, dim, kl, partial);
    else hipLaunchKernelGGL(knn_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, ld, n, dim, kl, partial);
    DS_CHECK_LAUNCH();
    hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)ceil_div(n, 256)), dim3(256), 0, (hipStream_t)stream, partial, n, kl, splits, radii_sq);
    DS_CHECK_LAUNCH();
    return DS_OK;
}

extern "C" int dsm_prdc_cross(const void* real, int real_f64, int ld_r, int n_real, const void* fake, int fake_f64, int ld_f, int n_fake, int dim,
                              const double* radii_sq_real, const double* radii_sq_fake, int* fake_count, int* real_hit, double* real_min_sq,
                              const unsigned char* realism_mask, double* realism_sq, void* workspace, long long workspace_bytes, void* stream) {
    if (!real || !fake || !radii_sq_real || !radii_sq_fake || !fake_count || !real_hit || !real_min_sq || !workspace) return DS_E_ARG;
    if ((realism_mask == nullptr) != (realism_sq == nullptr)) return DS_E_ARG;
    if (dim <= 0 || ld_r < dim || ld_f < dim || n_real < 1 || n_fake < 1) return DS_E_ARG;
    if ((real_f64 != 0 && real_f64 != 1) || (fake_f64 != 0 && fake_f64 != 1)) return DS_E_ARG;
    if (n_real > MAX_ROWS) return DS_E_SHAPE;
    if (workspace_bytes < cross_bytes(n_real, n_fake)) return DS_E_ARG;
    if (reinterpret_cast<uintptr_t>(workspace) & 7u) return DS_E_ALIGN;
    (void)hipGetLastError();
    const int splits = splits_for(n_real, n_fake), bands = ceil_div(n_real, TM);
    double* min_part = reinterpret_cast<double*>(workspace);                    // [splits][n_real]
    double* rls_part = min_part + (size_t)splits * n_real;                      // [bands][n_fake]
    int* hit_part = reinterpret_cast<int*>(rls_part + (size_t)bands * n_fake);  // [splits][n_real]
    int* cnt_part = hit_part + (size_t)splits * n_real;                         // [bands][n_fake]
    const dim3 grid((unsigned)splits, (unsigned)bands);
    const bool realism = realism_sq != nullptr;
    hipStream_t s = (hipStream_t)stream;
    if (real_f64 && fake_f64) launch_cross<true, true>(realism, grid, s, real, ld_r, n_real, fake, ld_f, n_fake, dim, radii_sq_real, radii_sq_fake, realism_mask, min_part, rls_part, hit_part, cnt_part);
    else if (real_f64) launch_cross<true, false>(realism, grid, s, real, ld_r, n_real, fake, ld_f, n_fake, dim, radii_sq_real, radii_sq_fake, realism_mask, min_part, rls_part, hit_part, cnt_part);
    else if (fake_f64) launch_cross<false, true>(realism, grid, s, real, ld_r, n_real, fake, ld_f, n_fake, dim, radii_sq_real, radii_sq_fake, realism_mask, min_part, rls_part, hit_part, cnt_part);
    else launch_cross<false, false>(realism, grid, s, real, ld_r, n_real, fake, ld_f, n_fake, dim, radii_sq_real, radii_sq_fake, realism_mask, min_part, rls_part, hit_part, cnt_part);
    DS_CHECK_LAUNCH();
    const int m = n_real > n_fake ? n_real : n_fake;
    hipLaunchKernelGGL(cross_reduce_kernel, dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, s, n_real, n_fake, splits, bands, min_part, rls_part,
                       hit_part, cnt_part, fake_count, real_hit, real_min_sq, realism_sq);
    DS_CHECK_LAUNCH();
    return DS_OK;
}
