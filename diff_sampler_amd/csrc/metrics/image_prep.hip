// Image preparation for the CLIP score: the antialiased bicubic resize and the centre crop of the reference transform, to the last bit
// what Pillow's 8-bit resampler (Resample.c) computes -- integer arithmetic once the coefficient tables exist (clip_preprocess.py builds them).
//
//   dsm_resize_crop_u8   n interleaved RGB uint8 images [h][w][3] -> planar uint8 [n][3][size][size]: the window (top, left, size, size) of the
//                        image resized to nh x nw.  Horizontal pass, then vertical; each  acc = 1 << 21; acc += pixel * weight  over the
//                        taps of the output index in int32,  clamp(acc >> 22, 0, 255);  the intermediate is uint8.  A pass whose size does
//                        not change takes the pixel itself (one tap of weight 1 << 22: (2^21 + p 2^22) >> 22 = p).
//
// One workgroup (256 threads) per (image, band of R output rows).  The band needs the source rows first-tap(first row) ... last-tap(last
// row); they pass through LDS in chunks of T rows: global -> S with the widest loads that the base, the pitch and the image stride allow
// (16 / 4 / 1 bytes; the bytes behind the last whole vector of a row singly), only the columns that the cropped window's taps reach; the
// horizontal pass reads S and writes H, planar ([row][channel][column], column pitch a multiple of 4), one thread = one output column of
// four rows, so a weight is loaded once for 12 multiply-adds; the vertical pass reads H a dword (4 columns of one channel) at a time and
// stores packed dwords to the three planes (bytes when size is no multiple of 4).  Multiplies are v_mad_i32_i24: a pixel has 8 bits, a
// weight lies in (-2^23, 2^23) (clip_preprocess.resample_coeffs checks), so the 24-bit product is the 32-bit one.
//
// LDS: S = T rows x (staged bytes of a row rounded up to 16), T = 4 ... 16 with S <= 24 KB (at least 4 rows);  H = (rows of the tallest band)
// x 3 x (size rounded up to 4) <= 40 KB: R is the largest band <= 32 rows whose H fits 28 KB; a band of 4 rows or fewer may take 40 KB.
// At 512 -> 224: T = 8, R = 15 (42 rows of H), 40 512 bytes, three workgroups per CU; at 2048 -> 224: T = 4, R = 3 (55 rows), 61 536 bytes.
//
// The tables are device memory the host cannot inspect: the kernel clamps every first tap and tap count to the rows and columns it
// holds, so a wrong table gives wrong pixels, never an access outside the source or the LDS.
#include <algorithm>
#include <cmath>

#include "../ds_common.h"
#include "ds_metrics.h"

namespace {

constexpr int IP_S_BYTES = 12 * 1024;        // S aims at this, and may take twice as much to hold four rows
constexpr int IP_S_MAX = 24 * 1024;
constexpr int IP_H_BYTES = 28 * 1024;
constexpr int IP_H_MAX = 40 * 1024;
constexpr int IP_BAND_MAX = 32;

struct PrepArgs {
    const unsigned char* src; unsigned char* out;
    const int* hb; const int* hc; const int* vb; const int* vc;
    long long image_stride;
    int pitch, h, w, top, left, size, hk, vk;       // hk / vk == 0: that pass is skipped
    int bands, R, T, cap_rows;                      // rows per band, rows per chunk, rows H holds
    int col_lo, col_hi, byte_lo, srow;              // source columns staged, the first staged byte of a row (vector aligned), S row pitch
    int P;                                          // H column pitch: size rounded up to 4
};

template <int V> struct Vec;
template <> struct Vec<16> { using type = uint4; };
template <> struct Vec<4> { using type = unsigned int; };
template <> struct Vec<1> { using type = unsigned char; };

__device__ __forceinline__ int clamp_u8(int acc) { return min(max(acc >> 22, 0), 255); }

template <int V>
__global__ void __launch_bounds__(256) resize_crop_kernel(const PrepArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ip_smem[];
    unsigned char* S = ip_smem;
    unsigned char* H = ip_smem + a.T * a.srow;
    using vec_t = typename Vec<V>::type;

    const int tid = threadIdx.x;
    const int img = blockIdx.x / a.bands, band = blockIdx.x - img * a.bands;
    const int r0 = band * a.R, rb = min(a.R, a.size - r0);
    const int hrow = 3 * a.P;

    // the source rows of this band
    int row_lo, nrows;
    if (a.vk == 0) {
        row_lo = a.top + r0;
        nrows = rb;
    } else {
        const int first = a.top + r0, last = first + rb - 1;
        row_lo = min(max(a.vb[2 * first], 0), a.h - 1);
        const int hi = min(max(a.vb[2 * last] + a.vb[2 * last + 1], row_lo + 1), a.h);
        nrows = min(hi - row_lo, a.cap_rows);
    }

    const unsigned char* base = a.src + (size_t)img * a.image_stride + a.byte_lo;
    const int span = 3 * a.col_hi - a.byte_lo;          // staged bytes of a row
    const int nvec = span / V, tail = span - nvec * V;

    for (int c0 = 0; c0 < nrows; c0 += a.T) {
        const int tr = min(a.T, nrows - c0);
        __syncthreads();                                 // the previous chunk's S has been read
        for (int i = tid; i < tr * nvec; i += 256) {
            const int j = i / nvec, v = i - j * nvec;
            *reinterpret_cast<vec_t*>(S + j * a.srow + v * V) =
                *reinterpret_cast<const vec_t*>(base + (size_t)(row_lo + c0 + j) * a.pitch + v * V);
        }
        if (V > 1) {
            for (int i = tid; i < tr * tail; i += 256) {
                const int j = i / tail, v = nvec * V + (i - j * tail);
                S[j * a.srow + v] = base[(size_t)(row_lo + c0 + j) * a.pitch + v];
            }
        }
        __syncthreads();

        // horizontal: thread = (group of four rows, output column)
        const int items = ((tr + 3) >> 2) * a.size;
        for (int i = tid; i < items; i += 256) {
            const int g = i / a.size, c = i - g * a.size, col = a.left + c;
            int xmin = col, cnt = 1;
            if (a.hk) { xmin = a.hb[2 * col]; cnt = a.hb[2 * col + 1]; }
            xmin = min(max(xmin, a.col_lo), a.col_hi - 1);
            cnt = min(max(cnt, 0), min(a.hk ? a.hk : 1, a.col_hi - xmin));
            const int* kk = a.hc + (size_t)col * a.hk;
            const unsigned char* s[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) s[j] = S + min(4 * g + j, tr - 1) * a.srow + (3 * xmin - a.byte_lo);
            int acc[4][3];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j][0] = acc[j][1] = acc[j][2] = 1 << 21;
#pragma unroll 4
            for (int k = 0; k < cnt; ++k) {                      // four taps' loads in flight
                const int wgt = a.hk ? kk[k] : (1 << 22);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[j][0] += __mul24((int)s[j][3 * k], wgt);
                    acc[j][1] += __mul24((int)s[j][3 * k + 1], wgt);
                    acc[j][2] += __mul24((int)s[j][3 * k + 2], wgt);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (4 * g + j < tr) {
                    unsigned char* hp = H + (c0 + 4 * g + j) * hrow + c;
                    hp[0] = (unsigned char)clamp_u8(acc[j][0]);
                    hp[a.P] = (unsigned char)clamp_u8(acc[j][1]);
                    hp[2 * a.P] = (unsigned char)clamp_u8(acc[j][2]);
                }
            }
        }
    }
    __syncthreads();

    // vertical: thread = (output row, channel, four columns)
    const int P4 = a.P >> 2, per_row = 3 * P4;
    const bool packed = (a.size & 3) == 0;
    for (int i = tid; i < rb * per_row; i += 256) {
        const int r = i / per_row, rem = i - r * per_row, ch = rem / P4, q = rem - ch * P4;
        const int orow = a.top + r0 + r;
        int xmin = orow, cnt = 1;
        if (a.vk) { xmin = a.vb[2 * orow]; cnt = a.vb[2 * orow + 1]; }
        xmin = min(max(xmin, row_lo), row_lo + nrows - 1);
        cnt = min(max(cnt, 0), min(a.vk ? a.vk : 1, row_lo + nrows - xmin));
        const int* kk = a.vc + (size_t)orow * a.vk;
        const unsigned char* hp = H + (xmin - row_lo) * hrow + ch * a.P + 4 * q;
        int acc0 = 1 << 21, acc1 = 1 << 21, acc2 = 1 << 21, acc3 = 1 << 21;
#pragma unroll 4
        for (int k = 0; k < cnt; ++k) {
            const int wgt = a.vk ? kk[k] : (1 << 22);
            const unsigned int u = *reinterpret_cast<const unsigned int*>(hp + k * hrow);
            acc0 += __mul24((int)(u & 255u), wgt);
            acc1 += __mul24((int)((u >> 8) & 255u), wgt);
            acc2 += __mul24((int)((u >> 16) & 255u), wgt);
            acc3 += __mul24((int)(u >> 24), wgt);
        }
        const unsigned int o = (unsigned)clamp_u8(acc0) | ((unsigned)clamp_u8(acc1) << 8) | ((unsigned)clamp_u8(acc2) << 16) | ((unsigned)clamp_u8(acc3) << 24);
        unsigned char* op = a.out + (((size_t)img * 3 + ch) * a.size + (r0 + r)) * a.size + 4 * q;
        if (packed) {
            *reinterpret_cast<unsigned int*>(op) = o;
        } else {
            for (int j = 0; j < 4; ++j)
                if (4 * q + j < a.size) op[j] = (unsigned char)(o >> (8 * j));
        }
    }
}

// Pillow's tap range of output index i (precompute_coeffs, bicubic support 2): the same double operations in the same order
void tap_range(int in, int out, int i, int* lo, int* hi) {
#pragma clang fp contract(off)
    if (in == out) { *lo = i; *hi = i + 1; return; }
    const double scale = (double)in / (double)out, fscale = scale < 1.0 ? 1.0 : scale, support = 2.0 * fscale;
    const double center = (i + 0.5) * scale;
    int a = (int)(center - support + 0.5), b = (int)(center + support + 0.5);
    *lo = a < 0 ? 0 : a;
    *hi = b > in ? in : b;
}

int table_ksize(int in, int out) {
    const double scale = (double)in / (double)out, support = 2.0 * (scale < 1.0 ? 1.0 : scale);
    return 2 * (int)std::ceil(support) + 1;
}

// rows of H the tallest band of R output rows needs
int band_rows(int h, int nh, int top, int size, int R) {
    int most = 0;
    for (int r0 = 0; r0 < size; r0 += R) {
        int lo, hi, unused;
        tap_range(h, nh, top + r0, &lo, &unused);
        tap_range(h, nh, top + std::min(r0 + R, size) - 1, &unused, &hi);
        most = std::max(most, hi - lo);
    }
    return most;
}

template <int V> int launch(const PrepArgs& a, int n, int lds, hipStream_t stream) {
    DS_ENSURE_DYN_LDS((&resize_crop_kernel<V>), 64 * 1024);
    hipLaunchKernelGGL(resize_crop_kernel<V>, dim3((unsigned)(n * a.bands)), dim3(256), lds, stream, a);
    DS_CHECK_LAUNCH();
    return DS_OK;
}

}  // namespace

extern "C" int dsm_resize_crop_u8(const void* src, long long image_stride, int pitch, int n, int h, int w, int nh, int nw, int top, int left,
                                  int size, const int* hbounds, const int* hcoeffs, int hksize, const int* vbounds, const int* vcoeffs,
                                  int vksize, void* out, void* stream) {
    if (!src || !out || n <= 0 || h <= 0 || w <= 0 || nh <= 0 || nw <= 0 || size <= 0 || image_stride < 0) return DS_E_ARG;
    if (h > 32768 || w > 32768 || nh > 32768 || nw > 32768) return DS_E_SHAPE;
    if (pitch < 3 * w || top < 0 || left < 0 || top + size > nh || left + size > nw) return DS_E_ARG;
    const bool hpass = nw != w, vpass = nh != h;
    if (hpass && (!hbounds || !hcoeffs || hksize < table_ksize(w, nw))) return DS_E_ARG;
    if (vpass && (!vbounds || !vcoeffs || vksize < table_ksize(h, nh))) return DS_E_ARG;
    if (!ds_aligned16(out)) return DS_E_ALIGN;
    if ((hpass && ((reinterpret_cast<uintptr_t>(hbounds) | reinterpret_cast<uintptr_t>(hcoeffs)) & 3u)) ||
        (vpass && ((reinterpret_cast<uintptr_t>(vbounds) | reinterpret_cast<uintptr_t>(vcoeffs)) & 3u)))
        return DS_E_ALIGN;

    PrepArgs a = {};
    a.src = static_cast<const unsigned char*>(src); a.out = static_cast<unsigned char*>(out);
    a.hb = hbounds; a.hc = hcoeffs; a.vb = vbounds; a.vc = vcoeffs;
    a.image_stride = image_stride;
    a.pitch = pitch; a.h = h; a.w = w; a.top = top; a.left = left; a.size = size;
    a.hk = hpass ? hksize : 0; a.vk = vpass ? vksize : 0;

    // the widest load every row start is aligned to
    const uintptr_t align = reinterpret_cast<uintptr_t>(src) | (uintptr_t)image_stride | (uintptr_t)pitch;
    const int V = (align & 15u) == 0 ? 16 : (align & 3u) == 0 ? 4 : 1;

    int unused;
    tap_range(w, nw, left, &a.col_lo, &unused);
    tap_range(w, nw, left + size - 1, &unused, &a.col_hi);
    a.byte_lo = (3 * a.col_lo) & ~(V - 1);
    a.srow = (3 * a.col_hi - a.byte_lo + 15) & ~15;
    a.T = std::min(16, std::max(4, (IP_S_BYTES / a.srow) & ~3));
    if ((long long)a.T * a.srow > IP_S_MAX) return DS_E_SHAPE;

    a.P = (size + 3) & ~3;
    const long long hrow = 3LL * a.P;
    a.R = 0;
    for (int R = std::min(IP_BAND_MAX, size); R >= 1 && !a.R; --R) {
        const int rows = band_rows(h, nh, top, size, R);
        if (rows * hrow <= (R <= 4 ? IP_H_MAX : IP_H_BYTES)) { a.R = R; a.cap_rows = rows; }
    }
    if (!a.R) return DS_E_SHAPE;
    a.bands = (size + a.R - 1) / a.R;
    if ((long long)n * a.bands > 0x7fffffffLL) return DS_E_SHAPE;
    const int lds = a.T * a.srow + (int)(a.cap_rows * hrow);

    (void)hipGetLastError();
    if (V == 16) return launch<16>(a, n, lds, (hipStream_t)stream);
    if (V == 4) return launch<4>(a, n, lds, (hipStream_t)stream);
    return launch<1>(a, n, lds, (hipStream_t)stream);
}
