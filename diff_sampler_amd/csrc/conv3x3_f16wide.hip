// 3x3 stride-1 convolution on fp16 activations for images WIDER than 64 pixels (gfx950, v_mfma_f32_32x32x16_f16): the matrix kernel of
// conv3x3_f16dma.hip on a 2-D PATCH of one image instead of whole image rows.  Kernel id 2575.
//
// Why: conv3x3_f16dma_kernel stages whole image rows (256 pixels = 256 / W rows with their halo), so its LDS halo grows with W and the
// kernel stops at W = 64.  The AutoencoderKL decoder (vae_engine.py) runs 3x3 convolutions at 128, 256 and 512 pixels wide -- 91 % of its
// FLOPs -- and had no fp16-activation route at all.  Here the pixel tile is a patch of 4 rows x 64 columns of ONE image with its one-pixel
// halo (6 x 66 = 396 pixels of a 64-channel slab = 7 DMA rounds of 8 KB), whatever the image size:
//
//   * a wave's 64 output pixels (wave row wr = wave >> 1) are ONE patch row = 64 CONSECUTIVE rows of the [M][cout] output matrix, so both
//     epilogues of the family (epi_direct.h, epilogue_pipe: bias, fp16 / fp32 residual, activation, fp16 / fp32 rows, GroupNorm column
//     sums per 64-row block) run unchanged on the wave's own row base -- a 16 x 16 or 8 x 32 patch would fetch 18 - 24 % fewer halo pixels
//     (324 / 340 against 396) but scatter a wave's rows over 4 / 2 image rows and need a third epilogue;
//   * the LDS image of the patch is exactly the one the 64-column instantiation of conv3x3_f16dma_kernel uses (pixel-major 128-B rows,
//     16-B chunk XOR-swizzled by (halo pixel >> 1) & 7 on the DMA source address and on the fragment read: the 32 lanes of a fragment read
//     are 32 consecutive pixels of one patch row), so the bank behaviour measured there carries over;
//   * halo pixels outside the IMAGE fetch a zero page (the convolution's zero padding); halo pixels inside the image that belong to a
//     neighbouring patch are simply fetched -- every patch reads its own halo from the activation tensor, nothing is exchanged;
//   * weights: the tap ring of conv3x3_f16dma (NB * 64 rows x 128 B per tap, D = 2 .. 4 taps deep), same packing (ops.pack_conv_weight_f16);
//   * tiles never span images and there is no split-K: no decision depends on the batch, every output element is the same K-ordered fp32
//     sum at any batch size (the batch-invariant mode needs nothing special here).
// LDS: 2 halo buffers x 56 KB + D x NB x 8 KB weights = 160 KB at NB = 3 (D = 2), 160 KB at NB = 2 (D = 3), 144 KB at NB = 1 (D = 4): one
// workgroup of eight waves per CU, like the kernel it derives from.
// Scope: taps == 9, stride 1, ONE activated fp16 source [M][c0] (c0 % 64 == 0), no fused input normalisation, W a power of two >= 128,
// H a power of two >= 4, cout % 64 == 0.  Reached from route_conv only where conv3x3_f16dma_applicable refuses.
// U-Net blocks above 64 pixels (the consistency-model LSUN nets: 256 channels x (1, 1, 2, 2, 4, 4) over 256 .. 8 pixels) need two more things:
//   * the per-image embedding row of conv0 (ds_conv_args.cbias): both epilogues already take it -- a patch never spans images and
//     HW % 32 == 0, so it is one row pointer per wave;
//   * appended 1x1 slabs, the fused skip projection of conv1 (ds_conv_args.e0 / ec0, ec0 % 64 == 0, ONE raw fp16 source of the layer's own
//     geometry; K order and packing of conv3x3_f16dma: ops.pack_conv_weight_f16(w, skip_w)): the X1 instantiations, kernel id 2576.  An
//     appended slab is a one-tap slab (the centre tap) behind the 3x3 slabs.  Its operand goes through the same patch image, of which the
//     centre tap reads the interior only (halo pixels 67 .. 328): DMA rounds 1 .. 5 of 7 are fetched.  The ec0 == 0 instantiations are the
//     code they were (2575).
#include "pipe_common.h"
#include "epi_direct.h"

namespace igemm {
namespace {

__device__ __attribute__((aligned(128))) _Float16 g_zero_halfs_wide[64];   // zero-initialised: the 128-B row of an out-of-image pixel

constexpr int PW = 64, PH = 4;                                             // output patch: 4 rows x 64 columns = 256 pixels
constexpr int WPW = PW + 2, HPW = PH + 2, NPW = HPW * WPW;                 // halo: 6 x 66 = 396 pixels
constexpr int NDMAW = (NPW * 8 + 511) / 512;                               // 7 DMA rounds (512 threads x 16 B = 8 KB each)
constexpr unsigned HALO_BW = NDMAW * 8192u;

template <int NB>
constexpr int f16wide_ring() {
    const int fit = (int)((160u * 1024u - 2u * HALO_BW) / (NB * 8192u));
    return NB >= 3 ? 2 : (fit > 4 ? 4 : (fit < 2 ? 2 : fit));
}
template <int NB>
constexpr unsigned f16wide_smem() { return (unsigned)f16wide_ring<NB>() * NB * 8192u + 2u * HALO_BW; }

// DIRECT: the epilogue that stores straight from the accumulators (fp16 rows out) or the staged one (fp32 rows out), as in conv3x3_f16dma
// X1: the layer has appended 1x1 slabs (p.ec0 > 0)
template <int NB, bool DIRECT, bool X1>
__global__ void __launch_bounds__(512, 2) conv3x3_f16wide_kernel(const KParams p) {
    constexpr unsigned WB = NB * 8192u, HB = HALO_BW;
    constexpr int D = f16wide_ring<NB>();                      // weight ring: taps kt .. kt + D - 1 are in LDS or in flight
    static_assert(f16wide_smem<NB>() <= 160u * 1024u, "LDS");
    extern __shared__ __attribute__((aligned(16))) float smem[];
    char* lds = reinterpret_cast<char*>(smem);                 // [weights 0 | ... | weights D - 1 | halo 0 | halo 1]
    typedef const __attribute__((address_space(1))) void* gptr_t;
    typedef __attribute__((address_space(3))) void* lptr_t;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    int mt, nt;
    if (!decode_tile(blockIdx.x, p.mtiles, p.ntiles, mt, nt, 0)) return;
    const int n0 = p.n_begin + nt * (NB * 64);
    const _Float16* a0 = reinterpret_cast<const _Float16*>(p.a0);
    const _Float16* wgt = reinterpret_cast<const _Float16*>(p.b);
    const size_t ldbh = (size_t)p.ldb * 2;                     // weight row pitch in halfs

    // patch mt of the batch: image, patch row, patch column (column fastest: neighbours in x share halo columns, neighbours in y halo rows)
    const int ptx = p.W / PW, ppi = ptx * (p.H / PH);
    const int img = mt / ppi, prem = mt - img * ppi;
    const int py0 = (prem / ptx) * PH, px0 = (prem % ptx) * PW;

    // ---- halo DMA: thread tid owns 16-B unit j * 512 + tid of round j: halo pixel j * 64 + (tid >> 3), LDS chunk slot tid & 7; the source
    // chunk is slot ^ ((pixel >> 1) & 7) = slot ^ ((tid >> 4) & 7) in every round ------------------------------------------------------
    int hpix[NDMAW];                                           // source pixel (-1: zero page)
    const int hch = ((tid & 7) ^ ((tid >> 4) & 7)) * 8;
#pragma unroll
    for (int j = 0; j < NDMAW; ++j) {
        const int hp = j * 64 + (tid >> 3);
        const int hr = hp / WPW, hc = hp - hr * WPW;
        const int y = py0 + hr - 1, x = px0 + hc - 1;
        const bool ok = hp < NPW && (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W;
        hpix[j] = ok ? (img * p.H + y) * p.W + x : -1;
    }
    const int N33 = p.c0 / 64;                                 // 64-channel slabs, nine taps each
    const int NCH = X1 ? N33 + p.ec0 / 64 : N33;               // ... followed by the appended 1x1 slabs, one (centre) tap each
    const int KT = X1 ? N33 * 9 + (NCH - N33) : N33 * 9;
    const _Float16* e0 = reinterpret_cast<const _Float16*>(p.e0);
    constexpr int JX0 = (WPW + 1) / 64, JX1 = ((PH - 1) * WPW + PW - 1 + WPW + 1) / 64;      // DMA rounds that hold the patch interior: 1 .. 5
    auto halo_dma = [&](int chunk, int hbuf, auto jc) {        // DMA round j of slab `chunk` into halo buffer hbuf
        constexpr int j = decltype(jc)::value;
        const _Float16* base = a0 + (size_t)chunk * 64;
        int ld = p.lda0;
        if constexpr (X1) {
            if (chunk >= N33) {                                // appended slab: the raw second tensor, interior rounds only
                if (j < JX0 || j > JX1) return;
                base = e0 + (size_t)(chunk - N33) * 64; ld = p.elda0;
            }
        }
        const _Float16* g = hpix[j] >= 0 ? base + (size_t)hpix[j] * ld + hch : g_zero_halfs_wide;
        DS_RACE_SKEW(wave);
        __builtin_amdgcn_global_load_lds((gptr_t)g, (lptr_t)(lds + D * WB + hbuf * HB + (j * 512 + wave * 64) * 16), 16, 0, 0);
    };

    // ---- weight DMA of tap kt: rows i * 64 + (tid >> 3), i < NB; the source chunk is pre-swizzled ---------------------------------------
    const _Float16* wsrc = wgt + (size_t)(n0 + (tid >> 3)) * ldbh + (((tid & 7) ^ ((tid >> 4) & 7)) * 8);
    auto w_dma = [&](int kt, int wbuf) {
        DS_RACE_SKEW(wave);
#pragma unroll
        for (int i = 0; i < NB; ++i)
            __builtin_amdgcn_global_load_lds((gptr_t)(wsrc + (size_t)i * 64 * ldbh + (size_t)kt * 64),
                                             (lptr_t)(lds + wbuf * WB + (i * 64 + wave * 8) * 128), 16, 0, 0);
    };
    auto w_dma_row = [&](int kt, int wbuf, auto ic) {          // one 64-row block of it (issued between MFMAs, see the tap)
        constexpr int i = decltype(ic)::value;
        if (i == 0) DS_RACE_SKEW(wave);
        __builtin_amdgcn_global_load_lds((gptr_t)(wsrc + (size_t)i * 64 * ldbh + (size_t)kt * 64),
                                         (lptr_t)(lds + wbuf * WB + (i * 64 + wave * 8) * 128), 16, 0, 0);
    };

    // ---- fragment addresses: row block i covers 32 consecutive pixels of patch row wr; tap (ty, tx) reads halo pixel hp0[i] + ty * 66 + tx,
    // chunk (2 ks + g) ^ ((hp >> 1) & 7) ------------------------------------------------------------------------------------------------
    int hp0[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) hp0[i] = wr * WPW + i * 32 + (lane & 31);
    const unsigned gsel = (unsigned)(lane >> 5);
    auto a_addr = [&](int i, int tt) -> unsigned {             // byte offset inside a halo buffer, K step 0
        const unsigned hp = (unsigned)(hp0[i] + (tt / 3) * WPW + (tt % 3));
        return hp * 128u + 16u * (((hp >> 1) & 7u) ^ gsel);
    };
    const int brow = wc * (NB * 32) + (lane & 31);
    const unsigned lds0 = lds_addr2(smem);
    const unsigned bbase = lds0 + (unsigned)brow * 128u + 16u * (unsigned)(((brow >> 1) & 7) ^ (lane >> 5));

    f32x16 accA[2][2], accB[2][2];                             // output columns [0, 64) and [64, 128) of the wave tile
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) { accA[i][j][r] = 0.f; accB[i][j][r] = 0.f; }

    // Fragment sets of one K step (16 channels): two A blocks (32 pixels each), NB weight blocks.  Reads are volatile asm in program
    // order; the wait names the set it releases ("+v"), so no use can move above it.
    struct Frag { f32x4 a0, a1, b0, b1, b2; };
    auto frag_read = [&](Frag& f, unsigned va0, unsigned va1, unsigned vb) {
        f.a0 = lds_rd<0>(va0);
        f.a1 = lds_rd<0>(va1);
        f.b0 = lds_rd<0>(vb);
        if constexpr (NB > 1) f.b1 = lds_rd<4096>(vb);
        if constexpr (NB > 2) f.b2 = lds_rd<8192>(vb);
    };
    auto frag_wait = [&](Frag& f, auto nc) {                   // wait until at most N younger LDS operations are outstanding
        constexpr int N = decltype(nc)::value;
        if constexpr (NB == 1) asm volatile("s_waitcnt lgkmcnt(%3)" : "+v"(f.a0), "+v"(f.a1), "+v"(f.b0) : "n"(N));
        if constexpr (NB == 2) asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(f.a0), "+v"(f.a1), "+v"(f.b0), "+v"(f.b1) : "n"(N));
        if constexpr (NB == 3) asm volatile("s_waitcnt lgkmcnt(%5)" : "+v"(f.a0), "+v"(f.a1), "+v"(f.b0), "+v"(f.b1), "+v"(f.b2) : "n"(N));
    };
    // SWAPPED product: the weight fragment is the MFMA's first operand, so an accumulator block holds lane = pixel, registers = channels
#define DSW_MM(acc_, a_, b_) acc_ = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8, b_), __builtin_bit_cast(h8, a_), acc_, 0, 0, 0)
    auto mfma_group = [&](Frag& f) {                           // consecutive MFMAs never touch the same accumulator
        DSW_MM(accA[0][0], f.a0, f.b0); DSW_MM(accA[1][0], f.a1, f.b0);
        if constexpr (NB > 1) { DSW_MM(accA[0][1], f.a0, f.b1); DSW_MM(accA[1][1], f.a1, f.b1); }
        if constexpr (NB > 2) { DSW_MM(accB[0][0], f.a0, f.b2); DSW_MM(accB[1][0], f.a1, f.b2); }
    };
    constexpr int NR = 2 + NB;                                 // LDS reads per fragment set
    const unsigned halo0 = lds0 + D * WB;

    // ---- prologue: halo of slab 0, round 0 of slab 1's halo, weights of the first D taps ------------------------------------------------
    static_for<NDMAW>([&](auto jc) { halo_dma(0, 0, jc); });
    if (1 < NCH) {
        if (X1 && 1 >= N33) static_for<NDMAW>([&](auto jc) { halo_dma(1, 1, jc); });      // slab 1 is a one-tap slab: all of it now
        else halo_dma(1, 1, IC<0>{});
    }
#pragma unroll
    for (int d = 0; d < D; ++d)
        if (d < KT) w_dma(d, d);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    Frag P_, Q_;
    frag_read(P_, halo0 + a_addr(0, 0), halo0 + a_addr(1, 0), bbase);

    int kt = 0, slot = 0;                                      // slot = kt % D: the ring buffer of tap kt
    // One tap (T9 = 0 .. 8 of a 3x3 slab, 9 = the centre tap of an appended 1x1 slab).  P holds the fragments of its K step 0 (read after the previous tap's barrier).
    //   K steps 0..2 : reads of step k+1 in flight under the MFMAs of step k
    //   then         : all reads of this tap done, own DMAs landed (counted, see below), barrier: ring buffer kt % D -- and, at a slab end, the
    //                  halo buffer -- are free and the operands of tap kt+1 are in LDS
    //   K step 3     : behind the barrier: the first fragment reads of tap kt+1, the step's MFMAs and -- between them -- the DMA issue of tap
    //                  kt+D's weights and of the next halo round
    // Halo schedule: slab s+1 lives in buffer (s+1) & 1, free once slab s-1 is done; its 7 DMA rounds are issued one per barrier: round 0 at
    // the last tap of slab s-1 (or in the prologue), rounds 1 .. 6 behind the barriers of taps 0 .. 5 of slab s.  Every round is covered by
    // the vmcnt(0) of the slab's last tap at the latest, and that tap's barrier publishes it.  A slab that FOLLOWS a one-tap slab has no such
    // taps to ride on: all its rounds are issued at once, at the last tap of the slab before that one (or in the prologue).
    auto tap = [&](auto t9c, int chunk) {
        Frag &P = P_, &Q = Q_;
        constexpr int T9 = decltype(t9c)::value;
        constexpr bool X = (T9 == 9);
        constexpr int TT = X ? 4 : T9;
        constexpr bool SLAB_END = X || T9 == 8;
        const unsigned hoff = halo0 + (unsigned)(chunk & 1) * HB;
        const unsigned woff = (unsigned)slot * WB;
        const int nslot = slot + 1 == D ? 0 : slot + 1;
        const unsigned a_0 = a_addr(0, TT) + hoff, a_1 = a_addr(1, TT) + hoff;
        const unsigned vb = bbase + woff;
        frag_read(Q, a_0 ^ 32u, a_1 ^ 32u, vb ^ 32u);
        frag_wait(P, IC<NR>{});
        DS2_FENCE(); mfma_group(P); DS2_FENCE();
        frag_read(P, a_0 ^ 64u, a_1 ^ 64u, vb ^ 64u);
        frag_wait(Q, IC<NR>{});
        DS2_FENCE(); mfma_group(Q); DS2_FENCE();
        frag_read(Q, a_0 ^ 96u, a_1 ^ 96u, vb ^ 96u);
        frag_wait(P, IC<NR>{});
        DS2_FENCE(); mfma_group(P); DS2_FENCE();
        frag_wait(Q, IC<0>{});
        // own DMAs landed: everything at a slab end (the next slab's halo) and in the last D - 1 taps; otherwise all but the youngest
        // (D - 2) * NB requests -- the weights of taps kt + 2 .. kt + D - 1 (loads complete in order; halo rounds issued in between only
        // make this wait for more than it needs)
        if (D == 2 || SLAB_END || kt + D > KT) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"((D - 2) * NB) : "memory");
        __builtin_amdgcn_s_barrier();
        DS2_FENCE();
        if (kt + 1 < KT) {
            const unsigned nwoff = (unsigned)nslot * WB;
            if constexpr (SLAB_END) {
                const unsigned nh = halo0 + (unsigned)((chunk + 1) & 1) * HB;
                const int nt9 = (X1 && chunk + 1 >= N33) ? 4 : 0;
                frag_read(P, nh + a_addr(0, nt9), nh + a_addr(1, nt9), bbase + nwoff);
            } else {
                frag_read(P, a_addr(0, T9 + 1) + hoff, a_addr(1, T9 + 1) + hoff, bbase + nwoff);
            }
        }
        auto halo_issue = [&]() {
            if constexpr (SLAB_END) {
                if (chunk + 2 < NCH) {
                    if (X1 && chunk + 1 >= N33) static_for<NDMAW>([&](auto jc) { halo_dma(chunk + 2, chunk & 1, jc); });   // next slab has one tap
                    else halo_dma(chunk + 2, chunk & 1, IC<0>{});
                }
            } else if constexpr (T9 + 1 < NDMAW) {
                if (chunk + 1 < NCH) halo_dma(chunk + 1, (chunk + 1) & 1, IC<T9 + 1>{});
            }
        };
        {
            const bool wd = kt + D < KT;
            DS2_FENCE();
            DSW_MM(accA[0][0], Q.a0, Q.b0); DSW_MM(accA[1][0], Q.a1, Q.b0);
            DS2_FENCE(); halo_issue(); if (wd) w_dma_row(kt + D, slot, IC<0>{}); DS2_FENCE();
            if constexpr (NB > 1) {
                DSW_MM(accA[0][1], Q.a0, Q.b1); DSW_MM(accA[1][1], Q.a1, Q.b1);
                DS2_FENCE(); if (wd) w_dma_row(kt + D, slot, IC<1>{}); DS2_FENCE();
            }
            if constexpr (NB > 2) {
                DSW_MM(accB[0][0], Q.a0, Q.b2); DSW_MM(accB[1][0], Q.a1, Q.b2);
                DS2_FENCE(); if (wd) w_dma_row(kt + D, slot, IC<2>{}); DS2_FENCE();
            }
        }
        DS2_FENCE();
        ++kt; slot = nslot;
    };
    for (int chunk = 0; chunk < N33; ++chunk) {
        tap(IC<0>{}, chunk); tap(IC<1>{}, chunk); tap(IC<2>{}, chunk);
        tap(IC<3>{}, chunk); tap(IC<4>{}, chunk); tap(IC<5>{}, chunk);
        tap(IC<6>{}, chunk); tap(IC<7>{}, chunk); tap(IC<8>{}, chunk);
    }
    if constexpr (X1)
        for (int chunk = N33; chunk < NCH; ++chunk) tap(IC<9>{}, chunk);
#undef DSW_MM
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // (no fragment read is pending after the last tap; cheap insurance)

    // the wave's 64 output pixels = patch row wr: 64 consecutive rows of the output matrix, a whole 64-row block of the column sums
    const int wm0 = (img * p.H + py0 + wr) * p.W + px0;
    const int wn0 = n0 + wc * (NB * 32);
    if constexpr (DIRECT) epilogue_direct<false, NB, true>(p, accA, accB, lane, wm0, wn0);
    else {
        float* stage = smem + wave * 32 * EPI_LD;
        epilogue_pipe<0, true, (NB == 1 ? 32 : 64), (NB == 3 ? 32 : 0), true>(p, accA, accB, stage, lane, wm0, wn0, p.out);
    }
}

template <int NB>
int launch_wide_nb(KParams p, int n_begin, int ntiles, hipStream_t stream) {
    p.mtiles = p.M / 256;
    p.ntiles = ntiles;
    p.n_begin = n_begin;
    p.splits = 1;
    p.coef_lds = 0;                                            // (epilogue_pipe reads its A/B switches here)
    int smem = (int)f16wide_smem<NB>();
    const bool staged = !epi_direct_ok(p, true, NB);
    const dim3 grid(grid_1d(p.mtiles, p.ntiles));
#define DSW_LAUNCH(DIRECT_, X1_)                                                                                   \
    do {                                                                                                          \
        DS_ENSURE_DYN_LDS((&conv3x3_f16wide_kernel<NB, DIRECT_, X1_>), 160 * 1024);                                \
        hipLaunchKernelGGL((conv3x3_f16wide_kernel<NB, DIRECT_, X1_>), grid, dim3(512), smem, stream, p);          \
    } while (0)
    if (p.ec0) { if (staged) DSW_LAUNCH(false, true); else DSW_LAUNCH(true, true); }
    else { if (staged) DSW_LAUNCH(false, false); else DSW_LAUNCH(true, false); }
#undef DSW_LAUNCH
    DS_CHECK_LAUNCH();
    return DS_OK;
}

bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

}  // namespace

bool conv3x3_f16wide_applicable(const KParams& p) {
    if (p.taps != 9 || p.stride > 1) return false;
    if (!pow2(p.W) || !pow2(p.H) || p.W < 2 * PW || p.H < PH) return false;           // whole 4 x 64 patches; narrower images: conv3x3_f16dma
    if (p.HW != p.H * p.W || p.M <= 0 || p.M % p.HW) return false;
    if (p.c0 <= 0 || p.c0 % 64 || p.c1 || p.ec1 || p.norm) return false;             // one activated fp16 source
    if (p.ec0 < 0 || p.ec0 % 64 || (p.ec0 && !p.e0)) return false;                   // appended 1x1 slabs: whole 64-channel slabs of one raw fp16 source
    if (p.rowbias || p.out_planar || p.act == DS_ACT_GEGLU) return false;
    if (p.N % 64 || !p.vec_ok || p.nrows_b < p.N) return false;
    return true;
}

// Column tiling: groups of (first column, tiles, NB), widest first, from the cost model of conv3x3_f16dma (a tile of 64 * nb columns costs
// about 1 + nb; these layers have thousands of pixel tiles, so only the sum over the column tiles matters): 128 -> 128, 256 -> 2 x 128,
// 512 -> 2 x 192 + 128.  ds_conv_args.tune.f16dma_nb forces the starting width.  No split-K.
void conv3x3_f16wide_route(const KParams& p, ConvRoute& r) {
    auto tiling = [&](int nb0, int (*out)[3], int* cost) {
        int n = 0, col = 0, c = 0;
        for (int w = nb0; w >= 1 && col < p.N; --w) {
            const int t = (p.N - col) / (64 * w);
            if (t > 0) { out[n][0] = col; out[n][1] = t; out[n][2] = w; ++n; col += t * 64 * w; c += t * (1 + w); }
        }
        *cost = c;
        return n;
    };
    int best_nb = 3, best_cost = 0x7fffffff, best_n = 99, cost;
    if (p.t_nb > 0) best_nb = p.t_nb < 3 ? p.t_nb : 3;
    else
        for (int nb = 3; nb >= 1; --nb) {
            int tmp[4][3];
            const int n = tiling(nb, tmp, &cost);
            if (cost < best_cost || (cost == best_cost && n < best_n)) { best_cost = cost; best_n = n; best_nb = nb; }
        }
    r.kernel_id = p.ec0 ? 2576 : 2575;                         // 2576: the instantiations with appended 1x1 slabs
    r.splits = 1;
    r.ngroups = tiling(best_nb, r.groups, &cost);
}

int launch_conv3x3_f16wide(KParams& p, const ConvRoute& r, hipStream_t stream) {
    for (int i = 0; i < r.ngroups; ++i) {
        const int col = r.groups[i][0], tiles = r.groups[i][1], nb = r.groups[i][2];
        int rc;
        switch (nb) {
            case 1: rc = launch_wide_nb<1>(p, col, tiles, stream); break;
            case 2: rc = launch_wide_nb<2>(p, col, tiles, stream); break;
            default: rc = launch_wide_nb<3>(p, col, tiles, stream); break;
        }
        if (rc) return rc;
    }
    return DS_OK;
}

}  // namespace igemm
