// 3x3 convolution, LDS-halo implicit GEMM, second generation of the 256-pixel x 128-channel tile (gfx950, split fp16 hi/lo operands).
//
// What round 2 measured on conv3x3_halo_kernel<4> (profiles/r2a_*): the matrix pipe is busy 82 % of the time at 2.4 GHz, every wave
// is parked ~20 % of its life, and the losses are ADDITIVE pieces of serialised non-MFMA work -- the slab-boundary phase that converts
// (GroupNorm affine + SiLU) and publishes the next halo between two barriers (4.5 %), the clustered per-tap scalar/address work (part
// of a 7 % "tap structure" loss; a software-pipelined fragment read alone changed nothing), the weight-DMA issue (2 %), the epilogue
// (3.5-7.5 %).  This kernel keeps the tile shape and data layout of the first one and removes the serialisation:
//
//   * compile-time geometry (template W: 16 / 32 / 64 columns, one image per tile): every LDS address of the tap loop is a
//     per-lane base register plus an instruction immediate -- no per-tap address arithmetic;
//   * the 9 taps of a slab are unrolled with static tap index; fragment reads of K step g+1 are in flight under the MFMAs of step g
//     (asm-ordered reads, counted lgkmcnt);
//   * TWO halo buffers: the next slab's halo is converted and written while the current slab is multiplied, one float4 slot per tap,
//     each slot cut into small pieces that issue in the shadow of individual MFMAs (sched_barrier fences pin the interleave).  There
//     is no slab-boundary phase and no second barrier;
//   * raw halo loads are asm global loads issued one slab ahead with hand-counted vmcnt, so that neither they nor the LDS-DMA weight
//     stream is ever drained by a compiler-inserted vmcnt(0);
//   * the fused 1x1 skip-projection slabs (one tap each) run through the same pipeline.
// Operands (template MODE 2, the only mode; the fp32 and plain-fp16 modes are records in docs/HISTORY.md): fp32 activations and weights as
// fp16 hi + lo halves, three v_mfma_f32_32x32x16_f16 per product (hi*hi, hi*lo, lo*hi), fp32 accumulation.  The halo writer splits the
// activations after the fp32 GroupNorm affine + SiLU (hi half-row and lo half-row of a 144-B halo row), the weights are packed once.
// Scope: taps == 9, stride 1, square power-of-two images: W in {16, 32, 64} with H*W a multiple of 256 (one image per tile), or 8x8
// images with four whole images per tile and no fused input normalisation; 128-column tiles, no split-K.  Everything else stays on
// conv3x3_halo.hip.
#include "pipe_common.h"

namespace igemm {
namespace {

__device__ __attribute__((aligned(16))) float g_zero_page2[64];                                                     // zero-initialised
__device__ __attribute__((aligned(16))) float g_ident_page2[16] = {0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0};  // {mu, A, B} = identity affine

template <int W>
struct Geo2 {
    static constexpr int T = 512;
    static constexpr int NIMG = (W * W >= 256) ? 1 : 256 / (W * W);      // image slots per tile (8x8 images: 4)
    static constexpr int TH = 256 / (W * NIMG), WP = W + 2, HP = TH + 2, NP = NIMG * HP * WP;
    static constexpr int NS = (NP * 8 + T - 1) / T;          // float4 halo slots per thread (6 or 7)
    static constexpr unsigned ROW = WP * 144;                // bytes per halo row (36 floats per pixel)
    static constexpr unsigned HALO_B = NP * 144;             // bytes per halo buffer
    static constexpr unsigned BS_B = 2 * 128 * 32 * 4;       // two weight buffers [128][32] floats (LDS-DMA image, unpadded)
    static constexpr unsigned SMEM = BS_B + 2 * HALO_B;
    static_assert(NS <= 7, "halo slots");
    static_assert(6 * 9216 + 15 < 65536 && 2 * ROW + 288 + 96 < 65536, "immediates");
};

template <int W, int MODE>
__global__ void __launch_bounds__(512, 2) conv3x3_halo2_kernel(const KParams p) {
    static_assert(MODE == 2, "split fp16 hi/lo operands: the only mode (the template argument stays in the kernel's printed name)");
    using G = Geo2<W>;
    constexpr int T = G::T, WP = G::WP, HP = G::HP, TH = G::TH, NIMG = G::NIMG, NP = G::NP, NS = G::NS;
    constexpr unsigned ROW = G::ROW, HALO_B = G::HALO_B, BS_B = G::BS_B;
    constexpr int BKC = 32;                       // channels per slab
    constexpr int NLOAD = NS + 3;                 // asm global loads per slab (raw slots + the three coefficient vectors)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const unsigned lds0 = lds_addr2(smem);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1;
    int mt, nt;
    if (!decode_tile(blockIdx.x, p.mtiles, p.ntiles, mt, nt, 0)) return;
    const int m0 = mt * 256, n0 = nt * 128;
    const int ld_row = tid >> 3, ld_col = (tid & 7) * 4;
    const float* zero = g_zero_page2;
    const float* ident = g_ident_page2;

    const int img0 = m0 / p.HW;
    const int r0 = NIMG == 1 ? (m0 - img0 * p.HW) / W : 0;

    // ---- per-thread halo slots (fixed for the whole K loop) ---------------------------------------------------------------------
    int h_pix[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int hp = (tid >> 3) + j * 64;
        const int sl = hp / (HP * WP), rem = hp - sl * (HP * WP);         // image slot of the tile, pixel inside its halo
        const int hr = rem / WP, hc = rem - hr * WP;
        const int y = r0 + hr - 1, x = hc - 1;
        const bool ok = hp < NP && (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)W;
        h_pix[j] = ok ? ((img0 + sl) * p.H + y) * W + x : -1;
    }
    const bool last_slot_valid = (tid >> 3) + (NS - 1) * 64 < NP;
    const unsigned st_base = lds0 + BS_B + (unsigned)(tid >> 3) * 144 + (unsigned)(tid & 7) * 8;   // + j * 9216 (+ HALO_B)

    // ---- fragment addresses -----------------------------------------------------------------------------------------------------
    unsigned abase[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int m = wr * 64 + i * 32 + (lane & 31);
        const int sl = m / (TH * W), rem = m - sl * (TH * W);
        const int r = rem / W, c = rem - r * W;
        abase[i] = lds0 + BS_B + (unsigned)(((sl * HP + r) * WP + c) * 144) + (unsigned)(lane >> 5) * 16;   // halo buffer 0, tap (0,0), ks 0
    }
    const int b_row = wc * 64 + (lane & 31);
    const unsigned c0 = (unsigned)((lane >> 5) ^ (((lane & 31) >> 1) & 7));
    unsigned bq[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) bq[ks] = lds0 + (unsigned)b_row * 128 + ((c0 ^ (2u * ks)) * 16);

    // ---- weight DMA: this thread's two source rows (16-B chunk pre-swizzled), wave-uniform LDS destinations ---------------------
    const float* bsrc[2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
        bsrc[i] = p.b + (size_t)(n0 + ld_row + 64 * i) * p.ldb + (((tid & 7) ^ ((ld_row >> 1) & 7)) * 4);
    auto b_dma = [&](int kt, int buf) {
        DS_RACE_SKEW(wave);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            float* dst = smem + buf * 4096 + (wave * 8 + 64 * i) * 32;
            typedef const __attribute__((address_space(1))) void* gptr_t;
            typedef __attribute__((address_space(3))) void* lptr_t;
            __builtin_amdgcn_global_load_lds((gptr_t)(bsrc[i] + (size_t)kt * 32), (lptr_t)(dst), 16, 0, 0);
        }
    };

    // ---- slab bookkeeping -------------------------------------------------------------------------------------------------------
    const int nchunks = (p.c0 + p.c1) / BKC;         // 3x3 slabs (9 taps)
    const int nextra = (p.ec0 + p.ec1) / BKC;        // appended 1x1 slabs (centre tap only)
    const int NCH = nchunks + nextra;
    const int KT = nchunks * 9 + nextra;
    const int Ctot = p.c0 + p.c1;
    const bool silu = p.norm_act == DS_ACT_SILU;

    f32x4 hreg[NS];                                   // raw halo of the slab that is converted next
    f32x4 cmu, cga, cbe;                              // its {mu, A, B} vectors (identity when there is nothing to normalise)
    // asm global loads of slab `chunk` (clamped to the last slab: the loads are unconditional so that their count is static)
    auto slab_src = [&](int chunk, const float*& src, int& ld) {
        const bool extra = chunk >= nchunks;
        const int c = (extra ? chunk - nchunks : chunk) * BKC;
        const int cc0 = extra ? p.ec0 : p.c0;
        const bool first = c < cc0;
        const float* s0 = extra ? p.e0 : p.a0;
        const float* s1 = extra ? p.e1 : p.a1;
        src = first ? s0 + c + ld_col : s1 + (c - cc0) + ld_col;
        ld = first ? (extra ? p.elda0 : p.lda0) : (extra ? p.elda1 : p.lda1);
    };
    const float* nsrc = zero; int nld = 0;            // source of the raw loads in progress (set once per slab by load_coefs)
    auto load_slot = [&](auto jc) {
        constexpr int j = decltype(jc)::value;
        const float* ptr = h_pix[j] >= 0 ? nsrc + (size_t)h_pix[j] * nld : zero;
        hreg[j] = gld16(ptr);
    };
    auto load_coefs = [&](int chunk) {
        const int ch = min(chunk, NCH - 1);
        slab_src(ch, nsrc, nld);
        const bool on = p.norm != nullptr && ch < nchunks;
        const float* cp = on ? p.norm + (size_t)img0 * 3 * Ctot + ch * BKC + ld_col : ident;
        const int st = on ? Ctot : 4;
        const float *cp1 = cp + st, *cp2 = cp + 2 * st;
        cmu = gld16(cp);
        cga = gld16(cp1);
        cbe = gld16(cp2);
    };
    // conversion of one element of slot j (GroupNorm affine + SiLU, networks_edm.py:160,167; then the hi / lo split, two elements per
    // dword), then the two 8-B stores of the slot
    f32x4 cvt;
    float cvt_even = 0.f, cvt_even_lo = 0.f;
    auto convert_elem = [&](auto jc, auto ec, bool act) {
        constexpr int j = decltype(jc)::value, e = decltype(ec)::value;
        float v = fmaf(hreg[j][e] - cmu[e], cga[e], cbe[e]);
        if (act) v = ds_silu(v);
        v = h_pix[j] >= 0 ? v : 0.f;
        const float hi = (float)(_Float16)v;
        const float lo = v - hi;                         // exact in fp32
        if constexpr ((e & 1) == 0) { cvt_even = hi; cvt_even_lo = lo; }
        else { cvt[e >> 1] = pack_h2(cvt_even, hi); cvt[2 + (e >> 1)] = pack_h2(cvt_even_lo, lo); }
    };
    auto store_slot = [&](auto jc, unsigned st_addr) {
        constexpr int j = decltype(jc)::value;
        DS_RACE_SKEW(wave);
        if (j < NS - 1 || last_slot_valid) {
            const f32x2 hi = {cvt[0], cvt[1]}, lo = {cvt[2], cvt[3]};
            lds_wr64<j * 9216>(st_addr, hi);              // channels ld_col .. ld_col+3 of the hi half-row
            lds_wr64<j * 9216 + 64>(st_addr, lo);         // and of the lo half-row
        }
    };
    constexpr int NE = 4;                             // elements (channels) per slot
    // "+v" pseudo-uses that tie the asm-loaded registers to the point where their data has landed (asm operands inside lambdas do
    // not capture: bind references first)
    auto touch_slot = [&](auto jc) { f32x4& r = hreg[decltype(jc)::value]; asm volatile("" : "+v"(r)); };
    auto touch_coefs = [&]() { f32x4 &m_ = cmu, &a_ = cga, &b_ = cbe; asm volatile("" : "+v"(m_), "+v"(a_), "+v"(b_)); };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    // ---- prologue: first halo (exposed, once per tile), raw data of the second slab, first two weight tiles --------------------
    b_dma(0, 0);
    if (KT > 1) b_dma(1, 1);
    {
        load_coefs(0);
        static_for<NS>([&](auto jc) { load_slot(jc); });
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        touch_coefs();
        const bool act0 = silu && p.norm != nullptr && nchunks > 0;
        static_for<NS>([&](auto jc) {
            touch_slot(jc);
            static_for<NE>([&](auto ec) { convert_elem(jc, ec, act0); });
            store_slot(jc, st_base);
        });
        load_coefs(1);
        static_for<NS>([&](auto jc) { load_slot(jc); });
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();                    // first halo and both weight tiles are in LDS (vmcnt(0) above)

    int kt = 0;                      // global tap counter = weight K tile
    unsigned hb = 0;                 // byte offset of the CURRENT halo buffer (0 or HALO_B); the other one is being filled
    const unsigned first_off = nchunks > 0 ? 0u : ROW + 144u;
    Frag2S P_, Q_;
    frag_read2s<0>(P_, abase[0] + first_off, abase[1] + first_off, bq[0], bq[2]);
#define DS2_MS(i, j, x, y, f) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(h8, (f).a##i##x), __builtin_bit_cast(h8, (f).b##j##y), acc[i][j], 0, 0, 0)
    // 12 MFMAs of one K step of 16 channels: hi*hi, hi*lo, lo*hi for the 2 x 2 tiles (the accumulators rotate, so that consecutive
    // MFMAs never depend on each other), a hook after each
#define DS2_GROUP_S(f, hook)                                                                                                      \
    DS2_MS(0, 0, h, h, f); hook(IC<0>{}); DS2_MS(0, 1, h, h, f); hook(IC<1>{}); DS2_MS(1, 0, h, h, f); hook(IC<2>{}); DS2_MS(1, 1, h, h, f); hook(IC<3>{});   \
    DS2_MS(0, 0, h, l, f); hook(IC<4>{}); DS2_MS(0, 1, h, l, f); hook(IC<5>{}); DS2_MS(1, 0, h, l, f); hook(IC<6>{}); DS2_MS(1, 1, h, l, f); hook(IC<7>{});   \
    DS2_MS(0, 0, l, h, f); hook(IC<8>{}); DS2_MS(0, 1, l, h, f); hook(IC<9>{}); DS2_MS(1, 0, l, h, f); hook(IC<10>{}); DS2_MS(1, 1, l, h, f); hook(IC<11>{});
    // One tap = two K steps of 16 channels.  Step 0 (fragments P, prefetched after the previous barrier) carries
    // the halo-conversion hooks; then lgkmcnt(0) + vmcnt + barrier; step 1 (fragments Q) carries the weight DMA of tap kt+2, the
    // fragment prefetch of tap kt+1 and the raw loads.
    auto tap = [&](auto t9c, int chunk) {
        Frag2S &P = P_, &Q = Q_;
        constexpr int T9 = decltype(t9c)::value;
        constexpr bool X = (T9 == 9);
        constexpr int TY = X ? 1 : T9 / 3, TX = X ? 1 : T9 % 3;
        constexpr int AOFF = TY * (int)ROW + TX * 144;
        constexpr bool SLAB_END = X || T9 == 8;
        constexpr bool LOADS = X || T9 == 7;
        constexpr int SE = NE + 1, NPOS = 12;
        constexpr int NSTEP = (X ? NS : 1) * SE;
        constexpr int SPP = (NSTEP + NPOS - 1) / NPOS;
        const unsigned va0 = abase[0] + hb, va1 = abase[1] + hb;
        const unsigned cb = (unsigned)(kt & 1) * 16384u;
        const unsigned st_addr = st_base + (hb ^ HALO_B);
        const bool conv_act = silu && p.norm != nullptr && (chunk + 1) < nchunks;
        auto conv_step = [&](auto hc) {
            constexpr int h = decltype(hc)::value;
            constexpr int j = X ? h / SE : T9 - 1, s = X ? h % SE : h;
            if constexpr (h >= 0 && h < NSTEP && j >= 0 && j < NS) {
                if constexpr (h == 0 || (!X && s == 0 && j == 0)) {
                    if constexpr (X) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    touch_coefs();
                }
                if constexpr (s == 0) touch_slot(IC<j>{});
                if constexpr (s < NE) convert_elem(IC<j>{}, IC<s>{}, conv_act);
                else store_slot(IC<j>{}, st_addr);
            }
        };
        auto hookA = [&](auto qc) {
            constexpr int q = decltype(qc)::value;
            constexpr int first = X ? NSTEP - (NPOS - q) * SPP : q * SPP;
            if constexpr (first + SPP > 0 && first < NSTEP) {
                DS2_FENCE();
                static_for<SPP>([&](auto ic) { conv_step(IC<first + decltype(ic)::value>{}); });
                DS2_FENCE();
            }
        };
        DS2_FRAG_WAIT_S(0, P);
        frag_read2s<AOFF + 32>(Q, va0, va1, bq[1] + cb, bq[3] + cb);
        DS2_GROUP_S(P, hookA)
        DS2_FENCE();
        DS2_FRAG_WAIT_S(0, Q);
        if constexpr (!X && T9 == 8) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NLOAD) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        if constexpr (SLAB_END) hb ^= HALO_B;
        const bool next_is_x = SLAB_END ? (chunk + 1 >= nchunks) : false;
        auto hookD = [&](auto kc) {
            constexpr int k = decltype(kc)::value;
            if constexpr (k == 0) {
                DS2_FENCE();
                if (kt + 2 < KT) b_dma(kt + 2, kt & 1);
                DS2_FENCE();
            } else if constexpr (k == 1) {
                DS2_FENCE();
                const unsigned nb = (unsigned)((kt + 1) & 1) * 16384u;
                if constexpr (SLAB_END) {
                    const unsigned off = next_is_x ? ROW + 144u : 0u;
                    frag_read2s<0>(P, abase[0] + hb + off, abase[1] + hb + off, bq[0] + nb, bq[2] + nb);
                } else {
                    constexpr int NY = (T9 + 1) / 3, NX = (T9 + 1) % 3;
                    frag_read2s<NY * (int)ROW + NX * 144>(P, va0, va1, bq[0] + nb, bq[2] + nb);
                }
                DS2_FENCE();
            } else if constexpr (LOADS && k >= 2 && k < 2 + NS + 1) {
                DS2_FENCE();
                if constexpr (k == 2) load_coefs(chunk + 2);
                else load_slot(IC<k - 3>{});
                DS2_FENCE();
            }
        };
        DS2_GROUP_S(Q, hookD)
        DS2_FENCE();
        ++kt;
    };
    int chunk = 0;
    for (; chunk < nchunks; ++chunk) {
        tap(IC<0>{}, chunk); tap(IC<1>{}, chunk); tap(IC<2>{}, chunk);
        tap(IC<3>{}, chunk); tap(IC<4>{}, chunk); tap(IC<5>{}, chunk);
        tap(IC<6>{}, chunk); tap(IC<7>{}, chunk); tap(IC<8>{}, chunk);
    }
    for (; chunk < NCH; ++chunk) tap(IC<9>{}, chunk);
#undef DS2_MS
#undef DS2_GROUP_S
    DS2_FRAG_WAIT_S(0, P_);                           // drain the last (discarded) fragment prefetch

    // drain the unconditional raw loads of the clamped "slab after next"
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    touch_coefs();
    static_for<NS>([&](auto jc) { touch_slot(jc); });
    __syncthreads();
    epilogue<0, true>(p, acc, smem + wave * 32 * EPI_LD, lane, m0 + wr * 64, n0 + wc * 64, p.out);
}

template <int W>
int launch_halo2_w(KParams p, int wide, hipStream_t stream) {
    using G = Geo2<W>;
    p.TH = G::TH; p.nimg = G::NIMG; p.HP = G::HP; p.WP = G::WP; p.NP = G::NP;
    p.mtiles = p.M / 256;
    p.ntiles = wide;
    p.n_begin = 0;
    p.splits = 1;
    int smem = (int)G::SMEM;
    const int epi = 8 * 32 * EPI_LD * (int)sizeof(float);
    if (smem < epi) smem = epi;
    DS_ENSURE_DYN_LDS((&conv3x3_halo2_kernel<W, 2>), 160 * 1024);
    hipLaunchKernelGGL((conv3x3_halo2_kernel<W, 2>), dim3(grid_1d(p.mtiles, p.ntiles), 1), dim3(512), smem, stream, p);
    DS_CHECK_LAUNCH();
    return DS_OK;
}

}  // namespace

// Layers this kernel takes: see the header comment.  `wide` = number of 128-column tiles the caller wants from it: ALL tiles of the layer, a
// ragged last tile multiplies the zero rows the weight packing pads to 128 and its epilogue guards the columns.
bool conv3x3_halo2_applicable(const KParams& p, int wide) {
    const int bkc = 32;
    if (p.taps != 9 || wide < 1) return false;
    if (!(p.W == 8 || p.W == 16 || p.W == 32 || p.W == 64)) return false;
    if (p.HW != p.H * p.W || p.M % 256) return false;
    if (p.W == 8 ? (p.H != 8 || p.norm != nullptr) : (p.HW % 256 != 0)) return false;   // 8x8: four whole images per tile, and no fused
                                                                                       // input normalisation (its planes are per image)
    if ((p.c0 + p.c1) % bkc || (p.ec0 + p.ec1) % bkc || (p.c1 > 0 && p.c0 % bkc) || (p.ec1 > 0 && p.ec0 % bkc)) return false;
    if ((p.c0 + p.c1) == 0) return false;
    if (p.nrows_b < wide * 128) return false;                 // every weight row of the tiles exists (rows are padded to 128)
    return true;
}

int launch_conv3x3_halo2(KParams& p, int wide, hipStream_t stream) {
    switch (p.W) {
        case 8: return launch_halo2_w<8>(p, wide, stream);
        case 16: return launch_halo2_w<16>(p, wide, stream);
        case 32: return launch_halo2_w<32>(p, wide, stream);
        default: return launch_halo2_w<64>(p, wide, stream);
    }
}

}  // namespace igemm
