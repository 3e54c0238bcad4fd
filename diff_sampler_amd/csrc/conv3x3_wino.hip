// 3x3 stride-1 convolution in the Winograd form F(2x2, 3x3) on the exact-fp32 MFMA (gfx950).
//
// The direct LDS-halo kernel (conv3x3_halo.hip) runs at 0.88 of the fp32 matrix peak on the 256 x 256 tile: only removing multiply-adds makes
// those layers faster.  F(2x2, 3x3) computes a 2 x 2 output patch ("tile") from a 4 x 4 input patch with 16 multiplies per (cin, cout) pair
// instead of 36 -- 2.25 x fewer MFMA operations, still in fp32:
//     Y = A^T [ sum_c (G g_c G^T) . (B^T d_c B) ] A          (. = elementwise over the 16 positions; entries of A, B: 0, +-1; of G: 0, +-1, +-1/2)
// i.e. 16 independent [tiles x channels] x [channels x cout] products, one per position of the 4 x 4 transformed patch.
//
// THREE KERNELS, bit-identical in `out` and in the statistics (tests/test_hip_wino_w8.py, tests/test_hip_wino_n128.py); launch_conv3x3_wino chooses:
//   wino_w8_kernel       32 tiles x 128 channels on EIGHT waves, two per SIMD: the DEFAULT at 16 and 32 columns (profiles/wino_w8_ab.txt:
//                        - 3.0 ... - 3.8 % per layer against wino_n128_kernel; nothing gained at 64 columns, where it is not built).
//   wino_n128_kernel     32 tiles x 128 channels on four waves, one per SIMD (profiles/wino_n128_ab.txt: - 4.3 ... - 5.1 % per layer at 16 and
//                        32 columns, - 10 % at 64, against the first kernel): the default at every other width, and ds_conv_tune.variant
//                        bit 15 (32768) selects it at 16 and 32 columns.
//   conv3x3_wino_kernel  64 tiles x 64 channels on four waves, the first kernel.  ds_conv_tune.variant bit 10 (1024) selects it: A/B
//                        timing in one process, the bit comparison of the tests, and the timing ablations (-DDS_CONV_ABLATIONS).
// What makes them bit-identical is what they share: the slab order, K step r = 0 .. 3 per position and slab, the halo stage, the skip
// loop's order (group, K step r, patch pixel), the association of the output transform's sums, and the epilogue.  The halo stage and
// the skip-slab staging are written ONCE (WinoHalo, WinoSkip below) and described once, here -- but for conv3x3_wino_kernel, which has
// its own copy of the halo stage, the same code text (the comment at WinoHalo says why).  The epilogue of a patch row is the same code
// text in each kernel: written once it compiled to 37 - 81 more instructions per kernel and the layers with the fewest slabs measured
// 0.4 - 1.3 % slower (profiles/wino_shared_isa.txt, profiles/wino_shared_ab.txt); a fix to it has to be made three times.  A kernel
// owns its tile, who holds which positions, its input transform, its weight path, its slot tables and (wino_w8_kernel) the exchange,
// described under its name further down.
//
// SHARED BY ALL THREE
//   workgroup = the output pixels of TH rows x W columns of ONE image (TH x W = 256 or 128, i.e. 64 or 32 tiles) x 64 or 128 output
//               channels; a wave's accumulators are 32 tiles x 32 channels per position (f32x16 each).
//   slab      = 8 input channels.  Per slab: the raw halo (TH+2) x (W+2) pixels x 8 channels goes global -> registers -> LDS `Hs` with the
//               consumer's GroupNorm affine + SiLU applied on the way (the halo stage), is transformed to V = B^T d B in LDS `Vs` (16
//               positions x tiles x 8 channels), and meets the transformed weights U (ops.pack_conv_weight_wino) in 16 positions x 4 K
//               steps of v_mfma_f32_32x32x2_f32 per 32 x 32 block.  Vs and Hs are double buffers.
//   LDS image = [position][channel quad kh = 0 / 1][row][4 floats]: an MFMA fragment read is one ds_read_b128 per lane at (kh = lane >> 5,
//               row = lane & 31), 512 contiguous bytes per 32 lanes -- conflict-free, and the K index of step r is channel 4 kh + r on
//               both operands.  Hs is split into planes [kh][column parity][row][column / 2][4] so that the tiles of a row (pixels two
//               apart) read consecutive 16-byte cells.
//   sum order = slab order, then the channel order inside the MFMA; no split-K, no dependence on batch or grid.
//
// Halo stage (WinoHalo).  A thread owns up to NSH float4 slots (halo pixel, channel quad), fixed for the whole K loop; NSL of them can
// hold a halo pixel at the launch's width.  Per slab a slot is one global load -- a SCALAR base (the source a0 | a1 at the slab's
// channel) plus a 32-bit byte offset chosen by a bit-select between two per-slot offsets, so that nothing between the MFMAs branches or
// does 64-bit vector arithmetic -- and, a slab later, the halo store: the consumer's affine (a subtraction and ONE fma on the
// coefficient planes {mu, A, B} of the tile's image, three more loads per slab) and SiLU (ds_silu's operations), once per element, then
// one ds_write_b128.  What is uniform per launch (normalisation none / affine / affine + SiLU; the active slots) is a template parameter.
// Out-of-image cells: which halo cells lie outside the image is fixed for the tile (its left and right columns; its top or bottom row
// where the tile touches the image's), so their zeros are written ONCE, into both Hs buffers, where the thread's LDS cells are set up
// (WinoHalo::cells, in front of the thread's first halo store) -- by the thread that owns the slot, which never stores there again: a slot that holds no in-image pixel -- an
// out-of-image pixel, loaded from the nearest pixel of the same image, or a slot beyond the halo -- stores into the spare cell behind
// its Hs buffer.  The prologue's first barrier publishes the zeros with halo 0 and 1, and the LDS may hold whatever the workgroup before
// left.  The halo store used to select `in-image ? v : 0` per element, 12 v_cndmask per slab and thread on top of the MFMAs
// (profiles/wino_persist_ab.txt: - 2.0 ... - 2.8 % per layer).
//
// Who orders what: ONE barrier per slab.  Between barrier s-1 and barrier s a wave
//     reads   Vs[s & 1] (and its weights)  the MFMAs of slab s
//     reads   Hs[(s+1) & 1]             the transform of slab s+1 (published at barrier s-1)
//     writes  Vs[(s+1) & 1]             the same; last read by the MFMAs of slab s-1 (barrier s-1 passed)
//     writes  Hs[s & 1]                 the halo store of slab s+2, from registers; last read by the transform of slab s, which ran in
//                                       front of barrier s-1
//     loads                             the halo and the coefficients of slab s+3 into the registers the halo store has just consumed
// The prologue stages halo 0 and 1 (requested together) and transform 0 and requests halo 2: two barriers.  s+1 / s+2 / s+3 are clamped
// to the last slab: the last slab issues a redundant transform and halo store into the buffers nobody reads and redundant loads (a wave's
// LDS writes complete in order in front of its later ones).  BEHIND THE LAST BARRIER EVERY K-LOOP BUFFER IS DEAD: the exchange, the
// skip-slab loop and the epilogue staging reuse the LDS from offset 0 on that ground alone.
//
// Between two barriers, in program order: the LDS reads of the transform, the halo store with its arithmetic, the transform's adds and
// writes, the fragment reads of position group 0, then ONE basic block of micro-slots -- an MFMA, then at most one memory instruction,
// pinned there by __builtin_amdgcn_sched_barrier(0).  Each kernel has its own slot table (at its K loop).  What stands between the fp32
// MFMAs is MEMORY instructions only.  Vector arithmetic beside v_mfma_f32_32x32x2_f32 is not hidden by it (profiles/wino_kloop_ab.txt:
// the transform costs the same in front of the block as spread over its slots, one packed add per slot is slower than both, and taking
// the 64-bit address adds of a slab's 14 or 15 global loads and DMA pieces out of the block gained 4-6 % per layer).  So the halo store's
// arithmetic and the transform's adds stay in FRONT of the block, and the global loads between the MFMAs take a SCALAR base and a 32-bit
// lane offset (the `global_load ... v, s[..]` form; the offsets are kept in bytes and opaque, so that the compiler does not widen them
// outside the loop).
//
// Skip slabs (WinoSkip): the fused skip projection, appended 1x1 slabs e0 | e1 of 32 raw channels each, as plain MFMA groups on the
// post-transform accumulators, one per patch pixel, in the order group, K step r, patch pixel.  The slab's pixels x 32 channels go global
// -> registers -> a V buffer as [patch pixel][8-channel group][kh][tile][4]; 8 threads hold the 8 chunks of 4 channels of one pixel, so a
// thread has (tile pixels x 8 / threads) float4 slots.  ONE barrier per slab, in the K loop's style: the MFMAs of slab es, the stores of
// the pixels of slab es+1 (requested a slab ago) and the loads of slab es+2 into the registers just stored; es+1 / es+2 clamped to the
// last slab.  No VALU between the MFMAs but the address adds of the stores and loads: the source e0 | e1 (scalar base, row step,
// per-thread offset) is selected in front.  The V buffers are swizzled: tile t of chunk c = 2 group + kh (the 8 lanes of a
// ds_write_b128 lane group hold the 8 chunks of ONE pixel, i.e. one t) lives in row t ^ c of its block.  Unswizzled, the 8 cells of a
// lane group are 1 KB apart -- one bank, 8 LDS cycles per group, 64 instead of 8 per store, and the four waves' stores kept the LDS busy
// for half of the slab's MFMA time; swizzled they are 8 consecutive 16-byte cells.  The fragment read of (group, kh) reads row (its row)
// ^ c: still one contiguous 512-byte block per 32 lanes, permuted inside aligned groups of 8 rows.  The weight path is each kernel's.
//
// Epilogue, per wave and patch row: the direct kernel's, in its order -- acc_scale, bias, per-image cbias, res, out_scale, act,
// non-temporal stores -- one patch pixel at a time through 32 wave-private staging rows, and the GroupNorm column sums of the row's 64
// pixels (a wave's 32 tiles x one patch row; an image's HW / 64 blocks stay contiguous, which is all ds_gn_finalize assumes), shuffled
// over the 8 lane groups in one fixed order.  The same 64 pixels are one block in every kernel: (m0 >> 6) + a on the 128-pixel tiles,
// (m0 >> 6) + 2 wr + a for wave row wr of the 256-pixel tile.
//
// One workgroup per tile.  A persistent form (one workgroup per compute unit, looping over the tiles b, b + G, ..., the next tile's
// halo and weight requests in front of the epilogue and its halo stores in the epilogue's middle, epilogue staging moved to Vs[1]) was
// built bit-identical and measured: + 1 % per layer by itself, nothing gained by the look-ahead (profiles/wino_persist_ab.txt).  It is
// in no committed source.
//
// conv3x3_wino_kernel (64 x 64)
//   workgroup = 64 tiles (256 output pixels: TH = 256 / W rows, the 256-pixel M tile of the direct kernel) x 64 output channels, four
//               waves (2 x 2), one per SIMD (512 registers); a wave holds ALL 16 positions of its 32 tiles x 32 channels (256
//               accumulator registers), so the output transform is lane-local.
//   halo      = 3 active float4 slots per thread and slab at 16 and 32 columns, 4 at 64.
//   transform = one thread per (tile, channel pair): 16 ds_read_b64, 32 packed adds, 16 ds_write_b64.
//   weights   = the U image of the workgroup's 64 columns (already in the LDS image's order) streams global -> LDS by LDS-DMA into `Us`,
//               doubled like Vs: 4 x 32 KiB + 2 x (NP x 32 + 16) bytes, at most 156 448 bytes of LDS.  The DMA of slab s+1 goes into
//               Us[(s+1) & 1], last read by the MFMAs of slab s-1, and `s_waitcnt vmcnt(0)` stands in front of the barrier (the DMA and
//               the loads have landed; the last slab's redundant DMA too).
//   slots     = 64:  0 ..  7   one LDS-DMA piece of the weights of slab s+1
//                    8 .. 14   the halo loads (one per active slot) and the 3 coefficient loads of slab s+3: ~50 MFMAs ahead of the `vmcnt(0)`
//               and the 8 fragment reads of position group g+1 in slots 8 .. 15 (20 .. 27, 32 .. 39) of group g.
//   skip loop = 256 pixels per slab, eight float4 per thread; the untransformed weights (behind the U images in `wgt`, already in LDS
//               order [group][kh][row][4]) by LDS-DMA into a doubled 8 KB buffer; slot table at the loop.
//
// wino_n128_kernel (32 x 128, four waves).  Every layer on this route has cout % 256 == 0, so on 64-column workgroups FOUR workgroups load
// the same halo, apply the same GroupNorm affine + SiLU to it and run the same input transform: the input side of every slab is computed
// four times, in vector instructions that add their cycles to the MFMAs' (profiles/wino_kloop_ab.txt).  This shape computes it twice:
//   workgroup = 32 tiles (128 output pixels: 128 / W rows x W columns) x 128 output channels, four waves laid out 1 x 4, one per SIMD:
//               every wave takes the SAME 32 tiles and owns 32 of the 128 channels, all 16 positions (256 accumulators, the output
//               transform lane-local).  The workgroup count of a layer is that of the 64 x 64 shape (M / 128 x N / 128).
//   halo      = (128 / W + 2) x (W + 2) pixels: 204 at 32 columns (340 on the 64 x 64 shape), 180 at 16 (324), 264 at 64 (396), i.e. 2
//               active float4 slots per thread and slab at 16 and 32 columns and 3 at 64.
//   transform = 32 tiles x 4 channel pairs = 128 items, each split over TWO threads by rows of B^T d B: a thread reads three rows of d
//               (12 ds_read_b64), makes rows {0, 1} or {2, 3} of B^T d and their eight positions (16 packed adds, 8 ds_write_b64).
//               Which row pair is uniform per wave -- a scalar branch -- and every wave does the same amount: the barrier waits for
//               the slowest.  Each value is made by the 64 x 64 kernel's operations on its operands.
//   weights   = NOT through the LDS.  In the 1 x 4 layout a wave's 32 columns of U belong to that wave alone, so LDS staging would share
//               nothing (and two doubled 64 KiB images would not fit beside V and the halo).  ops.pack_conv_weight_wino stores each
//               (position, kh) as 64 rows x 16 bytes per 64-column image: a wave's B fragment of a position is ONE global_load_dwordx4 per
//               lane, 512 contiguous bytes per kh, from image 2 nt + (wave >> 1), rows 32 (wave & 1) .. + 31 -- no repacking.  The four
//               loads of position group g+1 are issued in the first four slots of group g (group 0 of slab s+1 in group 3 of slab s),
//               16 MFMAs ~ 1 000 cycles ahead of their use, scalar base + 32-bit lane offset.  U is read from L2 at twice the 64 x 64
//               kernel's rate; the workgroups of an XCD walk the slabs together.
//   LDS       = Vs doubled (2 x 16 KiB) and Hs doubled: 44 320 ... 49 696 bytes.
//   order     = NO `vmcnt(0)` in the loop -- every global load targets registers of the wave that uses them, and the compiler's counted
//               waits stand in front of the first use (after the prologue's single `vmcnt(0)` the loop's waits follow from its own
//               order of loads).  Slots: 16 g + 0 .. 3 the B fragments, 4 .. 9 the halo and coefficient loads of slab s+3, 16 g + 10 ..
//               13 the A fragments of group g+1.
//   skip loop = 128 pixels per slab, four float4 per thread, V[0] = Vs[0], V[1] = Vs[1]; the wave's 32 weight columns from global
//               memory into the fragment registers one group ahead.
// What remains redundant: TWO workgroups per M tile (cout = 256: N tiles 0 and 1) still stage and transform the same halo.  A 32 x 256
// workgroup would need 512 accumulators per wave.
//
// wino_w8_kernel (32 x 128, eight waves, two per SIMD).  The fp32 MFMA shares the VALU: one wave per SIMD issues v_mfma_f32_32x32x2_f32
// every 68.7 cycles and pays ~ 5 cycles for every vector instruction beside it; two waves per SIMD issue it every 64.8 cycles and pay
// 3.0 - 3.4 (profiles/r2_probe_mfma_valu.txt).  Tile, packed weights, LDS image and mtiles x ntiles are wino_n128_kernel's:
//   workgroup = 512 threads, eight waves of at most 256 registers.  Wave w owns channel group w & 3 (32 columns, one wave's weight run
//               of the four-wave kernel) and half w >> 2 of the 16 positions: rows i = 2 (w >> 2), + 1 of position 4 i + j, i.e. 8
//               positions x one 32 x 32 block = 128 accumulators.  Per slab and wave 32 MFMAs in two groups of four positions, 8
//               ds_read_b128 of V and 8 global_load_dwordx4 of U one group ahead; per SIMD the MFMA, LDS-read and weight traffic is the
//               four-wave kernel's.
//   halo      = one float4 slot per thread (NP x 2 <= 512 at 16 and 32 columns; 64 columns would need a second slot for 16 threads).
//   transform = the 128 items split over FOUR threads each, by rows of B^T d: a thread reads the two rows of d its row is made of (8
//               ds_read_b64), and makes its row (4 packed adds) and that row's four positions (4 packed adds, 4 ds_write_b64).  Which
//               row is uniform per wave.  Each value is made by the 64 x 64 kernel's operations on its operands.
//   slots     = 16 g + 0 .. 3 the B fragments of the next group (group 0 of slab s+1 in group 1), 4 .. 7 the halo and coefficient loads
//               of slab s+3, 10 .. 13 the A fragments of group 1.  ONE barrier per slab, every wait a counted one.
//   exchange  = behind the last barrier the output transform's first sums run over the row index i, which the pair splits: half 0 finishes
//               patch row 0 = (M[j] + M[4 + j]) + M[8 + j] and needs row 2 of its partner, half 1 finishes patch row 1 = (M[4 + j] -
//               M[8 + j]) - M[12 + j] and needs row 1.  Each wave writes those four accumulators (64 registers per lane, 16 KiB) into
//               its own cells of the LDS and reads its partner's behind ONE barrier: 128 KiB in one round, which is what the launch
//               asks for.  The association of every sum is the lane-local output transform's.
//   skip loop = each wave on the two pixel accumulators of its patch row: 32 MFMAs per slab; two float4 per thread.
//   epilogue  = each wave writes its one patch row; its staging rows lie in the cells the wave itself read in the exchange.
//   OUTSIDE THE LOOPS a workgroup holds the whole compute unit and nothing overlaps it (profiles/wino_outside_ab.txt, wino_outside_isa.txt):
//     prologue  = first what the first loads need (tile decode, the slot's offsets, the bases: WinoHalo's constructor; the weight run), then the
//                 requests of halo 0 and 1 and of the B fragments of (slab 0, group 0), and under their latency the rest: the slot's LDS cell and
//                 zero cells (WinoHalo::cells), the transform's and the fragments' indices.  Divisions by W and W / 2 are shifts, hp / WP is a
//                 multiplication by wino_wp_rcp(W).
//     slab 0    = peeled: K step 0 of each position takes the constant 0 as C, no accumulator is zeroed.  The loop is back(s) (MFMA block,
//                 barrier), exit test, front(s + 1) (transform, halo store).
//     the tail's requests = behind the K loop's last barrier, in front of the exchange's writes: the skip loop's weights of slab 0 and pixels of
//                 slabs 0 and 1, colbias, the cbias row, the eight residual quads.  The exchange reads its partner one accumulator ahead, so
//                 that they fit beside the 128 accumulators.
//     branches  = on the wave's half, p.cbias, p.res, p.act as SCALARS (w8_uni), no selects; half 1's differences packed (w8_sub).
//     addresses = epilogue and residual: a 64-bit scalar base per (pass, patch pixel) plus one 32-bit lane offset per tensor.
#include <type_traits>

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

// `s_waitcnt vmcnt(0)` as the BUILTIN (simm16: vmcnt 0, expcnt 7, lgkmcnt 15), not inline asm: the compiler's own wait-count pass sees it, so it
// knows that the halo registers requested a slab ago are there and does not put a second vmcnt(0) -- which would also wait for the weight DMA
// just issued -- in front of the halo store in the middle of the slab's MFMAs.
#define DS_WINO_WAIT_VM0() do { __builtin_amdgcn_s_waitcnt(0x0F70); asm volatile("" ::: "memory"); } while (0)
#define DS_WINO_WAIT_VM(n) do { __builtin_amdgcn_s_waitcnt(0x0F70 | (n)); asm volatile("" ::: "memory"); } while (0)      // vmcnt(n), n < 16

// unrolling by hand: the slot tables of the kernels take their slot number as a type (DS_WINO_I), one statement per slot
#define DS_WINO_I(n) std::integral_constant<int, (n)>{}
#define DS_WINO_EACH4(F) F(0) F(1) F(2) F(3)
#define DS_WINO_EACH8(F) F(0) F(1) F(2) F(3) F(4) F(5) F(6) F(7)
#define DS_WINO_EACH12(F) F(0) F(1) F(2) F(3) F(4) F(5) F(6) F(7) F(8) F(9) F(10) F(11)
#define DS_WINO_EACH16(F, b) F((b) + 0) F((b) + 1) F((b) + 2) F((b) + 3) F((b) + 4) F((b) + 5) F((b) + 6) F((b) + 7)                \
                             F((b) + 8) F((b) + 9) F((b) + 10) F((b) + 11) F((b) + 12) F((b) + 13) F((b) + 14) F((b) + 15)

// ---- the halo stage (header comment, "Halo stage"): a thread's slots, and a slab's loads and store ------------------------------------------
// NT:    threads per workgroup; slot j of thread tid is (halo pixel (tid + j NT) >> 1, channel quad tid & 1)
// NSH:   slots per thread the launch route can need, NP * 2 <= NSH * NT;  NSL <= NSH: slots that can hold a halo pixel in THIS launch,
//        ceil(2 NP / NT) -- the loads and the store touch no other
// NORM:  the consumer's normalisation on the way into Hs -- 0 none, 1 affine, 2 affine + SiLU (uniform per launch: p.norm, p.norm_act)
// The kernels reach load1 and coef1 from their slot tables through one-line lambdas of their own, not directly: called directly, the
// compiler picks another slot's load for the one offset select it vectorises, and the K loop's instruction order moves.
// conv3x3_wino_kernel keeps a copy of this stage in its body: on this struct its K loop came out with that select on another slot at
// NORM != 0, whichever way the struct was cut (profiles/wino_shared_isa.txt); a fix to this stage has to be made there too.
// r = 65536 / WP + 1 for WP = W + 2 at the widths of this route (powers of two, 4 .. 64: conv3x3_wino_applicable): (hp * r) >> 16 == hp / WP
// for every halo pixel hp < 1024.  10923 at W = 4; 6554, 3641, 1928, 993 at W = 8 .. 64 are the 16-bit fields of one constant, taken
// with a scalar shift (a chain of selects compiled to 40 scalar instructions in front of the first load).  As a field of KParams,
// set by the launcher, it would change igemm_common.h, whose text is hashed into the measured fp16 tile table.
__device__ __forceinline__ int wino_wp_rcp(int W) {
    const int lw = __builtin_ctz(W);
    return lw == 2 ? 10923 : (int)((0x03E107880E39199Aull >> ((16 * (lw - 3)) & 63)) & 0xFFFF);
}

template <int NT, int NSH, int NSL, int NORM>
struct WinoHalo {
    // a slab's halo on its way: the raw pixels of this thread's slots and the slab's coefficient planes {mu, A, B}
    struct Regs {
        f32x4 h[NSH];
        f32x4 mu = {0.f, 0.f, 0.f, 0.f}, ga = {1.f, 1.f, 1.f, 1.f}, be = {0.f, 0.f, 0.f, 0.f};
    };
    const int c0, Ctot;                            // channels of the first source and of both
    const int buf;                                 // floats per buffer of Hs, its spare cell included
    unsigned off0[NSH], off1[NSH];
    int lds[NSH];
    const float *a0i, *a1i;
    const float* cpi;                              // scalar; the lane's channel quad is the byte offset c_lane
    unsigned c_lane;
    float t[4 * NSH], u[4 * NSH];                  // an element chain's affine value and its sigmoid on the way
    // source of a slab: scalar base, and an all-ones / all-zeros word that selects the per-slot offset without a branch (kept opaque)
    const float* h_src = nullptr;
    unsigned h_sel = 0;

    // The slots, fixed for the whole K loop, in two steps so that a kernel can request its first halos between them.  The constructor
    // makes what the LOADS need: element offsets inside the tile's image for either source (an out-of-image pixel: the nearest pixel of
    // the image) and the image's bases.  The halo row of a pixel is hp / WP as a multiplication by wino_wp_rcp(W) (exact for every
    // halo pixel hp < 1024), the image row of the tile comes as r0.
    __device__ __forceinline__ WinoHalo(const KParams& p, int tid, int img0, int r0)
        : c0(p.c0), Ctot(p.c0 + p.c1), buf(p.NP * WINO_K + 4) {
        const int kh_h = tid & 1, wp_rcp = wino_wp_rcp(p.W);
#pragma unroll
        for (int j = 0; j < NSH; ++j) {
            const int hp = (tid + j * NT) >> 1;
            const int hr = (hp * wp_rcp) >> 16, hc = hp - hr * p.WP;
            const int y = r0 + hr - 1, x = hc - 1;
            const int pix = min(max(y, 0), p.H - 1) * p.W + min(max(x, 0), p.W - 1);
            off0[j] = (unsigned)(pix * p.lda0 + kh_h * 4) * 4u;         // BYTES: a load's address is the scalar base plus this 32-bit offset,
            off1[j] = (unsigned)(pix * p.lda1 + kh_h * 4) * 4u;         // with no 64-bit vector arithmetic between the MFMAs
        }
        a0i = p.a0 + (size_t)img0 * p.HW * p.lda0;
        a1i = p.a1 + (size_t)img0 * p.HW * p.lda1;
        cpi = p.norm + (size_t)img0 * 3 * Ctot;
        c_lane = (unsigned)(kh_h * 16);
    }
    // ... and cells() what the STORES need, in front of the first of them: the LDS cell of every slot.  An out-of-image pixel's cell
    // holds zeros in BOTH Hs buffers for the whole tile: this thread writes them here, once, in front of every halo store (the LDS is
    // whatever the workgroup before left), and sends the slot's stores to the spare cell, as it does for a slot beyond the halo.  No
    // other thread writes those cells; the prologue's first barrier publishes them with halo 0 and 1.
    __device__ __forceinline__ void cells(const KParams& p, float* Hs, int tid, int r0) {
        const int kh_h = tid & 1, WPH = p.WP >> 1, wp_rcp = wino_wp_rcp(p.W);
#pragma unroll
        for (int j = 0; j < NSH; ++j) {
            const int hp = (tid + j * NT) >> 1;
            const int hr = (hp * wp_rcp) >> 16, hc = hp - hr * p.WP;
            const int y = r0 + hr - 1, x = hc - 1;
            const bool in = hp < p.NP;
            const bool ok = in && (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W;
            const int cell = (((kh_h * 2 + (hc & 1)) * p.HP + hr) * WPH + (hc >> 1)) * 4;
            lds[j] = ok ? cell : p.NP * WINO_K;
            if (in && !ok) {
                const f32x4 z = {0.f, 0.f, 0.f, 0.f};
                *reinterpret_cast<f32x4*>(Hs + cell) = z;
                *reinterpret_cast<f32x4*>(Hs + buf + cell) = z;
            }
        }
    }
    // the source a0 | a1 of slab s, for the loads that follow
    __device__ __forceinline__ void src(int s) {
        const int c = s * WINO_K;
        const bool first = c < c0;
        h_src = first ? a0i + c : a1i + (c - c0);
        h_sel = (unsigned)__builtin_amdgcn_readfirstlane(first ? -1 : 0);
        asm volatile("" : "+s"(h_sel));
    }
    template <int J>
    __device__ __forceinline__ void load1(Regs& R, std::integral_constant<int, J>) {
        if constexpr (J < NSL) {
            const unsigned off = (off0[J] & h_sel) | (off1[J] & ~h_sel);
            R.h[J] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(h_src) + off);
        }
    }
    // planes {mu, A, B} of the tile's image at slab s, one per call
    template <int I>
    __device__ __forceinline__ void coef1(Regs& R, int s, std::integral_constant<int, I>) {
        if constexpr (NORM != 0) {
            const char* cs = reinterpret_cast<const char*>(cpi + (size_t)I * Ctot + s * WINO_K);
            asm volatile("" : "+v"(c_lane));  // kept 32 bits wide up to the load, which takes the scalar `cs` as its base
            const f32x4 v = *reinterpret_cast<const f32x4*>(cs + c_lane);
            if constexpr (I == 0) R.mu = v; else if constexpr (I == 1) R.ga = v; else R.be = v;
        }
    }
    // every load of slab s, in the order the prologues request them
    __device__ __forceinline__ void loads(Regs& R, int s) {
#define DS_WINO_F(j) load1(R, DS_WINO_I(j));
        DS_WINO_EACH4(DS_WINO_F)
#undef DS_WINO_F
        coef1(R, s, DS_WINO_I(0)); coef1(R, s, DS_WINO_I(1)); coef1(R, s, DS_WINO_I(2));
    }
    // stage ST of element chain C (slot C / 4, float C % 4) of the halo store into the buffer `hs` of Hs: the consumer's GroupNorm affine
    // + SiLU, applied once per element (an out-of-image pixel's value goes to the spare cell; its own cell holds zeros).  The affine
    // is a subtraction and ONE fma, the SiLU is ds_silu's operations.
    template <int C, int ST>
    __device__ __forceinline__ void chain(Regs& R, float* hs) {
        constexpr int j = C >> 2, e = C & 3;
        if constexpr (j < NSL) {
            if constexpr (ST == 0 && NORM != 0) {
                t[C] = __builtin_fmaf(R.h[j][e] - R.mu[e], R.ga[e], R.be[e]);
                if constexpr (NORM == 2) u[C] = __expf(-t[C]);
            }
            if constexpr (ST == 1 && NORM == 2) u[C] = __builtin_amdgcn_rcpf(1.0f + u[C]);
            if constexpr (ST == 2) {
                float v = R.h[j][e];
                if constexpr (NORM == 1) v = t[C];
                if constexpr (NORM == 2) v = t[C] * u[C];
                R.h[j][e] = v;
                if constexpr (e == 3) *reinterpret_cast<f32x4*>(hs + lds[j]) = R.h[j];
            }
        }
    }
    // the halo store of a slab: every chain of every active slot, three stages each
    __device__ __forceinline__ void store(Regs& R, float* hs) {
#define DS_WINO_F(c) chain<c, 0>(R, hs); chain<c, 1>(R, hs); chain<c, 2>(R, hs);
        DS_WINO_EACH16(DS_WINO_F, 0)
#undef DS_WINO_F
    }
};

// ---- skip-slab staging (header comment, "Skip slabs"): a thread's cells of a V buffer, the swizzled fragment offsets, a slab's source -------
// NT:    threads per workgroup: 8 threads (chunks of 4 channels) per pixel, so slot j of thread tid is pixel (tid >> 3) + j NT / 8 of the tile
// ROWS:  tiles per V block, 64 or 32: the tile is 4 ROWS pixels, NE = 32 ROWS / NT slots per thread
template <int NT, int ROWS>
struct WinoSkip {
    static constexpr int STEP = NT / 8, NE = 4 * ROWS / STEP;
    int lds[NE];                                   // V cell of slot j: [patch pixel][8-channel group][kh][tile ^ chunk][4]
    int a_off[4];                                  // fragment offset of group g in a patch pixel's block, swizzled: row ^ (2 g + kh)
    unsigned t_pix, t_e4;                          // pixel of slot 0 and the thread's channel chunk: slot 0 is element t_pix * ld + t_e4 of e0 | e1; a slot steps STEP rows
    const float* src = nullptr;
    unsigned off = 0;
    int step = 0;

    // row0: the first of the 32 tiles whose fragments this wave reads
    __device__ __forceinline__ WinoSkip(const KParams& p, int tid, int lane, int row0) { setup(p, tid, lane, row0); }
    // for a kernel that sets its slots up only where the launch has skip slabs
    __device__ __forceinline__ WinoSkip() {}
    __device__ __forceinline__ void setup(const KParams& p, int tid, int lane, int row0) {
        setup_loads(p, tid);
        setup_cells(p, tid, lane, row0);
    }
    // what the loads need ...
    __device__ __forceinline__ void setup_loads(const KParams& p, int tid) {
        const int e_chunk = tid & 7;                   // channels 4 e_chunk .. + 3 of the slab: group e_chunk >> 1, kh = e_chunk & 1
        t_pix = (unsigned)(tid >> 3);
        t_e4 = (unsigned)(e_chunk * 4);
    }
    // ... and what the stores and the fragment reads need
    __device__ __forceinline__ void setup_cells(const KParams& p, int tid, int lane, int row0) {
        const int e_chunk = tid & 7, Wt = p.W >> 1;
        const int lw = __builtin_ctz(p.W);             // every width on this route is a power of two (conv3x3_wino_applicable)
#pragma unroll
        for (int j = 0; j < NE; ++j) {
            const int lp = (tid >> 3) + STEP * j;      // pixel of the tile
            const int yl = lp >> lw, x = lp & (p.W - 1);
            const int ph = (yl & 1) * 2 + (x & 1), t = (yl >> 1) * Wt + (x >> 1);
            lds[j] = (((ph * 4 + (e_chunk >> 1)) * 2 + (e_chunk & 1)) * ROWS + (t ^ e_chunk)) * 4;
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) a_off[g] = ((lane >> 5) * ROWS + ((row0 + (lane & 31)) ^ (2 * g + (lane >> 5)))) * 4;
    }
    // the source e0 | e1 of slab es of the tile at output row m0, for the loads that follow
    __device__ __forceinline__ void sel(const KParams& p, int es, int m0) {
        const int c = es * 32;
        const bool first = c < p.ec0;
        const int ld = first ? p.elda0 : p.elda1;
        src = (first ? p.e0 + c : p.e1 + (c - p.ec0)) + (size_t)m0 * ld;
        step = STEP * ld;
        off = __umul24(t_pix, (unsigned)ld) + t_e4;    // one v_mad_u32_u24 on the scalar row step (a row step is far below 2^24 floats)
    }
    template <int J>
    __device__ __forceinline__ void load1(f32x4* dst, std::integral_constant<int, J>) {
        dst[J] = *reinterpret_cast<const f32x4*>(src + (size_t)(J * step) + off);
    }
};

// ---- launching: one kernel instantiation on one workgroup of NT threads per tile, and the choice of NORM, which every kernel takes as a
// template argument (nothing in the K loop branches on it)
template <auto KERNEL, int NT, int LDS_MAX>
int wino_launch(KParams& p, int smem, hipStream_t stream) {
    DS_ENSURE_DYN_LDS(KERNEL, LDS_MAX);
    hipLaunchKernelGGL(KERNEL, dim3(grid_1d(p.mtiles, p.ntiles)), dim3(NT), smem, stream, p);
    DS_CHECK_LAUNCH();
    return DS_OK;
}

template <typename F>
int wino_by_norm(const KParams& p, F launch) {
    if (!p.norm) return launch(DS_WINO_I(0));
    return p.norm_act == DS_ACT_SILU ? launch(DS_WINO_I(2)) : launch(DS_WINO_I(1));
}

// ---- conv3x3_wino_kernel: 64 tiles x 64 channels (header comment) --------------------------------------------------------------------------
// VAR: the timing ablations (0 in the product).  NORM, NSL: WinoHalo's; NSL = 3 for 16- and 32-column images, 4 for 64-column ones
template <int VAR, int NORM, int NSL>
__global__ void __launch_bounds__(256, 1) conv3x3_wino_kernel(const KParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Us = smem;                              // [2][16][2][64][4]
    float* Vs = smem + 2 * WINO_IMG;               // [2][16][2][64][4]
    float* Hs = smem + 4 * WINO_IMG;               // [2] x { [2][2][HP][WP / 2][4], and one spare 16-byte cell behind it }

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
    constexpr bool kDma = !(VAR & WV_NO_DMA), kHalo = !(VAR & WV_NO_HALO);

    // ---- halo stage: WinoHalo's, kept as this kernel's own copy (WinoHalo's comment says why), on 256 threads and WINO_NSH slots ------------
    constexpr int kNorm = (VAR & WV_NO_NORM) ? 0 : NORM;       // the arithmetic of the halo store; the ablation keeps the coefficient loads
    const int kh_h = tid & 1;
    const int h_buf = p.NP * WINO_K + 4;           // floats per buffer of Hs, its spare cell included
    unsigned h_off0[WINO_NSH], h_off1[WINO_NSH];
    int h_lds[WINO_NSH];
#pragma unroll
    for (int j = 0; j < WINO_NSH; ++j) {
        const int hp = (tid + j * 256) >> 1;
        const int hr = hp / p.WP, hc = hp - hr * p.WP;
        const int y = r0 + hr - 1, x = hc - 1;
        const bool in = hp < p.NP;
        const bool ok = in && (unsigned)y < (unsigned)p.H && (unsigned)x < (unsigned)p.W;
        const int pix = min(max(y, 0), p.H - 1) * p.W + min(max(x, 0), p.W - 1);
        h_off0[j] = (unsigned)(pix * p.lda0 + kh_h * 4) * 4u;       // BYTES: a load's address is the scalar base plus this 32-bit offset,
        h_off1[j] = (unsigned)(pix * p.lda1 + kh_h * 4) * 4u;       // with no 64-bit vector arithmetic between the MFMAs
        const int cell = (((kh_h * 2 + (hc & 1)) * p.HP + hr) * WPH + (hc >> 1)) * 4;
        h_lds[j] = ok ? cell : p.NP * WINO_K;
        if (in && !ok) {
            const f32x4 z = {0.f, 0.f, 0.f, 0.f};
            *reinterpret_cast<f32x4*>(Hs + cell) = z;
            *reinterpret_cast<f32x4*>(Hs + h_buf + cell) = z;
        }
    }
    const float* a0i = p.a0 + (size_t)img0 * p.HW * p.lda0;
    const float* a1i = p.a1 + (size_t)img0 * p.HW * p.lda1;
    const float* cpi = p.norm + (size_t)img0 * 3 * Ctot;       // scalar; the lane's channel quad is the byte offset c_lane
    unsigned c_lane = (unsigned)(kh_h * 16);
    // a slab's halo on its way: the raw pixels of this thread's slots and the slab's coefficient planes {mu, A, B}
    struct HaloRegs {
        f32x4 h[WINO_NSH];
        f32x4 mu = {0.f, 0.f, 0.f, 0.f}, ga = {1.f, 1.f, 1.f, 1.f}, be = {0.f, 0.f, 0.f, 0.f};
    };
    HaloRegs hreg;
    float h_t[4 * WINO_NSH], h_u[4 * WINO_NSH];    // an element chain's affine value and its sigmoid on the way
    // source of slab s: scalar base, and an all-ones / all-zeros word that selects the per-slot offset without a branch (kept opaque)
    const float* h_src = nullptr;
    unsigned h_sel = 0;
    auto halo_src = [&](int s) {
        const int c = s * WINO_K;
        const bool first = c < p.c0;
        h_src = first ? a0i + c : a1i + (c - p.c0);
        h_sel = (unsigned)__builtin_amdgcn_readfirstlane(first ? -1 : 0);
        asm volatile("" : "+s"(h_sel));
    };
    auto halo_load1 = [&](HaloRegs& R, auto J) {
        constexpr int j = decltype(J)::value;
        if constexpr (j >= NSL) return;
        const unsigned off = (h_off0[j] & h_sel) | (h_off1[j] & ~h_sel);
        R.h[j] = *reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(h_src) + off);
    };
    // planes {mu, A, B} of the tile's image, one per call
    auto coef_load1 = [&](HaloRegs& R, int s, auto I) {
        constexpr int i = decltype(I)::value;
        if constexpr (NORM != 0) {
            const char* cs = reinterpret_cast<const char*>(cpi + (size_t)i * Ctot + s * WINO_K);
            asm volatile("" : "+v"(c_lane));  // kept 32 bits wide up to the load, which takes the scalar `cs` as its base
            const f32x4 v = *reinterpret_cast<const f32x4*>(cs + c_lane);
            if constexpr (i == 0) R.mu = v; else if constexpr (i == 1) R.ga = v; else R.be = v;
        }
    };
    // stage ST of element chain C (slot C / 4, float C % 4) of the halo store into the buffer `hs` of Hs: the consumer's GroupNorm affine
    // + SiLU, applied once per element (an out-of-image pixel's value goes to the spare cell; its own cell holds zeros).  The affine
    // is a subtraction and ONE fma, the SiLU is ds_silu's operations.
    auto halo_chain = [&](HaloRegs& R, float* hs, auto C, auto ST) {
        constexpr int c = decltype(C)::value, st = decltype(ST)::value, j = c >> 2, e = c & 3;
        if constexpr (j >= NSL) return;
        if constexpr (st == 0 && kNorm != 0) {
            h_t[c] = __builtin_fmaf(R.h[j][e] - R.mu[e], R.ga[e], R.be[e]);
            if constexpr (kNorm == 2) h_u[c] = __expf(-h_t[c]);
        }
        if constexpr (st == 1 && kNorm == 2) h_u[c] = __builtin_amdgcn_rcpf(1.0f + h_u[c]);
        if constexpr (st == 2) {
            float v = R.h[j][e];
            if constexpr (kNorm == 1) v = h_t[c];
            if constexpr (kNorm == 2) v = h_t[c] * h_u[c];
            R.h[j][e] = v;
            if constexpr (e == 3) *reinterpret_cast<f32x4*>(hs + h_lds[j]) = R.h[j];
        }
    };

    // ---- input transform: this thread owns (tile t_t, channels 4 kh_t + 2 cpl .. + 1) -----------------------------------------------
    const int t_t = (tid >> 1) & 63, cpl = tid & 1, kh_t = tid >> 7;
    const int t_ty = t_t / Wt, t_tx = t_t - t_ty * Wt;
    const int h_rd = ((kh_t * 2 * p.HP + 2 * t_ty) * WPH + t_tx) * 4 + cpl * 2;         // float offsets inside a buffer of Hs / of Vs
    const int h_par = p.HP * WPH * 4;              // odd-column plane
    const int v_wr = (kh_t * 64 + t_t) * 4 + cpl * 2;
    // in 16 + 16 pieces, so that the K loop can place them: piece I of the reads is d[I / 4][I % 4], piece I of the writes is position I
    // (row I / 4 of B^T d, made when its first position is written: it needs rows 0,2 / 1,2 / 1,2 / 1,3 of d)
    f32x2 t_d[4][4], t_r[4];
    auto tr_read1 = [&](const float* hs, auto I) {
        constexpr int i = decltype(I)::value >> 2, j = decltype(I)::value & 3;
        t_d[i][j] = *reinterpret_cast<const f32x2*>(hs + h_rd + (j & 1) * h_par + i * WPH * 4 + (j >> 1) * 4);
    };
    auto tr_write1 = [&](float* vs, auto I) {
        constexpr int i = decltype(I)::value >> 2, j = decltype(I)::value & 3;
        if constexpr (j == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q)            // B^T d
                t_r[q] = i == 0 ? t_d[0][q] - t_d[2][q] : i == 1 ? t_d[1][q] + t_d[2][q] : i == 2 ? t_d[2][q] - t_d[1][q] : t_d[1][q] - t_d[3][q];
        }
        const f32x2 v = j == 0 ? t_r[0] - t_r[2] : j == 1 ? t_r[1] + t_r[2] : j == 2 ? t_r[2] - t_r[1] : t_r[1] - t_r[3];     // (B^T d) B
        *reinterpret_cast<f32x2*>(vs + v_wr + (i * 4 + j) * WINO_POS) = v;
    };

    // ---- transformed weights -> a buffer of Us: 8 LDS-DMA pieces per wave, source already in the LDS image's order -------------------------
    const float* u_src = p.b + (size_t)nt * nslabs * WINO_IMG;                         // scalar; the lane's piece of a DMA is the byte offset tid * 16
    unsigned u_lane = (unsigned)tid * 16u;
    auto u_dma1 = [&](const float* src, float* ubuf, auto I) {                          // src: u_src + slab * WINO_IMG
        constexpr int i = decltype(I)::value;
        float* dst = ubuf + (i * 256 + wave * 64) * 4;                                  // wave-uniform base; the DMA writes lane-linear
        typedef const __attribute__((address_space(1))) void* gptr_t;
        typedef __attribute__((address_space(3))) void* lptr_t;
        const char* us = reinterpret_cast<const char*>(src + i * 1024);
        asm volatile("" : "+s"(us));          // kept scalar: the DMA takes it as its base ...
        asm volatile("" : "+v"(u_lane));     // ... and the offset 32 bits wide up to the load
        __builtin_amdgcn_global_load_lds((gptr_t)(us + u_lane), (lptr_t)(dst), 16, 0, 0);
    };

    f32x16 acc[16];
#pragma unroll
    for (int q = 0; q < 16; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
    const int a_off = ((lane >> 5) * 64 + wr * 32 + (lane & 31)) * 4;
    const int b_off = ((lane >> 5) * 64 + wc * 32 + (lane & 31)) * 4;

#define DS_WINO_LOADS(R, sl)                                                                                                           \
    halo_load1(R, DS_WINO_I(0)); halo_load1(R, DS_WINO_I(1)); halo_load1(R, DS_WINO_I(2)); halo_load1(R, DS_WINO_I(3));                \
    coef_load1(R, sl, DS_WINO_I(0)); coef_load1(R, sl, DS_WINO_I(1)); coef_load1(R, sl, DS_WINO_I(2));

    // ---- prologue: halo 0 and 1 and transform 0 staged, halo 2 requested (two barriers) ------------------------------------------------
    halo_src(0);
    DS_WINO_LOADS(hreg, 0)
    {
        HaloRegs hreg1;                                // slab 1, requested behind slab 0 so that the two latencies overlap
        const int s1 = min(1, nslabs - 1);
        halo_src(s1);
        DS_WINO_LOADS(hreg1, s1)
        DS_RACE_SKEW(wave);
#define DS_WINO_F(i) u_dma1(u_src, Us, DS_WINO_I(i)); u_dma1(u_src, Us, DS_WINO_I((i) + 4));
        DS_WINO_EACH4(DS_WINO_F)
#undef DS_WINO_F
        DS_RACE_SKEW(wave);
#define DS_WINO_CHAIN1(c) halo_chain(hreg, Hs, DS_WINO_I(c), DS_WINO_I(0)); halo_chain(hreg, Hs, DS_WINO_I(c), DS_WINO_I(1));          \
                          halo_chain(hreg, Hs, DS_WINO_I(c), DS_WINO_I(2));
        DS_WINO_EACH16(DS_WINO_CHAIN1, 0)
#undef DS_WINO_CHAIN1
        DS_RACE_SKEW(wave);
#define DS_WINO_CHAIN1(c) halo_chain(hreg1, Hs + h_buf, DS_WINO_I(c), DS_WINO_I(0)); halo_chain(hreg1, Hs + h_buf, DS_WINO_I(c), DS_WINO_I(1)); \
                          halo_chain(hreg1, Hs + h_buf, DS_WINO_I(c), DS_WINO_I(2));
        DS_WINO_EACH16(DS_WINO_CHAIN1, 0)
#undef DS_WINO_CHAIN1
    }
    {
        const int s2 = min(2, nslabs - 1);
        halo_src(s2);
        DS_WINO_LOADS(hreg, s2)
    }
    __syncthreads();                                   // Hs[0], Hs[1] published
#define DS_WINO_F(i) tr_read1(Hs, DS_WINO_I(i));
    DS_WINO_EACH16(DS_WINO_F, 0)
#undef DS_WINO_F
    DS_RACE_SKEW(wave);
#define DS_WINO_F(i) tr_write1(Vs, DS_WINO_I(i));
    DS_WINO_EACH16(DS_WINO_F, 0)
#undef DS_WINO_F
    DS_WINO_WAIT_VM0();
    __syncthreads();                                   // Vs[0], Us[0] published; the halo of slab 2 is in its registers

    // ---- K loop: ONE barrier per slab -----------------------------------------------------------------------------------------------------
    // fragments of position group g (positions 4 g .. 4 g + 3) live in fa / fb[g & 1]; group g+1 is read in slots FR(g) .. FR(g) + 7 of
    // group g (behind the DMA pieces in group 0)
    f32x4 fa[2][4], fb[2][4];
    int s = 0;
    do {                                               // nslabs >= 1 (conv3x3_wino_applicable)
        const int par = s & 1;
        const float* ub = Us + par * WINO_IMG;
        const float* vb = Vs + par * WINO_IMG;
        float* ubn = Us + (par ^ 1) * WINO_IMG;        // last read by the MFMAs of slab s-1 (barrier s-1 passed)
        float* vbn = Vs + (par ^ 1) * WINO_IMG;        // likewise
        float* hb = Hs + par * h_buf;                  // last read by the transform of slab s, in front of barrier s-1
        const float* hbn = Hs + (par ^ 1) * h_buf;     // the halo of slab s+1, published at barrier s-1
        const int s1 = min(s + 1, nslabs - 1), s3 = min(s + 3, nslabs - 1);
        const float* un = u_src + (size_t)s1 * WINO_IMG;
        auto frag_read = [&](auto G, auto I) {
            constexpr int g = decltype(G)::value, i = decltype(I)::value;
            if constexpr (i < 4) fa[g & 1][i] = *reinterpret_cast<const f32x4*>(vb + (g * 4 + i) * WINO_POS + a_off);
            else fb[g & 1][i - 4] = *reinterpret_cast<const f32x4*>(ub + (g * 4 + i - 4) * WINO_POS + b_off);
        };
#define DS_WINO_F(i) tr_read1(hbn, DS_WINO_I(i));         // transform of slab s+1, first half: Hs[par ^ 1] -> registers
        DS_WINO_EACH16(DS_WINO_F, 0)
#undef DS_WINO_F
        if constexpr (kHalo) {                         // halo of slab s+2 (its loads were issued a slab ago, landed at barrier s-1)
            DS_RACE_SKEW(wave);
#define DS_WINO_CHAIN1(c) halo_chain(hreg, hb, DS_WINO_I(c), DS_WINO_I(0)); halo_chain(hreg, hb, DS_WINO_I(c), DS_WINO_I(1));          \
                          halo_chain(hreg, hb, DS_WINO_I(c), DS_WINO_I(2));
            DS_WINO_EACH16(DS_WINO_CHAIN1, 0)
#undef DS_WINO_CHAIN1
            halo_src(s3);
        }
        DS_RACE_SKEW(wave);
#define DS_WINO_F(i) tr_write1(vbn, DS_WINO_I(i));        // second half: its adds, registers -> Vs[par ^ 1]
        DS_WINO_EACH16(DS_WINO_F, 0)
#undef DS_WINO_F
        auto fill = [&](auto K) {
            constexpr int k = decltype(K)::value, g = k >> 4;
            if constexpr (k < 8) {                     // weights of slab s+1
                if constexpr (kDma) {
                    if constexpr (k == 0) DS_RACE_SKEW(wave);
                    u_dma1(un, ubn, DS_WINO_I(k));
                }
            } else if constexpr (k < 12) {             // loads of slab s+3: they land at the barrier (vmcnt(0) for the weight DMA)
                if constexpr (kHalo) halo_load1(hreg, DS_WINO_I(k - 8));
            } else if constexpr (k < 15) {
                if constexpr (kHalo) coef_load1(hreg, s3, DS_WINO_I(k - 12));
            }
            constexpr int fr = g == 0 ? 8 : g == 1 ? 20 : g == 2 ? 32 : 64;
            if constexpr (k >= fr && k < fr + 8) frag_read(DS_WINO_I(g + 1), DS_WINO_I(k - fr));
        };
        // micro-slot k: K step r = (k >> 2) & 3 of position 4 (k >> 4) + (k & 3), then its fillers, pinned
#define DS_WINO_STEP(k)                                                                                                                \
        acc[((k) >> 4) * 4 + ((k) & 3)] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[((k) >> 4) & 1][(k) & 3][((k) >> 2) & 3],            \
                                                                               fb[((k) >> 4) & 1][(k) & 3][((k) >> 2) & 3],            \
                                                                               acc[((k) >> 4) * 4 + ((k) & 3)], 0, 0, 0);              \
        fill(DS_WINO_I(k));                                                                                                            \
        __builtin_amdgcn_sched_barrier(0);
#define DS_WINO_F(i) frag_read(DS_WINO_I(0), DS_WINO_I(i)); frag_read(DS_WINO_I(0), DS_WINO_I((i) + 4));
        DS_WINO_EACH4(DS_WINO_F)
#undef DS_WINO_F
        __builtin_amdgcn_sched_barrier(0);
        DS_WINO_EACH16(DS_WINO_STEP, 0)
        DS_WINO_EACH16(DS_WINO_STEP, 16)
        DS_WINO_EACH16(DS_WINO_STEP, 32)
        DS_WINO_EACH16(DS_WINO_STEP, 48)
#undef DS_WINO_STEP
        DS_WINO_WAIT_VM0();                            // the LDS-DMA of slab s+1 has landed (hipcc waits only in front of LDS reads it can tie to it)
        __syncthreads();                               // slab s done: Vs[par], Us[par] dead; Vs, Us and Hs [par ^ 1] published
    } while (++s < nslabs);
#undef DS_WINO_LOADS

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

    // ---- appended 1x1 slabs (header comment, "Skip slabs"): 256 pixels x 32 channels per slab through a V buffer, the untransformed weights
    // (behind the U images in `wgt`, already in LDS order [group][kh][row][4]) by LDS-DMA into a weight buffer.  Every LDS buffer of the K
    // loop died at its last barrier (its clamped redundant DMA landed at the `vmcnt(0)` in front of it, its redundant transform wrote a Vs
    // buffer in front of it, and the redundant halo store went to Hs, which this loop does not touch), so both are doubled inside the
    // first three images:
    //     W[b] = smem + b * 2048 (8 KB each, the first half of Us[0]),   V[0] = Vs[0],   V[1] = Us[1]
    // Between barrier es-1 and barrier es, one basic block of 64 micro-slots: the MFMAs of slab es on V[es & 1] and W[es & 1], and
    //     slots  0 ..  1   the two LDS-DMA pieces of the weights of slab es+1 -> W[(es+1) & 1]   (last read by slab es-1)
    //     slots  2 ..  6   (24 .. 28, 36 .. 40 of groups 1, 2) the five fragment reads of group g+1
    //     slots  7 .. 14   the eight ds_write_b128 of the pixels of slab es+1, registers -> V[(es+1) & 1]   (last read by slab es-1; the
    //                      registers were requested a slab ago and landed at the `vmcnt(0)` in front of barrier es-1)
    //     slots 15 .. 22   the eight global loads of slab es+2 into the registers just stored: ~40 MFMAs ahead of the `vmcnt(0)`
    // The last slab's redundant DMA, store and loads have all landed at its barrier, behind which the epilogue reuses smem from offset 0.
    const int nextra = (p.ec0 + p.ec1) / 32;
    if (nextra > 0) {
        const float* wsk = p.b + (size_t)p.ntiles * nslabs * WINO_IMG + (size_t)nt * nextra * 2048 + tid * 4;
        WinoSkip<256, 64> skip(p, tid, lane, wr * 32);
        auto e_load1 = [&](f32x4* dst, auto J) { skip.load1(dst, J); };
        auto w_dma1 = [&](int es, float* wbuf, auto I) {
            constexpr int i = decltype(I)::value;
            float* dst = wbuf + (i * 256 + wave * 64) * 4;
            typedef const __attribute__((address_space(1))) void* gptr_t;
            typedef __attribute__((address_space(3))) void* lptr_t;
            __builtin_amdgcn_global_load_lds((gptr_t)(wsk + (size_t)es * 2048 + i * 1024), (lptr_t)(dst), 16, 0, 0);
        };

        // prologue: weights and pixels of slab 0 staged, pixels of slab 1 requested behind them
        f32x4 ereg[8];
        {
            f32x4 ereg0[8];
            DS_RACE_SKEW(wave);
            w_dma1(0, smem, DS_WINO_I(0)); w_dma1(0, smem, DS_WINO_I(1));
            skip.sel(p, 0, m0);
#define DS_WINO_F(j) e_load1(ereg0, DS_WINO_I(j));
            DS_WINO_EACH8(DS_WINO_F)
#undef DS_WINO_F
            skip.sel(p, min(1, nextra - 1), m0);
#define DS_WINO_F(j) e_load1(ereg, DS_WINO_I(j));
            DS_WINO_EACH8(DS_WINO_F)
#undef DS_WINO_F
            DS_WINO_WAIT_VM(8);                        // all but the eight loads of slab 1
            DS_RACE_SKEW(wave);
#pragma unroll
            for (int j = 0; j < 8; ++j) *reinterpret_cast<f32x4*>(Vs + skip.lds[j]) = ereg0[j];
        }
        __syncthreads();

        f32x4 ga[2][4], gb[2];                         // fragments of group g: the four patch pixels' pixels and the weights
        int es = 0;
        do {
            const float* vb = smem + (2 - (es & 1)) * WINO_IMG;
            float* vn = smem + (1 + (es & 1)) * WINO_IMG;
            const float* wb = smem + (es & 1) * 2048;
            float* wn = smem + ((es + 1) & 1) * 2048;
            const int es1 = min(es + 1, nextra - 1);
            skip.sel(p, min(es + 2, nextra - 1), m0);
            auto frag_read = [&](auto G, auto I) {
                constexpr int g = decltype(G)::value, i = decltype(I)::value;
                if constexpr (i < 4) ga[g & 1][i] = *reinterpret_cast<const f32x4*>(vb + (i * 4 + g) * WINO_POS + skip.a_off[g]);
                else gb[g & 1] = *reinterpret_cast<const f32x4*>(wb + g * WINO_POS + b_off);
            };
            auto fill = [&](auto K) {
                constexpr int k = decltype(K)::value, g = k >> 4;
                if constexpr (k < 2) {                 // weights of slab es+1
                    if constexpr (k == 0) DS_RACE_SKEW(wave);
                    w_dma1(es1, wn, DS_WINO_I(k));
                } else if constexpr (k >= 7 && k < 15) {   // pixels of slab es+1
                    if constexpr (k == 7) DS_RACE_SKEW(wave);
                    *reinterpret_cast<f32x4*>(vn + skip.lds[k - 7]) = ereg[k - 7];
                } else if constexpr (k >= 15 && k < 23) {  // loads of slab es+2
                    e_load1(ereg, DS_WINO_I(k - 15));
                }
                constexpr int fr = g == 0 ? 2 : g == 1 ? 24 : g == 2 ? 36 : 64;
                if constexpr (k >= fr && k < fr + 5) frag_read(DS_WINO_I(g + 1), DS_WINO_I(k - fr));
            };
            // micro-slot k: K step r = (k >> 2) & 3 of group k >> 4 into patch pixel k & 3, then its filler, pinned
#define DS_WINO_STEP(k)                                                                                                                \
            Y[(k) & 3] = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[((k) >> 4) & 1][(k) & 3][((k) >> 2) & 3], gb[((k) >> 4) & 1][((k) >> 2) & 3], \
                                                              Y[(k) & 3], 0, 0, 0);                                                    \
            fill(DS_WINO_I(k));                                                                                                        \
            __builtin_amdgcn_sched_barrier(0);
            frag_read(DS_WINO_I(0), DS_WINO_I(0)); frag_read(DS_WINO_I(0), DS_WINO_I(4)); frag_read(DS_WINO_I(0), DS_WINO_I(1));
            frag_read(DS_WINO_I(0), DS_WINO_I(2)); frag_read(DS_WINO_I(0), DS_WINO_I(3));
            __builtin_amdgcn_sched_barrier(0);
            DS_WINO_EACH16(DS_WINO_STEP, 0)
            DS_WINO_EACH16(DS_WINO_STEP, 16)
            DS_WINO_EACH16(DS_WINO_STEP, 32)
            DS_WINO_EACH16(DS_WINO_STEP, 48)
#undef DS_WINO_STEP
            DS_WINO_WAIT_VM0();                        // the weights of slab es+1 and the pixels of slab es+2 have landed
            __syncthreads();                           // V[es & 1], W[es & 1] dead; V[(es+1) & 1], W[(es+1) & 1] published
        } while (++es < nextra);
    }

    // ---- the fused epilogue, one patch pixel (a, b) at a time ----------------------------------------------------------------------------
    float* stage = smem + wave * 32 * WINO_EPI_LD;     // wave-private rows; every LDS buffer died at the last barrier
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

// ---- wino_n128_kernel: 32 tiles x 128 output channels on four waves (header comment) ----------------------------------------------------------
constexpr int WN_POS = 2 * 32 * 4;                // floats per position of a V image of 32 tiles
constexpr int WN_IMG = 16 * WN_POS;               // floats per V image (4096)
constexpr int WN_NSH = 3;                         // halo float4 slots per thread: NP * 2 <= 768

// NORM, NSL: WinoHalo's; NSL = 2 for 16- and 32-column images (NP = 180, 204), 3 for 64-column ones (NP = 264)
template <int NORM, int NSL>
__global__ void __launch_bounds__(256, 1) wino_n128_kernel(const KParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Vs = smem;                              // [2][16][2][32][4]
    float* Hs = smem + 2 * WN_IMG;                 // [2] x { [2][2][HP][WP / 2][4], and one spare 16-byte cell behind it }

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int mt, nt;
    if (!decode_tile(blockIdx.x, p.mtiles, p.ntiles, mt, nt)) return;
    const int m0 = mt * 128, n0 = nt * 128;
    const int img0 = m0 / p.HW;
    const int r0 = (m0 - img0 * p.HW) / p.W;
    const int WPH = p.WP >> 1, Wt = p.W >> 1;
    const int Ctot = p.c0 + p.c1;
    const int nslabs = Ctot / WINO_K;

    // ---- halo stage: NSL of three float4 slots per thread -----------------------------------------------------------------------------------
    using Halo = WinoHalo<256, WN_NSH, NSL, NORM>;
    Halo halo(p, tid, img0, r0);
    halo.cells(p, Hs, tid, r0);
    const int h_buf = halo.buf;
    typename Halo::Regs hreg;
    auto halo_load1 = [&](typename Halo::Regs& R, auto J) { halo.load1(R, J); };
    auto coef_load1 = [&](typename Halo::Regs& R, int sl, auto I) { halo.coef1(R, sl, I); };

    // ---- input transform: 32 tiles x 4 channel pairs, each split over two threads by rows of B^T d B.  A thread owns (tile t_t, channels
    // 4 kh_t + 2 cpl .. + 1, rows 2 half, 2 half + 1): it reads the rows half .. half + 2 of d and writes eight positions.  kh_t and half
    // are uniform per wave (wave = kh_t + 2 half), so the choice between the two row pairs is a scalar branch and every wave issues the
    // same count of instructions.  Every value is made by the 64 x 64 kernel's operations on the same operands.
    const int t_t = (tid >> 1) & 31, cpl = tid & 1, kh_t = wave & 1, half = wave >> 1;
    const int t_ty = t_t / Wt, t_tx = t_t - t_ty * Wt;
    const int h_rd = ((kh_t * 2 * p.HP + 2 * t_ty + half) * WPH + t_tx) * 4 + cpl * 2;
    const int h_par = p.HP * WPH * 4;              // odd-column plane
    const int v_wr = (kh_t * 32 + t_t) * 4 + cpl * 2 + half * 8 * WN_POS;
    f32x2 t_e[3][4];
    auto tr_read1 = [&](const float* hs, auto I) {             // piece I = row I / 4 (of this thread's three), column I % 4
        constexpr int i = decltype(I)::value >> 2, j = decltype(I)::value & 3;
        t_e[i][j] = *reinterpret_cast<const f32x2*>(hs + h_rd + (j & 1) * h_par + i * WPH * 4 + (j >> 1) * 4);
    };
    auto tr_write = [&](float* vs) {
        f32x2 ra[4], rb[4];
        if (half == 0) {                           // rows 0, 1 of B^T d: d0 - d2, d1 + d2
#pragma unroll
            for (int q = 0; q < 4; ++q) { ra[q] = t_e[0][q] - t_e[2][q]; rb[q] = t_e[1][q] + t_e[2][q]; }
        } else {                                   // rows 2, 3: d2 - d1, d1 - d3
#pragma unroll
            for (int q = 0; q < 4; ++q) { ra[q] = t_e[1][q] - t_e[0][q]; rb[q] = t_e[0][q] - t_e[2][q]; }
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const f32x2* t_r = i == 0 ? ra : rb;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x2 v = j == 0 ? t_r[0] - t_r[2] : j == 1 ? t_r[1] + t_r[2] : j == 2 ? t_r[2] - t_r[1] : t_r[1] - t_r[3];     // (B^T d) B
                *reinterpret_cast<f32x2*>(vs + v_wr + (i * 4 + j) * WN_POS) = v;
            }
        }
    };

    // ---- transformed weights: global -> the B fragment registers.  The wave's 32 columns are rows 32 (wave & 1) .. + 31 of the 64-column
    // image 2 nt + (wave >> 1) of ops.pack_conv_weight_wino: per (position, kh) one contiguous 512-byte run, which no other wave of the
    // workgroup reads.  Scalar base, 32-bit lane offset.
    const float* u_src = p.b + (size_t)(2 * nt + (wave >> 1)) * nslabs * WINO_IMG;
    unsigned b_lane = (unsigned)(((lane >> 5) * 64 + (wave & 1) * 32 + (lane & 31)) * 16);
    f32x4 fa[2][4], fb[2][4];
    typedef const __attribute__((address_space(1))) f32x4* gf4_t;     // global, not flat: the opaque scalar base has lost its address space
    auto b_load1 = [&](const float* src, auto G, auto I) {     // src: u_src + slab * WINO_IMG
        constexpr int g = decltype(G)::value, i = decltype(I)::value;
        const char* us = reinterpret_cast<const char*>(src + (g * 4 + i) * WINO_POS);
        asm volatile("" : "+s"(us));
        asm volatile("" : "+v"(b_lane));
        fb[g & 1][i] = *(gf4_t)(us + b_lane);
    };

    f32x16 acc[16];
#pragma unroll
    for (int q = 0; q < 16; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
    const int a_off = ((lane >> 5) * 32 + (lane & 31)) * 4;

    // ---- prologue: halo 0 and 1 and transform 0 staged, halo 2 and the weights of (slab 0, group 0) requested (two barriers) -----------
    halo.src(0);
    halo.loads(hreg, 0);
    {
        typename Halo::Regs hreg1;
        const int s1 = min(1, nslabs - 1);
        halo.src(s1);
        halo.loads(hreg1, s1);
#define DS_WINO_F(i) b_load1(u_src, DS_WINO_I(0), DS_WINO_I(i));
        DS_WINO_EACH4(DS_WINO_F)
#undef DS_WINO_F
        DS_RACE_SKEW(wave);
        halo.store(hreg, Hs);
        DS_RACE_SKEW(wave);
        halo.store(hreg1, Hs + h_buf);
    }
    {
        const int s2 = min(2, nslabs - 1);
        halo.src(s2);
        halo.loads(hreg, s2);
    }
    __syncthreads();                                   // Hs[0], Hs[1] published
#define DS_WINO_TR1(i) tr_read1(Hs, DS_WINO_I(i));
    DS_WINO_EACH12(DS_WINO_TR1)
#undef DS_WINO_TR1
    DS_RACE_SKEW(wave);
    tr_write(Vs);
    DS_WINO_WAIT_VM0();                                // nothing in flight on entry: the loop's counted waits then follow from its own order of loads alone
    __syncthreads();                                   // Vs[0] published

    // ---- K loop: ONE barrier per slab, no LDS-DMA and hence no vmcnt(0): every global load goes to registers of the wave that uses them,
    // and the compiler's counted waits stand in front of the first use (the halo store of the next slab; the MFMAs of the next group)
    int s = 0;
    do {                                               // nslabs >= 1 (conv3x3_wino_applicable)
        const int par = s & 1;
        const float* vb = Vs + par * WN_IMG;
        float* vbn = Vs + (par ^ 1) * WN_IMG;          // last read by the MFMAs of slab s-1 (barrier s-1 passed)
        float* hb = Hs + par * h_buf;                  // last read by the transform of slab s, in front of barrier s-1
        const float* hbn = Hs + (par ^ 1) * h_buf;     // the halo of slab s+1, published at barrier s-1
        const int s1 = min(s + 1, nslabs - 1), s3 = min(s + 3, nslabs - 1);
        const float* uc = u_src + (size_t)s * WINO_IMG;
        const float* un = u_src + (size_t)s1 * WINO_IMG;
        auto a_read = [&](auto G, auto I) {
            constexpr int g = decltype(G)::value, i = decltype(I)::value;
            fa[g & 1][i] = *reinterpret_cast<const f32x4*>(vb + (g * 4 + i) * WN_POS + a_off);
        };
#define DS_WINO_TR1(i) tr_read1(hbn, DS_WINO_I(i));       // transform of slab s+1, first half: Hs[par ^ 1] -> registers
        DS_WINO_EACH12(DS_WINO_TR1)
#undef DS_WINO_TR1
        DS_RACE_SKEW(wave);                            // halo of slab s+2 (its loads were issued a slab ago)
        halo.store(hreg, hb);
        halo.src(s3);
        DS_RACE_SKEW(wave);
        tr_write(vbn);                                 // second half: its adds, registers -> Vs[par ^ 1]
        // micro-slot k of group g = k >> 4, one memory instruction at most:
        //     16 g + 0 .. 3    the B fragments of group g+1 -- of group 0 of slab s+1 in group 3: a whole group (16 MFMAs) ahead of their use
        //     4 .. 9           (group 0) the halo loads and the 3 coefficient loads of slab s+3
        //     16 g + 10 .. 13  the A fragment reads of group g+1
        auto fill = [&](auto K) {
            constexpr int k = decltype(K)::value, g = k >> 4, q = k & 15;
            if constexpr (q < 4) {
                if constexpr (g < 3) b_load1(uc, DS_WINO_I(g + 1), DS_WINO_I(q));
                else b_load1(un, DS_WINO_I(0), DS_WINO_I(q));
            } else if constexpr (k < 7) {
                halo_load1(hreg, DS_WINO_I(k - 4));
            } else if constexpr (k < 10) {
                coef_load1(hreg, s3, DS_WINO_I(k - 7));
            } else if constexpr (q >= 10 && q < 14 && g < 3) {
                a_read(DS_WINO_I(g + 1), DS_WINO_I(q - 10));
            }
        };
        // micro-slot k: K step r = (k >> 2) & 3 of position 4 (k >> 4) + (k & 3), then its filler, pinned
#define DS_WINO_STEP(k)                                                                                                                \
        acc[((k) >> 4) * 4 + ((k) & 3)] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[((k) >> 4) & 1][(k) & 3][((k) >> 2) & 3],            \
                                                                               fb[((k) >> 4) & 1][(k) & 3][((k) >> 2) & 3],            \
                                                                               acc[((k) >> 4) * 4 + ((k) & 3)], 0, 0, 0);              \
        fill(DS_WINO_I(k));                                                                                                            \
        __builtin_amdgcn_sched_barrier(0);
#define DS_WINO_F(i) a_read(DS_WINO_I(0), DS_WINO_I(i));
        DS_WINO_EACH4(DS_WINO_F)
#undef DS_WINO_F
        __builtin_amdgcn_sched_barrier(0);
        DS_WINO_EACH16(DS_WINO_STEP, 0)
        DS_WINO_EACH16(DS_WINO_STEP, 16)
        DS_WINO_EACH16(DS_WINO_STEP, 32)
        DS_WINO_EACH16(DS_WINO_STEP, 48)
#undef DS_WINO_STEP
        __syncthreads();                               // slab s done: Vs[par] dead; Vs and Hs [par ^ 1] published
    } while (++s < nslabs);

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

    // ---- appended 1x1 slabs (header comment, "Skip slabs"): 128 pixels x 32 raw channels per slab, four float4 per thread, through V[0] =
    // Vs[0], V[1] = Vs[1] (dead behind the K loop's last barrier); the wave's 32 weight columns go global -> fragment registers like U, one
    // group ahead.  Slots:
    //     slot 16 g        the weight fragment of group g+1 (of group 0 of slab es+1 in group 3)
    //     slots 16 g + 1 .. 4   the four pixel fragment reads of group g+1
    //     slots 5 .. 8     the four ds_write_b128 of the pixels of slab es+1 -> V[(es+1) & 1]
    //     slots 9 .. 12    the four global loads of slab es+2 into the registers just stored
    const int nextra = (p.ec0 + p.ec1) / 32;
    if (nextra > 0) {
        const float* wsk = p.b + (size_t)(p.N / 64) * nslabs * WINO_IMG + (size_t)(2 * nt + (wave >> 1)) * nextra * 2048;
        WinoSkip<256, 32> skip(p, tid, lane, 0);
        auto e_load1 = [&](f32x4* dst, auto J) { skip.load1(dst, J); };
        f32x4 ga[2][4], gb[2];                         // fragments of group g: the four patch pixels' pixels and the weights
        auto w_load1 = [&](int es, auto G) {
            constexpr int g = decltype(G)::value;
            const char* ws = reinterpret_cast<const char*>(wsk + (size_t)es * 2048 + g * WINO_POS);
            asm volatile("" : "+s"(ws));
            asm volatile("" : "+v"(b_lane));
            gb[g & 1] = *(gf4_t)(ws + b_lane);
        };

        // prologue: weights of (slab 0, group 0) requested, pixels of slab 0 staged, pixels of slab 1 requested behind them
        f32x4 ereg[4];
        {
            f32x4 ereg0[4];
            w_load1(0, DS_WINO_I(0));
            skip.sel(p, 0, m0);
#define DS_WINO_F(j) e_load1(ereg0, DS_WINO_I(j));
            DS_WINO_EACH4(DS_WINO_F)
#undef DS_WINO_F
            skip.sel(p, min(1, nextra - 1), m0);
#define DS_WINO_F(j) e_load1(ereg, DS_WINO_I(j));
            DS_WINO_EACH4(DS_WINO_F)
#undef DS_WINO_F
            DS_RACE_SKEW(wave);
#pragma unroll
            for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4*>(Vs + skip.lds[j]) = ereg0[j];
        }
        __syncthreads();

        int es = 0;
        do {
            const float* vb = smem + (es & 1) * WN_IMG;
            float* vn = smem + ((es + 1) & 1) * WN_IMG;
            const int es1 = min(es + 1, nextra - 1);
            skip.sel(p, min(es + 2, nextra - 1), m0);
            auto a_read = [&](auto G, auto I) {
                constexpr int g = decltype(G)::value, i = decltype(I)::value;
                ga[g & 1][i] = *reinterpret_cast<const f32x4*>(vb + (i * 4 + g) * WN_POS + skip.a_off[g]);
            };
            auto fill = [&](auto K) {
                constexpr int k = decltype(K)::value, g = k >> 4, q = k & 15;
                if constexpr (q == 0) {
                    if constexpr (g < 3) w_load1(es, DS_WINO_I(g + 1));
                    else w_load1(es1, DS_WINO_I(0));
                } else if constexpr (q < 5) {
                    if constexpr (g < 3) a_read(DS_WINO_I(g + 1), DS_WINO_I(q - 1));
                } else if constexpr (k < 9) {          // pixels of slab es+1
                    if constexpr (k == 5) DS_RACE_SKEW(wave);
                    *reinterpret_cast<f32x4*>(vn + skip.lds[k - 5]) = ereg[k - 5];
                } else if constexpr (k < 13) {         // loads of slab es+2
                    e_load1(ereg, DS_WINO_I(k - 9));
                }
            };
            // micro-slot k: K step r = (k >> 2) & 3 of group k >> 4 into patch pixel k & 3, then its filler, pinned
#define DS_WINO_STEP(k)                                                                                                                \
            Y[(k) & 3] = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[((k) >> 4) & 1][(k) & 3][((k) >> 2) & 3], gb[((k) >> 4) & 1][((k) >> 2) & 3], \
                                                              Y[(k) & 3], 0, 0, 0);                                                    \
            fill(DS_WINO_I(k));                                                                                                        \
            __builtin_amdgcn_sched_barrier(0);
#define DS_WINO_F(i) a_read(DS_WINO_I(0), DS_WINO_I(i));
            DS_WINO_EACH4(DS_WINO_F)
#undef DS_WINO_F
            __builtin_amdgcn_sched_barrier(0);
            DS_WINO_EACH16(DS_WINO_STEP, 0)
            DS_WINO_EACH16(DS_WINO_STEP, 16)
            DS_WINO_EACH16(DS_WINO_STEP, 32)
            DS_WINO_EACH16(DS_WINO_STEP, 48)
#undef DS_WINO_STEP
            __syncthreads();                           // V[es & 1] dead; V[(es+1) & 1] published
        } while (++es < nextra);
    }

    // ---- the fused epilogue, one patch pixel (a, b) at a time: the first kernel's, on this wave's 32 tiles x 32 channels ------------------
    float* stage = smem + wave * 32 * WINO_EPI_LD;     // wave-private rows; every LDS buffer died at the last barrier
    const int c4 = (lane & 7) * 4;
    const int col = n0 + wave * 32 + c4;
    f32x4 cb = {0.f, 0.f, 0.f, 0.f}, cvu = {0.f, 0.f, 0.f, 0.f};
    if (p.colbias) cb = *reinterpret_cast<const f32x4*>(p.colbias + col);
    if (p.cbias) cvu = *reinterpret_cast<const f32x4*>(p.cbias + (size_t)(p.cbias_bcast ? 0 : img0) * p.cbias_ld + col);
    const float acc_scale = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, p.acc_scale)));
    const float scale = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, p.scale)));
    int e_row[4];                                      // output row of (pass, patch pixel (0, 0)) of this lane
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {
        const int tl = pass * 8 + (lane >> 3);
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
            // column sums of the 64 pixels of patch row a of the 32 tiles: block (m0 >> 6) + a, the block the first kernel's wave row gives it
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                st_s[q] += __shfl_xor(st_s[q], 8); st_s[q] += __shfl_xor(st_s[q], 16); st_s[q] += __shfl_xor(st_s[q], 32);
                st_q[q] += __shfl_xor(st_q[q], 8); st_q[q] += __shfl_xor(st_q[q], 16); st_q[q] += __shfl_xor(st_q[q], 32);
            }
            if (lane < 8) {
                float* sp = p.stats + (size_t)((m0 >> 6) + a) * 2 * p.N + col;
                *reinterpret_cast<f32x4*>(sp) = st_s;
                *reinterpret_cast<f32x4*>(sp + p.N) = st_q;
            }
        }
    }
}

int launch_wino_n128(KParams& p, hipStream_t stream) {
    const int smem = (2 * WN_IMG + 2 * (p.NP * WINO_K + 4)) * (int)sizeof(float);    // Vs and Hs doubled; + a spare halo cell each
    return wino_by_norm(p, [&](auto NORM) {
        constexpr int norm = decltype(NORM)::value;
        return p.NP * 2 <= 2 * 256 ? wino_launch<wino_n128_kernel<norm, 2>, 256, 64 * 1024>(p, smem, stream)
                                   : wino_launch<wino_n128_kernel<norm, 3>, 256, 64 * 1024>(p, smem, stream);
    });
}

// ---- wino_w8_kernel: the 32 x 128 tile on eight waves, two per SIMD (header comment) --------------------------------------------------------
constexpr int W8_NSH = 1;                         // halo float4 slots per thread: NP * 2 <= 512, i.e. 16- and 32-column images (NP = 180, 204)
constexpr int W8_XCH = 4 * 16 * 64;               // floats a wave passes to its partner: four accumulators x 16 registers x 64 lanes (16 KiB)

// a - b on register pairs, as v_pk_add_f32 with the negate bits -- what the compiler makes of a two-float subtraction in the input
// transform.  A sixteen-float one it leaves as sixteen v_sub_f32, and pairs cut out of it in the source are widened again or cost a
// register copy per operand; the same IEEE subtraction on the same operands either way.
__device__ __forceinline__ f32x16 w8_sub(const f32x16& a, const f32x16& b) {
    f32x16 d;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const f32x2 x = {a[2 * i], a[2 * i + 1]}, y = {b[2 * i], b[2 * i + 1]};
        f32x2 z;
        asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(z) : "v"(x), "v"(y));
        d[2 * i] = z[0]; d[2 * i + 1] = z[1];
    }
    return d;
}

// A wave-uniform value (a kernel argument, the wave's half) as a fresh scalar at each use: the branch on it is then s_cmp + s_cbranch_scc.
// One flag shared by several branches is kept as a lane mask, inverted with v_cndmask + v_cmp where a branch wants its complement, or
// turned into selects.
template <typename T>
__device__ __forceinline__ T w8_uni(T x) {
    asm volatile("" : "+s"(x));
    return x;
}

// NORM: WinoHalo's
template <int NORM>
__global__ void __launch_bounds__(512, 1) wino_w8_kernel(const KParams p) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* Vs = smem;                              // [2][16][2][32][4]
    float* Hs = smem + 2 * WN_IMG;                 // [2] x { [2][2][HP][WP / 2][4], and one spare 16-byte cell behind it }

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cg = wave & 3, ph = wave >> 2;       // channel group (32 columns) and half of the 16 positions (rows 2 ph, 2 ph + 1 of the patch)
    int mt, nt;
    if (!decode_tile(blockIdx.x, p.mtiles, p.ntiles, mt, nt)) return;
    const int m0 = mt * 128, n0 = nt * 128;
    const int lw = __builtin_ctz(p.W);             // W = 16 | 32 on this kernel: divisions by W and by W / 2 are shifts
    const int img0 = m0 / p.HW;
    const int r0 = (m0 - img0 * p.HW) >> lw;
    const int Ctot = p.c0 + p.c1;
    const int nslabs = Ctot / WINO_K;

    // ---- FIRST what the first loads need, and the loads: the slot's offsets and the image's bases (WinoHalo's constructor), the weight
    // run.  Halo 0 and 1 and the B fragments of (slab 0, group 0) are on their way while the rest of the set-up runs.
    // halo stage: one float4 slot per thread over 512 threads
    using Halo = WinoHalo<512, W8_NSH, W8_NSH, NORM>;
    Halo halo(p, tid, img0, r0);
    const int h_buf = halo.buf;
    typename Halo::Regs hreg, hreg1;
    auto halo_load1 = [&](typename Halo::Regs& R, auto J) { halo.load1(R, J); };
    auto coef_load1 = [&](typename Halo::Regs& R, int sl, auto I) { halo.coef1(R, sl, I); };

    // transformed weights: global -> the B fragment registers, as in wino_n128_kernel: the 32 columns of channel group cg are rows
    // 32 (cg & 1) .. + 31 of the 64-column image 2 nt + (cg >> 1); this wave reads the positions 8 ph .. 8 ph + 7 of them.  The two waves
    // of a pair read disjoint halves of the run: per SIMD the weight traffic is wino_n128_kernel's.
    const float* u_src = p.b + (size_t)(2 * nt + (cg >> 1)) * nslabs * WINO_IMG + ph * 8 * WINO_POS;
    unsigned b_lane = (unsigned)(((lane >> 5) * 64 + (cg & 1) * 32 + (lane & 31)) * 16);
    f32x4 fa[2][4], fb[2][4];
    typedef const __attribute__((address_space(1))) f32x4* gf4_t;     // global, not flat: the opaque scalar base has lost its address space
    auto b_load1 = [&](const float* src, auto G, auto I) {     // src: u_src + slab * WINO_IMG
        constexpr int g = decltype(G)::value, i = decltype(I)::value;
        const char* us = reinterpret_cast<const char*>(src + (g * 4 + i) * WINO_POS);
        asm volatile("" : "+s"(us));
        asm volatile("" : "+v"(b_lane));
        fb[g & 1][i] = *(gf4_t)(us + b_lane);
    };

    halo.src(0);
    halo.loads(hreg, 0);
    {
        const int s1 = min(1, nslabs - 1);             // slab 1, requested behind slab 0 so that the two latencies overlap
        halo.src(s1);
        halo.loads(hreg1, s1);
    }
#define DS_WINO_F(i) b_load1(u_src, DS_WINO_I(0), DS_WINO_I(i));
    DS_WINO_EACH4(DS_WINO_F)
#undef DS_WINO_F
    __builtin_amdgcn_sched_barrier(0);                 // the requests stay in front of the set-up below

    // ---- THEN, under their latency, the rest: the slot's LDS cell and its zero cells (written here, by the thread that owns the slot, in
    // front of its first halo store; the first barrier publishes them), the transform's and the fragments' indices.
    halo.cells(p, Hs, tid, r0);
    const int WPH = p.WP >> 1, Wt = p.W >> 1;

    // ---- input transform: 32 tiles x 4 channel pairs, each split over FOUR threads by rows of B^T d B.  A thread owns (tile t_t, channels
    // 4 kh_t + 2 cpl .. + 1, row t_row): it reads the two rows of d its row of B^T d is made of (d0 - d2, d1 + d2, d2 - d1, d1 - d3) and
    // writes four positions.  kh_t and t_row are uniform per wave (wave = kh_t + 2 t_row): scalar branches, the same instruction count in
    // every wave.  Every value is made by the 64 x 64 kernel's operations on the same operands.
    const int t_t = (tid >> 1) & 31, cpl = tid & 1, kh_t = wave & 1, t_row = wave >> 1;
    const int t_ty = t_t >> (lw - 1), t_tx = t_t & (Wt - 1);
    const int h_rd0 = ((kh_t * 2 * p.HP + 2 * t_ty + (t_row == 0 ? 0 : 1)) * WPH + t_tx) * 4 + cpl * 2;     // row 0 | 1 | 1 | 1 of d
    const int h_rd1 = ((kh_t * 2 * p.HP + 2 * t_ty + (t_row == 3 ? 3 : 2)) * WPH + t_tx) * 4 + cpl * 2;     // row 2 | 2 | 2 | 3
    const int h_par = p.HP * WPH * 4;              // odd-column plane
    const int v_wr = (kh_t * 32 + t_t) * 4 + cpl * 2 + t_row * 4 * WN_POS;
    f32x2 t_e[2][4];
    auto tr_read1 = [&](const float* hs, auto I) {             // piece I = row I / 4 (of this thread's two), column I % 4
        constexpr int i = decltype(I)::value >> 2, j = decltype(I)::value & 3;
        t_e[i][j] = *reinterpret_cast<const f32x2*>(hs + (i == 0 ? h_rd0 : h_rd1) + (j & 1) * h_par + (j >> 1) * 4);
    };
    auto tr_write = [&](float* vs) {
        f32x2 t_r[4];
        if (t_row == 1) {                          // d1 + d2
#pragma unroll
            for (int q = 0; q < 4; ++q) t_r[q] = t_e[0][q] + t_e[1][q];
        } else if (t_row == 2) {                   // d2 - d1
#pragma unroll
            for (int q = 0; q < 4; ++q) t_r[q] = t_e[1][q] - t_e[0][q];
        } else {                                   // d0 - d2, d1 - d3
#pragma unroll
            for (int q = 0; q < 4; ++q) t_r[q] = t_e[0][q] - t_e[1][q];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f32x2 v = j == 0 ? t_r[0] - t_r[2] : j == 1 ? t_r[1] + t_r[2] : j == 2 ? t_r[2] - t_r[1] : t_r[1] - t_r[3];     // (B^T d) B
            *reinterpret_cast<f32x2*>(vs + v_wr + j * WN_POS) = v;
        }
    };

    f32x16 acc[8];                                 // position 8 ph + q; never zeroed: the first slab's first K step takes the constant 0 as C
    const int a_off = ((lane >> 5) * 32 + (lane & 31)) * 4 + ph * 8 * WN_POS;

    // ---- prologue, second part: halo 0 and 1 and transform 0 staged, halo 2 requested (two barriers) ------------------------------------
    DS_RACE_SKEW(wave);
    halo.store(hreg, Hs);
    DS_RACE_SKEW(wave);
    halo.store(hreg1, Hs + h_buf);
    {
        const int s2 = min(2, nslabs - 1);
        halo.src(s2);
        halo.loads(hreg, s2);
    }
    __syncthreads();                                   // Hs[0], Hs[1] and the zero cells published
#define DS_WINO_TR1(i) tr_read1(Hs, DS_WINO_I(i));
    DS_WINO_EACH8(DS_WINO_TR1)
#undef DS_WINO_TR1
    DS_RACE_SKEW(wave);
    tr_write(Vs);
    DS_WINO_WAIT_VM0();                                // nothing in flight on entry: the loop's counted waits then follow from its own order of loads alone
    __syncthreads();                                   // Vs[0] published

    // ---- K loop: ONE barrier per slab and no forced `vmcnt(0)`, as in wino_n128_kernel; 32 micro-slots per wave, two waves per SIMD --------
    // A slab in two parts.  front(s): the transform of slab s+1 and the halo store of slab s+2, i.e. everything in front of the MFMA
    // block; back(s): the fragment reads of group 0, the block of micro-slots, the barrier.  Slab 0 is PEELED in front of the loop, and K
    // step 0 of each of its positions takes the constant 0 as its C operand -- 0 + a b has the bits the zeroed accumulator gave -- so no
    // move zeroes an accumulator.  The loop runs back(s), the exit test, front(s + 1): the MFMA block is the loop's header and the
    // scalar branches on the wave's transform row, which end front(), jump straight to it; with the whole slab as the body the compiler
    // put one more taken branch behind every barrier, and the layers of 64 slabs measured 0.3 - 0.7 % slower for it
    // (profiles/wino_outside_ab.txt).
    auto front = [&](const int s) {
        const int par = s & 1;
        float* vbn = Vs + (par ^ 1) * WN_IMG;          // last read by the MFMAs of slab s-1 (barrier s-1 passed)
        float* hb = Hs + par * h_buf;                  // last read by the transform of slab s, in front of barrier s-1
        const float* hbn = Hs + (par ^ 1) * h_buf;     // the halo of slab s+1, published at barrier s-1
        const int s3 = min(s + 3, nslabs - 1);
#define DS_WINO_TR1(i) tr_read1(hbn, DS_WINO_I(i));       // transform of slab s+1, first half: Hs[par ^ 1] -> registers
        DS_WINO_EACH8(DS_WINO_TR1)
#undef DS_WINO_TR1
        DS_RACE_SKEW(wave);                            // halo of slab s+2 (its loads were issued a slab ago)
        halo.store(hreg, hb);
        halo.src(s3);
        DS_RACE_SKEW(wave);
        tr_write(vbn);                                 // second half: its adds, registers -> Vs[par ^ 1]
    };
    auto back = [&](const int s, auto FIRST) {
        constexpr bool first = decltype(FIRST)::value != 0;
        const int par = s & 1;
        const float* vb = Vs + par * WN_IMG;
        const int s1 = min(s + 1, nslabs - 1), s3 = min(s + 3, nslabs - 1);
        const float* uc = u_src + (size_t)s * WINO_IMG;
        const float* un = u_src + (size_t)s1 * WINO_IMG;
        auto a_read = [&](auto G, auto I) {
            constexpr int g = decltype(G)::value, i = decltype(I)::value;
            fa[g & 1][i] = *reinterpret_cast<const f32x4*>(vb + (g * 4 + i) * WN_POS + a_off);
        };
        // micro-slot k of group g = k >> 4 (positions 8 ph + 4 g .. + 3), one memory instruction at most:
        //     16 g + 0 .. 3    the B fragments of the next group -- of group 0 of slab s+1 in group 1: a whole group (16 MFMAs) ahead of their use
        //     4 .. 7           (group 0) the halo load and the 3 coefficient loads of slab s+3
        //     10 .. 13         (group 0) the A fragment reads of group 1
        auto fill = [&](auto K) {
            constexpr int k = decltype(K)::value, g = k >> 4, q = k & 15;
            if constexpr (q < 4) {
                if constexpr (g == 0) b_load1(uc, DS_WINO_I(1), DS_WINO_I(q));
                else b_load1(un, DS_WINO_I(0), DS_WINO_I(q));
            } else if constexpr (k == 4) {
                halo_load1(hreg, DS_WINO_I(0));
            } else if constexpr (k < 8) {
                coef_load1(hreg, s3, DS_WINO_I(k - 5));
            } else if constexpr (k >= 10 && k < 14) {
                a_read(DS_WINO_I(1), DS_WINO_I(k - 10));
            }
        };
        auto c_in = [&](auto K) -> f32x16 {
            constexpr int k = decltype(K)::value;
            if constexpr (first && ((k >> 2) & 3) == 0) return f32x16{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            else return acc[(k >> 4) * 4 + (k & 3)];
        };
        // micro-slot k: K step r = (k >> 2) & 3 of position 8 ph + 4 (k >> 4) + (k & 3), then its filler, pinned
#define DS_WINO_STEP(k)                                                                                                                \
        acc[((k) >> 4) * 4 + ((k) & 3)] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[((k) >> 4) & 1][(k) & 3][((k) >> 2) & 3],            \
                                                                               fb[((k) >> 4) & 1][(k) & 3][((k) >> 2) & 3],            \
                                                                               c_in(DS_WINO_I(k)), 0, 0, 0);                           \
        fill(DS_WINO_I(k));                                                                                                            \
        __builtin_amdgcn_sched_barrier(0);
#define DS_WINO_F(i) a_read(DS_WINO_I(0), DS_WINO_I(i));
        DS_WINO_EACH4(DS_WINO_F)
#undef DS_WINO_F
        __builtin_amdgcn_sched_barrier(0);
        DS_WINO_EACH16(DS_WINO_STEP, 0)
        DS_WINO_EACH16(DS_WINO_STEP, 16)
#undef DS_WINO_STEP
        __syncthreads();                               // slab s done: Vs[par] dead; Vs and Hs [par ^ 1] published
    };
    front(0);
    back(0, DS_WINO_I(1));                             // nslabs >= 1 (conv3x3_wino_applicable)
    if (nslabs > 1) {
        int s = 1;
        front(1);
        for (;;) {
            back(s, DS_WINO_I(0));
            if (++s >= nslabs) break;
            front(s);
        }
    }

    // ---- output transform Y = A^T M A across the pair.  The sums over the row index i of position 4 i + j come first, as in the lane-local
    // output transform: patch row 0 is (M[j] + M[4 + j]) + M[8 + j], patch row 1 is (M[4 + j] - M[8 + j]) - M[12 + j].  The wave of half 0 holds rows
    // i = 0, 1 and finishes patch row 0, for which it needs row 2 of its partner; the wave of half 1 holds rows 2, 3 and finishes patch row
    // 1, for which it needs row 1.  Each passes those four accumulators through the LDS (every K-loop buffer died at the last barrier):
    // wave w writes 16 KiB at smem + w * W8_XCH as [accumulator][register quad][lane][4] and reads the same cells of wave w ^ 4 -- the
    // same lane holds the same (tile, channel) in both waves of a pair.  One barrier.  Y[b] = the wave's 32 tiles x 32 channels at patch
    // pixel (ph, b).
    //
    // THE TAIL'S REQUESTS stand here, in front of the exchange's writes and its barrier: behind the K loop's last barrier its registers
    // (fragments, halo, transform) are dead, and what the skip-slab loop and the epilogue read from global memory depends on nothing the
    // exchange makes.  In the order of their use: the skip loop's weights of slab 0 and its pixels of slabs 0 and 1, the column bias, the
    // image's cbias row, and all eight residual quads of the wave's patch row (two patch pixels x four passes).  Only the requests
    // moved; every value is used where it was.
    //
    // Rows of the epilogue.  Lane l handles tile tl = 8 pass + (l >> 3) of the wave's 32 in pass 0 .. 3, i.e. output row
    // m0 + (2 ty + ph) W + 2 tx + b with ty = tl / Wt, tx = tl % Wt.  Wt >= 8, so the lane's part of tl never carries into ty: the row is a
    // scalar row of (pass, b) plus 2 (l >> 3), and an address is a 64-bit SCALAR base per (pass, b) plus ONE 32-bit lane offset per
    // tensor -- the form of the K loop's loads.  A tile spans 128 rows, so the lane offset fits whatever the tensor's size.
    const int nextra = (p.ec0 + p.ec1) / 32;
    const int c4 = (lane & 7) * 4;
    const int colw = n0 + cg * 32, col = colw + c4;    // the wave's first column (scalar), the lane's
    typedef __attribute__((address_space(1))) f32x4* gf4w_t;
    unsigned res_lane = (unsigned)(2 * (lane >> 3) * p.res_ld + c4) * 4u, out_lane = (unsigned)(2 * (lane >> 3) * p.ldo + c4) * 4u;   // BYTES
    auto e_srow = [&](int pass, int b) {               // scalar
        const int tp = pass * 8;
        return m0 + (((2 * (tp >> (lw - 1)) + ph)) << lw) + 2 * (tp & (Wt - 1)) + b;
    };

    WinoSkip<512, 32> skip;
    const float* wsk = p.b + (size_t)(p.N / 64) * nslabs * WINO_IMG + (size_t)(2 * nt + (cg >> 1)) * nextra * 2048;
    f32x4 ga[2][2], gb[4];                             // skip-loop fragments: the two patch pixels' pixels of group g, and the weights of every group
    auto e_load1 = [&](f32x4* dst, auto J) { skip.load1(dst, J); };
    auto w_load1 = [&](int es, auto G) {
        constexpr int g = decltype(G)::value;
        const char* ws = reinterpret_cast<const char*>(wsk + (size_t)es * 2048 + g * WINO_POS);
        asm volatile("" : "+s"(ws));
        asm volatile("" : "+v"(b_lane));
        gb[g] = *(gf4_t)(ws + b_lane);
    };
    f32x4 ereg[2], ereg0[2];
    if (nextra > 0) {                                  // weights of slab 0, pixels of slab 0 and, behind them, of slab 1
        skip.setup_loads(p, tid);
        w_load1(0, DS_WINO_I(0)); w_load1(0, DS_WINO_I(1)); w_load1(0, DS_WINO_I(2)); w_load1(0, DS_WINO_I(3));
        skip.sel(p, 0, m0);
        e_load1(ereg0, DS_WINO_I(0)); e_load1(ereg0, DS_WINO_I(1));
        skip.sel(p, min(1, nextra - 1), m0);
        e_load1(ereg, DS_WINO_I(0)); e_load1(ereg, DS_WINO_I(1));
    }
    f32x4 cb = {0.f, 0.f, 0.f, 0.f}, cvu = {0.f, 0.f, 0.f, 0.f};
    if (p.colbias) cb = *reinterpret_cast<const f32x4*>(p.colbias + col);
    if (p.cbias) cvu = *reinterpret_cast<const f32x4*>(p.cbias + (size_t)(p.cbias_bcast ? 0 : img0) * p.cbias_ld + col);
    f32x4 rv[2][4];
    auto res_load = [&](auto B) {                      // the four residual quads of patch pixel (ph, b)
        constexpr int b = decltype(B)::value;
        if (p.res) {
#pragma unroll
            for (int pass = 0; pass < 4; ++pass) {
                const char* rs = reinterpret_cast<const char*>(p.res + (size_t)e_srow(pass, b) * p.res_ld + colw);
                asm volatile("" : "+s"(rs));
                asm volatile("" : "+v"(res_lane));
                rv[b][pass] = __builtin_nontemporal_load((gf4_t)(rs + res_lane));
            }
        }
    };
    res_load(DS_WINO_I(0));
    res_load(DS_WINO_I(1));
    __builtin_amdgcn_sched_barrier(0);                 // the requests stay in front of the exchange

    f32x16 Y[2];
    {
        float* xw = smem + wave * W8_XCH + lane * 4;
        const float* xr = smem + (wave ^ 4) * W8_XCH + lane * 4;
        // `ph` is uniform per wave: ONE scalar branch per step, and each half names its accumulators directly (selected per register,
        // `ph == 0 ? acc[4 + q] : acc[q]` cost 64 v_cndmask and left half 1's differences unpacked)
        auto put = [&](const f32x16 (&m)[4]) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    const f32x4 v = {m[q][4 * r4], m[q][4 * r4 + 1], m[q][4 * r4 + 2], m[q][4 * r4 + 3]};
                    *reinterpret_cast<f32x4*>(xw + (q * 4 + r4) * 256) = v;
                }
        };
        auto get = [&](int j) {
            f32x16 o;
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(xr + (j * 4 + r4) * 256);
                o[4 * r4] = v[0]; o[4 * r4 + 1] = v[1]; o[4 * r4 + 2] = v[2]; o[4 * r4 + 3] = v[3];
            }
            return o;
        };
        DS_RACE_SKEW(wave);
        // (the empty asm statements differ, so the two halves' stores are not merged back into one run of selected stores)
        if (w8_uni(ph) == 0) { put(reinterpret_cast<const f32x16 (&)[4]>(acc[4])); asm volatile("; exchange: half 0 has written row 1" ::: "memory"); }
        else { put(reinterpret_cast<const f32x16 (&)[4]>(acc[0])); asm volatile("; exchange: half 1 has written row 2" ::: "memory"); }
        __syncthreads();
        // The partner's accumulator j + 1 is read while sum j is made, no further ahead, and accumulator 1 only behind sum 0, which frees 16
        // registers: all sixteen reads at once would hold 64 registers beside the 128 accumulators and what the tail has requested.
        f32x16 t[4], o[2];
        auto sum = [&](auto J) {
            constexpr int j = decltype(J)::value;
            __builtin_amdgcn_sched_barrier(0);
            if (w8_uni(ph) == 0) t[j] = acc[j] + acc[4 + j] + o[j & 1];
            else t[j] = w8_sub(w8_sub(o[j & 1], acc[j]), acc[4 + j]);
            __builtin_amdgcn_sched_barrier(0);
        };
        o[0] = get(0);
        sum(DS_WINO_I(0));
        o[1] = get(1);
        o[0] = get(2);
        sum(DS_WINO_I(1));
        o[1] = get(3);
        sum(DS_WINO_I(2));
        sum(DS_WINO_I(3));
        Y[0] = t[0] + t[1] + t[2];
        Y[1] = w8_sub(w8_sub(t[1], t[2]), t[3]);
    }

    // ---- appended 1x1 slabs (header comment, "Skip slabs") on this wave's TWO patch pixels (ph, 0) and (ph, 1): 32 MFMAs per slab and
    // wave.  The slab's 128 pixels x 32 raw channels go through V[0] = Vs[0], V[1] = Vs[1], two float4 per thread; the wave's 32 weight
    // columns go global -> the fragment registers gb[group], each group's weights of slab es+1 requested right behind the group's last
    // MFMA of slab es.  Slots:
    //     slot 8 g         (g >= 1) the weight fragment of group g-1 of slab es+1; slot 31: of group 3
    //     slots 8 g + 1, 2 the two pixel fragment reads of group g+1
    //     slots 3, 4       the two ds_write_b128 of the pixels of slab es+1 -> V[(es+1) & 1]
    //     slots 5, 6       the two global loads of slab es+2 into the registers just stored
    // The barrier in front keeps the staging from overwriting what a partner has yet to read.
    if (nextra > 0) {
        skip.setup_cells(p, tid, lane, 0);
        __syncthreads();
        // prologue: the pixels of slab 0 staged (requested in front of the exchange, with the weights of slab 0 and the pixels of slab 1)
        DS_RACE_SKEW(wave);
#pragma unroll
        for (int j = 0; j < 2; ++j) *reinterpret_cast<f32x4*>(Vs + skip.lds[j]) = ereg0[j];
        __syncthreads();

        int es = 0;
        do {
            const float* vb = smem + (es & 1) * WN_IMG + ph * 8 * WN_POS;      // patch pixels 2 ph, 2 ph + 1
            float* vn = smem + ((es + 1) & 1) * WN_IMG;
            const int es1 = min(es + 1, nextra - 1);
            skip.sel(p, min(es + 2, nextra - 1), m0);
            auto a_read = [&](auto G, auto I) {
                constexpr int g = decltype(G)::value, i = decltype(I)::value;
                ga[g & 1][i] = *reinterpret_cast<const f32x4*>(vb + (i * 4 + g) * WN_POS + skip.a_off[g]);
            };
            auto fill = [&](auto K) {
                constexpr int k = decltype(K)::value, g = k >> 3, q = k & 7;
                if constexpr (q == 0) {
                    if constexpr (g >= 1) w_load1(es1, DS_WINO_I(g - 1));
                } else if constexpr (q < 3) {
                    if constexpr (g < 3) a_read(DS_WINO_I(g + 1), DS_WINO_I(q - 1));
                } else if constexpr (k < 5) {          // pixels of slab es+1
                    if constexpr (k == 3) DS_RACE_SKEW(wave);
                    *reinterpret_cast<f32x4*>(vn + skip.lds[k - 3]) = ereg[k - 3];
                } else if constexpr (k < 7) {          // loads of slab es+2
                    e_load1(ereg, DS_WINO_I(k - 5));
                } else if constexpr (k == 31) {
                    w_load1(es1, DS_WINO_I(3));
                }
            };
            // micro-slot k: K step r = (k >> 1) & 3 of group k >> 3 into patch pixel (ph, k & 1), then its filler, pinned
#define DS_WINO_STEP(k)                                                                                                                \
            Y[(k) & 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[((k) >> 3) & 1][(k) & 1][((k) >> 1) & 3], gb[(k) >> 3][((k) >> 1) & 3], \
                                                              Y[(k) & 1], 0, 0, 0);                                                    \
            fill(DS_WINO_I(k));                                                                                                        \
            __builtin_amdgcn_sched_barrier(0);
            a_read(DS_WINO_I(0), DS_WINO_I(0)); a_read(DS_WINO_I(0), DS_WINO_I(1));
            __builtin_amdgcn_sched_barrier(0);
            DS_WINO_EACH16(DS_WINO_STEP, 0)
            DS_WINO_EACH16(DS_WINO_STEP, 16)
#undef DS_WINO_STEP
            __syncthreads();                           // V[es & 1] dead; V[(es+1) & 1] published
        } while (++es < nextra);
    }

    // ---- the fused epilogue of patch row ph, one patch pixel at a time: the first kernel's, on this wave's 32 tiles x 32 channels.  The
    // staging rows lie in the cells this wave alone read in the exchange (its partner wrote them in front of the exchange's barrier).
    float* stage = smem + (wave ^ 4) * W8_XCH;
    const float acc_scale = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, p.acc_scale)));
    const float scale = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, p.scale)));
    f32x4 st_s = {0.f, 0.f, 0.f, 0.f}, st_q = {0.f, 0.f, 0.f, 0.f};
    // p.cbias, p.res and p.act are uniform per launch: scalar branches (the empty asm statements keep the compiler from turning them
    // into four selects per quad again)
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const f32x16 y = Y[b];
#pragma unroll
        for (int r = 0; r < 16; ++r) stage[((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * WINO_EPI_LD + (lane & 31)] = y[r];
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            f32x4 v = *reinterpret_cast<const f32x4*>(stage + (pass * 8 + (lane >> 3)) * WINO_EPI_LD + c4);
            v *= acc_scale;
            v += cb;
            if (w8_uni(p.cbias) != nullptr) { v += cvu; asm volatile("" ::: "memory"); }
            if (w8_uni(p.res) != nullptr) { v += rv[b][pass]; asm volatile("" ::: "memory"); }
            v *= scale;
            if (w8_uni(p.act) == DS_ACT_SILU) {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = ds_silu(v[q]);
                asm volatile("" ::: "memory");
            }
            char* os = reinterpret_cast<char*>(p.out + (size_t)e_srow(pass, b) * p.ldo + colw);
            asm volatile("" : "+s"(os));
            asm volatile("" : "+v"(out_lane));
            __builtin_nontemporal_store(v, (gf4w_t)(os + out_lane));
            st_s += v; st_q += v * v;
        }
    }
    if (p.stats) {
        // column sums of the 64 pixels of patch row ph of the 32 tiles: block (m0 >> 6) + ph, summed in the other kernels' order
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            st_s[q] += __shfl_xor(st_s[q], 8); st_s[q] += __shfl_xor(st_s[q], 16); st_s[q] += __shfl_xor(st_s[q], 32);
            st_q[q] += __shfl_xor(st_q[q], 8); st_q[q] += __shfl_xor(st_q[q], 16); st_q[q] += __shfl_xor(st_q[q], 32);
        }
        if (lane < 8) {
            float* sp = p.stats + (size_t)((m0 >> 6) + ph) * 2 * p.N + col;
            *reinterpret_cast<f32x4*>(sp) = st_s;
            *reinterpret_cast<f32x4*>(sp + p.N) = st_q;
        }
    }
}

int launch_wino_w8(KParams& p, hipStream_t stream) {
    // the K loop's Vs and Hs (doubled; + a spare halo cell each) and, behind its last barrier, the eight waves' exchange
    const int kloop = (2 * WN_IMG + 2 * (p.NP * WINO_K + 4)) * (int)sizeof(float), xch = 8 * W8_XCH * (int)sizeof(float);
    return wino_by_norm(p, [&](auto NORM) {
        return wino_launch<wino_w8_kernel<decltype(NORM)::value>, 512, 160 * 1024>(p, kloop > xch ? kloop : xch, stream);
    });
}

template <int VAR>
int launch_wino(KParams& p, hipStream_t stream) {
    const int smem = (4 * WINO_IMG + 2 * (p.NP * WINO_K + 4)) * (int)sizeof(float);  // Us, Vs and Hs doubled; + a spare halo cell each
    return wino_by_norm(p, [&](auto NORM) {
        constexpr int norm = decltype(NORM)::value;
        return p.NP * 2 <= 3 * 256 ? wino_launch<conv3x3_wino_kernel<VAR, norm, 3>, 256, 160 * 1024>(p, smem, stream)
                                   : wino_launch<conv3x3_wino_kernel<VAR, norm, 4>, 256, 160 * 1024>(p, smem, stream);
    });
}

#undef DS_WINO_EACH16
#undef DS_WINO_EACH12
#undef DS_WINO_EACH8
#undef DS_WINO_EACH4
#undef DS_WINO_I

}  // namespace

// The layer as the kernel above takes it: one image per 256-pixel M tile with an even number of rows (16-, 32- and 64-column images),
// whole 64-column tiles, the vector epilogue, no split-K.
bool conv3x3_wino_applicable(const KParams& p) {
    if (p.taps != 9 || p.stride != 1 || p.splits != 1 || (p.ec0 & 31) || (p.ec1 & 31)) return false;
    if ((p.H & 1) || (p.W & 1) || p.W < 4 || p.W > 64 || p.HW % 256 || 256 % p.W || ((256 / p.W) & 1)) return false;
    if ((p.N & 63) || (p.c0 % WINO_K) || (p.c1 % WINO_K) || !p.vec_ok || p.out_planar || p.out_f16 || p.res_f16 || p.rowbias) return false;
    if (p.act != DS_ACT_NONE && p.act != DS_ACT_SILU) return false;
    const int np = (256 / p.W + 2) * (p.W + 2);
    if (np * 2 > WINO_NSH * 256 || (4 * WINO_IMG + 2 * (np * WINO_K + 4)) * (int)sizeof(float) > 160 * 1024) return false;
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
    // Tile shape: 32 tiles x 128 channels unless ds_conv_tune.variant bit 10 asks for the first kernel's 64 x 64 (A/B timing, the bit
    // comparison of tests/test_hip_wino_n128.py).  Every accepted shape fits it: 128 / W is even for W in 4 .. 64, and the route gives
    // this file only layers whose columns all lie on 256-column tiles.  On that tile: eight waves, two per SIMD (wino_w8_kernel), at 16 and
    // 32 columns -- the widths at which it was measured faster (profiles/wino_w8_ab.txt: - 3.0 ... - 3.8 % per layer; at 64 columns it
    // gains nothing, 4 and 8 columns are in no network and were not measured) -- unless bit 15 asks for the four-wave kernel (A/B
    // timing, the bit comparison of tests/test_hip_wino_w8.py).
    if (!(p.t_variant & 1024) && p.N % 128 == 0) {
        p.TH = 128 / p.W; p.HP = p.TH + 2; p.NP = p.HP * p.WP;
        p.mtiles = p.M / 128; p.ntiles = p.N / 128;
        const bool w8 = (p.W == 16 || p.W == 32) && !(p.t_variant & 32768);
        return w8 ? launch_wino_w8(p, stream) : launch_wino_n128(p, stream);
    }
    return launch_wino<0>(p, stream);
}

}  // namespace igemm
