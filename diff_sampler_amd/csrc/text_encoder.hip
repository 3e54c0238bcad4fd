// The three launches the CLIP text encoder of Stable Diffusion v1.x needs beyond the shared projection / LayerNorm kernels
// (diff-solvers-main/models/ldm/modules/encoders/modules.py:137-159 FrozenCLIPEmbedder -> transformers CLIPTextModel): the token + position
// embedding gather, the causal self-attention and quick_gelu.  fp32 only: the reference encodes its prompts outside autocast
// (diff-solvers-main/sample.py:286-289), so there is no fp16 form of any of them.
//
// ds_attention_causal: softmax over j <= i of (scale * q_i . k_j) v_j on the exact-fp32 matrix pipe, for SHORT sequences (sq <= 128; CLIP: 77).
// One block = one (image, head); the whole K and V of the head are staged in LDS once (77 x 64 fp32: 2 x 96 padded rows = 52 KB), wave w owns
// queries [32 w, 32 w + 32) and walks key tiles 0 .. w only -- the tiles right of the diagonal are never touched, the diagonal tile is masked
// per element.  Same transposed formulation as csrc/attention.hip (a query is a lane; S^T = K Q^T, O^T += V P^T; 32x32 MFMA C/D layout:
// register r of lane (q, hb) is key (r & 3) + 8 (r >> 2) + 4 hb of the tile), online softmax over the at most four tiles.
//   * a masked score is REPLACED by -1e30 (finite) before the row maximum is taken: its weight is exp2(-1e30 - m) = +0 exactly, so it is
//     excluded from the sum and from P V, and no inf - inf can form.  Tile 0 holds key 0 <= i for every query, so the running maximum is a
//     real score from the first tile on.
//   * keys >= sq (the padding of the last 32-key tile) are > i for every stored query: the causal mask covers them; their LDS rows are
//     zero-filled so that 0 x padding stays 0.  Query lanes >= sq compute on a clamped row and are not stored.
//   * the order in which a row's scores are summed depends on the row index alone (tile 0, 1, .. in turn; the MFMA's own order inside a tile):
//     the same bits at every batch size.
#include "ds_common.h"

namespace {

constexpr int CA_MAX_SQ = 128;

template <int D>
__global__ void __launch_bounds__(256) attn_causal_kernel(const ds_attn_args a) {
    constexpr int DB = D / 32;               // 32-row blocks of O^T
    constexpr int KLD = D + 4;               // (D + 4) / 4 odd: conflict-free ds_read_b128 of 32 distinct rows
    constexpr int VLD = D + 8;               // rows 4 apart land 32 banks apart
    constexpr int NQ4 = D / 8;
    constexpr int D4 = D / 4;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int SP = (a.sq + 31) & ~31;        // staged key rows: whole 32-key tiles
    float* Ks = smem;
    float* Vs = smem + SP * KLD;
    float* Es = Vs + SP * VLD;               // epilogue transposition patches, 32 x 33 floats per wave

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hb = lane >> 5, l31 = lane & 31;
    const int h = blockIdx.x, b = blockIdx.y;
    const int q0 = wave * 32;
    const float* qp = a.q + (size_t)b * a.q_bs + h * D;
    const float* kp = a.k + (size_t)b * a.k_bs + h * D;
    const float* vp = a.v + (size_t)b * a.v_bs + h * D;

    // K and V of the head -> LDS, once; rows >= sq are zeros
    DS_RACE_SKEW(wave);
    for (int idx = tid; idx < SP * D4; idx += 256) {
        const int row = idx / D4, c4 = idx - row * D4;
        f32x4 kv = {0.f, 0.f, 0.f, 0.f}, vv = {0.f, 0.f, 0.f, 0.f};
        if (row < a.sq) {
            kv = *reinterpret_cast<const f32x4*>(kp + (size_t)row * a.ldk + c4 * 4);
            vv = *reinterpret_cast<const f32x4*>(vp + (size_t)row * a.ldv + c4 * 4);
        }
        *reinterpret_cast<f32x4*>(Ks + row * KLD + c4 * 4) = kv;
        *reinterpret_cast<f32x4*>(Vs + row * VLD + c4 * 4) = vv;
    }
    __syncthreads();
    if (q0 >= a.sq) return;                  // no barrier below this line

    const float sc = a.scale * 1.4426950408889634f;
    const int qi = q0 + l31;                 // this lane's query
    f32x4 qf[NQ4];
    {
        const float* qr = qp + (size_t)min(qi, a.sq - 1) * a.ldq + 4 * hb;
#pragma unroll
        for (int ks = 0; ks < NQ4; ++ks) qf[ks] = *reinterpret_cast<const f32x4*>(qr + 8 * ks) * sc;
    }
    f32x16 ot[DB];
#pragma unroll
    for (int i = 0; i < DB; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) ot[i][r] = 0.f;
    float m = -1e30f, l = 0.f;

    for (int t = 0; t <= wave; ++t) {        // key tiles left of and on the diagonal
        f32x16 st;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.f;
        const float* kfrag = Ks + (t * 32 + l31) * KLD + 4 * hb;
#pragma unroll
        for (int ks = 0; ks < NQ4; ++ks) {
            const f32x4 kv = *reinterpret_cast<const f32x4*>(kfrag + 8 * ks);
#pragma unroll
            for (int r = 0; r < 4; ++r) st = __builtin_amdgcn_mfma_f32_32x32x2f32(kv[r], qf[ks][r], st, 0, 0, 0);
        }
        if (t == wave) {                     // the diagonal tile: keys j > i are excluded
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (t * 32 + 4 * hb + (r & 3) + 8 * (r >> 2) > qi) st[r] = -1e30f;
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
        for (int i = 0; i < DB; ++i) {
            ot[i] *= alpha;
            const float* vcol = Vs + (t * 32 + 4 * hb) * VLD + i * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r)
                ot[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(vcol[((r & 3) + 8 * (r >> 2)) * VLD], st[r], ot[i], 0, 0, 0);
        }
    }

    const float inv = 1.0f / (l + __shfl_xor(l, 32));
    float* patch = Es + wave * (32 * 33);    // private to the wave
    float* op = a.out + (size_t)b * a.o_bs + h * D;
#pragma unroll
    for (int i = 0; i < DB; ++i) {
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
            if (q0 + q < a.sq) *reinterpret_cast<f32x4*>(op + (size_t)(q0 + q) * a.ldo + i * 32 + c4) = o;
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// out[(b * seq + s) * out_ld + c] = tok_table[clamp(tokens[b * seq + s])][c] + pos_table[s][c]; one thread per 16 bytes
__global__ void __launch_bounds__(256) token_embed_kernel(const ds_token_embed_args a) {
    const int w4 = a.width >> 2;
    const long long total = (long long)a.batch * a.seq * w4;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long row = i / w4;
    const int c = (int)(i - row * w4) * 4;
    const int s = (int)(row % a.seq);
    const int id = min(max(a.tokens[row], 0), a.vocab - 1);      // never outside the table, whatever the host sent
    const f32x4 t = *reinterpret_cast<const f32x4*>(a.tok_table + (size_t)id * a.width + c);
    const f32x4 p = *reinterpret_cast<const f32x4*>(a.pos_table + (size_t)s * a.width + c);
    *reinterpret_cast<f32x4*>(a.out + (size_t)row * a.out_ld + c) = t + p;
}

// y = x * sigmoid(1.702 x) (transformers' quick_gelu, the activation of the OpenAI CLIP towers); one thread per 16 bytes
__global__ void __launch_bounds__(256) quick_gelu_kernel(const ds_quick_gelu_args a) {
    const int c4n = a.cols >> 2;
    const long long total = a.rows * c4n;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long row = i / c4n;
    const int c = (int)(i - row * c4n) * 4;
    const f32x4 v = *reinterpret_cast<const f32x4*>(a.x + (size_t)row * a.ldx + c);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = v[j] * __builtin_amdgcn_rcpf(1.0f + __expf(-1.702f * v[j]));
    *reinterpret_cast<f32x4*>(a.y + (size_t)row * a.ldy + c) = o;
}

}  // namespace

extern "C" int ds_attention_causal_supported(int d, int sq) { return d == 64 && sq >= 1 && sq <= CA_MAX_SQ; }

extern "C" int ds_attention_causal(const ds_attn_args* a, void* stream) {
    (void)hipGetLastError();
    if (!a || !a->q || !a->k || !a->v || !a->out) return DS_E_ARG;
    if (a->out_f16 || a->in_f16) return DS_E_ARG;                 // fp32 tensors only
    if (a->batch <= 0 || a->heads <= 0 || a->sq <= 0 || a->skv <= 0 || a->batch > 65535) return DS_E_ARG;
    if (a->sq != a->skv) return DS_E_ARG;                         // self-attention: the mask j <= i needs one sequence
    if (!ds_attention_causal_supported(a->d, a->sq)) return DS_E_SHAPE;
    if ((a->ldq & 3) || (a->ldk & 3) || (a->ldv & 3) || (a->ldo & 3) || (a->q_bs & 3) || (a->k_bs & 3) || (a->v_bs & 3) || (a->o_bs & 3))
        return DS_E_ALIGN;
    if (!ds_aligned16(a->q) || !ds_aligned16(a->k) || !ds_aligned16(a->v) || !ds_aligned16(a->out)) return DS_E_ALIGN;
    constexpr int D = 64;
    constexpr int max_bytes = (CA_MAX_SQ * (D + 4) + CA_MAX_SQ * (D + 8) + 4 * 32 * 33) * (int)sizeof(float);
    DS_ENSURE_DYN_LDS((&attn_causal_kernel<D>), max_bytes);
    const int sp = (a->sq + 31) & ~31;
    const int bytes = (sp * (D + 4) + sp * (D + 8) + 4 * 32 * 33) * (int)sizeof(float);
    hipLaunchKernelGGL(attn_causal_kernel<D>, dim3(a->heads, a->batch), dim3(256), bytes, (hipStream_t)stream, *a);
    DS_CHECK_LAUNCH();
    return DS_OK;
}

extern "C" int ds_token_embed(const int* tokens, const float* tok_table, const float* pos_table, float* out, int out_ld, int batch, int seq,
                              int width, int vocab, void* stream) {
    (void)hipGetLastError();
    if (!tokens || !tok_table || !pos_table || !out || batch <= 0 || seq <= 0 || width <= 0 || vocab <= 0) return DS_E_ARG;
    if ((width & 3) || (out_ld & 3) || out_ld < width) return DS_E_ALIGN;
    if (!ds_aligned16(tok_table) || !ds_aligned16(pos_table) || !ds_aligned16(out)) return DS_E_ALIGN;
    const ds_token_embed_args a = {tokens, tok_table, pos_table, out, out_ld, batch, seq, width, vocab};
    const long long total = (long long)batch * seq * (width >> 2);
    if ((total + 255) / 256 > 0x7fffffffLL) return DS_E_SHAPE;
    hipLaunchKernelGGL(token_embed_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    DS_CHECK_LAUNCH();
    return DS_OK;
}

extern "C" int ds_quick_gelu(const float* x, int ldx, float* y, int ldy, long long rows, int cols, void* stream) {
    (void)hipGetLastError();
    if (!x || !y || rows <= 0 || cols <= 0) return DS_E_ARG;
    if ((cols & 3) || (ldx & 3) || (ldy & 3) || ldx < cols || ldy < cols) return DS_E_ALIGN;
    if (!ds_aligned16(x) || !ds_aligned16(y)) return DS_E_ALIGN;
    const ds_quick_gelu_args a = {x, ldx, y, ldy, rows, cols};
    const long long total = rows * (cols >> 2);
    if ((total + 255) / 256 > 0x7fffffffLL) return DS_E_SHAPE;
    hipLaunchKernelGGL(quick_gelu_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    DS_CHECK_LAUNCH();
    return DS_OK;
}
