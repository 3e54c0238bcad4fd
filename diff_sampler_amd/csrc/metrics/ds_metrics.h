/* libdsmetrics.so -- evaluation metrics on the fp64 matrix pipe of the MI355X (gfx950), a SECOND library next to libdsamd.so
 * (include/ds_engine.h): nothing here is part of the sampling engine's ABI, its build hashes or its tile tables.
 *
 * Second part (DSM_VERSION 2, below the PRDC entry points): the device code of the CLIP score -- csrc/metrics/clip_score.hip, and the
 * resize and crop in front of it -- csrc/metrics/image_prep.hip (added without a version step: nothing existing changed).
 * Third part (at the end; again without a version step): dsm_gemm_split -- csrc/metrics/gemm_split.hip, the Linear layer of the towers' fp16x3
 * mode: fp32 operands and fp32 results, every product as three fp16 products (split hi / lo halves) on the fp16 matrix pipe.
 * Fourth part (after it; no version step either): dsm_fir_resample / dsm_zero_border -- csrc/metrics/fir_resample.hip, the two launches the
 * NCSN++ denoisers need beyond libdsamd.so.  They are no metric; they live here because a declaration in a header of csrc/ or include/ enters every
 * source hash of the engine (tile table, profile ties), and this library is where every kernel since those were pinned has gone.
 *
 * Precision / recall / density / coverage and per-sample realism (sfd-main/prdc.py) on detector features.  Features are
 * [n][ld] row-major with ld >= dim, fp32 (widened exactly) or fp64 chosen by a flag per operand; all arithmetic is fp64.
 * Squared distances take the expanded form  d2(i, j) = max(|x_i|^2 + |y_j|^2 - 2 x_i . y_j, 0)  with the dot products on
 * v_mfma_f64_16x16x4_f64; NO n x n matrix is written to memory -- the selection and the counts run on the accumulators of
 * each 128 x 128 tile.  Everything is compared in the squared domain; the caller takes square roots of outputs only.
 *
 * Conventions as in ds_engine.h: every entry point returns 0 or an error code (positive = hipError_t, negative = DS_E_ARG -1 /
 * DS_E_ALIGN -2 / DS_E_SHAPE -3), checks its arguments on the host before any launch, never allocates (the caller passes a
 * workspace of dsm_prdc_workspace_bytes, 8-byte aligned) and never synchronises.  Results are bitwise reproducible: no
 * floating-point atomics, every cross-workgroup reduction goes through per-workgroup partials in the workspace. */
#pragma once

#ifdef __cplusplus
extern "C" {
#endif

#define DSM_API __attribute__((visibility("default")))
#define DSM_VERSION 2      /* 2: the CLIP-score entry points (clip_score.hip) added; nothing of version 1 changed */
#define DSM_MAX_K 8          /* largest nearest_k the selection kernel is instantiated for (list of k + 1 values per row) */

DSM_API int dsm_version(void);
DSM_API const char* dsm_error_string(int code);

/* Bytes of workspace that dsm_knn_radii_sq (on either feature set) and dsm_prdc_cross need; negative error code for n < 1 or k < 1. */
DSM_API long long dsm_prdc_workspace_bytes(int n_real, int n_fake, int k);

/* Number of column splits a launch over n_rows x n_cols distances uses: each 128-row band is walked by this many workgroups,
 * each over a contiguous range of 128-column tiles (a fixed function of the two sizes -- not of the device). */
DSM_API int dsm_prdc_splits(int n_rows, int n_cols);

/* radii_sq[i] = the (k + 1)-th smallest d2(i, j) over all j in [0, n), counting multiplicity, with d2(i, i) forced to exactly 0
 * (prdc.py: get_kth_value(pairwise_distances(x), k = nearest_k + 1)).  DS_E_ARG: NULL pointer, ld < dim, k < 1, k + 1 > n,
 * workspace too small; DS_E_SHAPE: k > DSM_MAX_K, n > 65535 * 128. */
DSM_API int dsm_knn_radii_sq(const void* x, int x_f64, int ld, int n, int dim, int k, double* radii_sq, void* workspace,
                             long long workspace_bytes, void* stream);

/* One pass over the n_real x n_fake distances (no diagonal treatment; all comparisons strict):
 *   fake_count[j]  = #{i : d2(i, j) < radii_sq_real[i]}                 (density; precision = count > 0)
 *   real_hit[i]    = #{j : d2(i, j) < radii_sq_fake[j]}                 (recall = hit > 0)
 *   real_min_sq[i] = min_j d2(i, j)                                     (coverage = min < radii_sq_real[i])
 *   realism_sq[j]  = max over i with realism_mask[i] of radii_sq_real[i] / d2(i, j)      (only when both pointers are given;
 *                    +inf for a zero distance, NaN -- which the maximum keeps, as numpy's does -- for radius 0 over distance 0)
 * DS_E_ARG: NULL pointer (the two realism pointers may be NULL together), ld < dim, n < 1, workspace too small;
 * DS_E_SHAPE: n_real > 65535 * 128. */
DSM_API int dsm_prdc_cross(const void* real, int real_f64, int ld_r, int n_real, const void* fake, int fake_f64, int ld_f, int n_fake,
                           int dim, const double* radii_sq_real, const double* radii_sq_fake, int* fake_count, int* real_hit,
                           double* real_min_sq, const unsigned char* realism_mask, double* realism_sq, void* workspace,
                           long long workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------------------
 * CLIP score (clip_score.py of the reference repositories): what the two CLIP towers need beyond libdsamd.so, fp32 throughout.
 * These calls need no workspace.  DS_E_ARG: NULL pointer, non-positive count, a leading dimension smaller than the columns it carries;
 * DS_E_ALIGN: pointer not 16-byte aligned / columns or leading dimension not a multiple of 4 where a call says so; DS_E_SHAPE: a geometry
 * no kernel covers. */

/* Bidirectional attention  out[b, i, h*d : (h+1)*d] = sum_j softmax_j(scale * q[b,i,h,:] . k[b,j,h,:]) v[b,j,h,:]  with the operand
 * convention of ds_attn_args (include/ds_engine.h), field for field: token-major matrices [rows][ld] whose head h occupies columns
 * h*d ... (h+1)*d - 1, image b at b * *_bs floats, so a packed q|k|v projection is consumed in place.  Head sizes:
 * dsm_attention_supported(d) -- 88 (ViT-g-14) only; the head sizes ds_attention covers are the caller's to route there (DS_E_SHAPE here).
 * sq, skv >= 1 of any length.  Keys at or beyond skv have weight exactly 0 and are never read; rows at or beyond sq and columns beyond
 * heads * d of `out` are not written; a row's summation order depends on the row alone.  Pointers 16-byte aligned, ld* and *_bs
 * multiples of 4 (DS_E_ALIGN), ld* >= heads * d and `reserved` zero (DS_E_ARG). */
typedef struct dsm_attn_args {
    const float* q; const float* k; const float* v; float* out;
    int ldq, ldk, ldv, ldo;
    long long q_bs, k_bs, v_bs, o_bs;
    int batch, heads, sq, skv, d;
    float scale;
    int reserved[3];     /* where ds_attn_args carries out_f16 / in_f16 / variant: must be 0 */
} dsm_attn_args;

DSM_API int dsm_attention(const dsm_attn_args* a, void* stream);
DSM_API int dsm_attention_supported(int d);

/* y[r, :cols] = 0.5 x (1 + erf(x / sqrt 2)) -- the exact (erf) GELU; in place allowed; columns [cols, ld) untouched.  cols, ldx, ldy multiples of 4. */
DSM_API int dsm_gelu_rows(const float* x, int ldx, float* y, int ldy, long long rows, int cols, void* stream);

/* The A operand of a ViT patch projection: images [n][3][size][size] (uint8, or fp32 in [0, 1] with images_f32 = 1) ->
 * out[n * (size / patch)^2][ld], row = (image, patch row, patch column), column = (channel, py, px) as patch_embedding.weight.reshape(width, -1);
 * value (v / 255 - mean[c]) / std[c] (fp32 input: (v - mean[c]) / std[c]); columns [3 patch^2, ld) are written as zeros.  mean3 / std3:
 * three floats each in HOST memory, read during the call.  DS_E_SHAPE: size not a multiple of patch. */
DSM_API int dsm_vit_patch_rows(const void* images, int images_f32, int n, int size, int patch, const float* mean3, const float* std3, float* out,
                               int ld, void* stream);

/* out[b * tokens + 0] = cls + pos[0];  out[b * tokens + 1 + i] = patches[b * (tokens - 1) + i] + pos[1 + i]   (pos [tokens][width], dense). */
DSM_API int dsm_vit_tokens(const float* patches, int ldp, const float* cls, const float* pos, float* out, int ldo, int n, int tokens, int width,
                           void* stream);

/* out[i, :cols] = x[row_index[i], :cols] for i < n; row_index: int32 on the device, values in [0, x_rows) (the caller checks; the kernel clamps). */
DSM_API int dsm_gather_rows(const float* x, int ldx, long long x_rows, const int* row_index, float* out, int ldo, int n, int cols, void* stream);

/* scores[i] = 100 <a_i, b_i> / (|a_i| |b_i|) in fp32 for i < n, then  *sum += scores[0] + ... + scores[n - 1]  in fp64 in a fixed order
 * (no atomics: two runs give the same bits). */
DSM_API int dsm_clip_score(const float* a, int lda, const float* b, int ldb, int n, int dim, float* scores, double* sum, void* stream);

/* The resize and centre crop of the CLIP transform, bit for bit Pillow's 8-bit bicubic resampler (csrc/metrics/image_prep.hip; tables:
 * clip_preprocess.resample_coeffs).  src: n images of h x w interleaved RGB bytes, row r of image i at src + i * image_stride + r * pitch;
 * out: [n][3][size][size] bytes, the window of `size` rows from `top` and `size` columns from `left` of the image resized to nh x nw.
 * Horizontal pass first, then vertical, each  clamp((2^21 + sum_k pixel[first + k] * weight[k]) >> 22, 0, 255)  in int32 with a uint8
 * intermediate; a pass whose size does not change (nw == w, nh == h) is skipped and its table pointers are not read (they may be NULL).
 * hbounds [nw][2] = (first tap, taps), hcoeffs [nw][hksize] for the columns, vbounds [nh][2], vcoeffs [nh][vksize] for the rows: int32
 * on the device, weights in (-2^23, 2^23) (the kernel multiplies 24-bit operands); a table that contradicts the geometry yields wrong
 * pixels, never an access outside src.
 * DS_E_ARG: NULL src / out / table of a pass that runs, a non-positive size or count, negative image_stride, pitch < 3 w, a window outside
 * nh x nw, a ksize below 2 ceil(2 max(in / out, 1)) + 1;  DS_E_ALIGN: out not 16-byte aligned, a table not 4-byte aligned (src may
 * have any alignment: rows are read 16, 4 or 1 bytes at a time as src, pitch and image_stride allow);  DS_E_SHAPE: a side above 32768,
 * more than 2^31 - 1 workgroups, or a geometry beyond the kernel's LDS: four rows of the source columns the window's taps reach must fit
 * 24 KB (w <= 2048 for a full-width window) and the source rows one output row needs, times 3 (size rounded up to 4) bytes, 40 KB --
 * any source up to 2048 x 2048 down to size 224 (and to 288 x 288 at size 32) is inside. */
DSM_API int dsm_resize_crop_u8(const void* src, long long image_stride, int pitch, int n, int h, int w, int nh, int nw, int top, int left,
                               int size, const int* hbounds, const int* hcoeffs, int hksize, const int* vbounds, const int* vcoeffs,
                               int vksize, void* out, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------------------
 * fp16x3: a Linear layer with fp32 operands and results on the fp16 matrix pipe (csrc/metrics/gemm_split.hip; added without a version
 * step: nothing existing changed).
 *
 *     out[r, :cout] = act(x[r, :k] . W^T . 2^-shift + bias) + res[r, :cout]          for r < rows
 *
 * x, bias, res, out: fp32.  w_split: the weights W [cout][k] split once on the host (ops.pack_linear_weight_split): W' = W 2^shift,
 * hi = fp16(W'), lo = fp16(W' - hi), stored as fp16 [ceil(cout / 128) * 128][2 k] -- per 32-column block of K 32 hi halves, then 32 lo halves;
 * the rows beyond cout are zeros and ARE read.  The kernel splits x the same way while it stages a tile, without scaling, and adds
 * hi.hi + hi.lo + lo.hi per product on v_mfma_f32_32x32x16_f16 into an fp32 accumulator, which the epilogue multiplies by the exact 2^-shift.
 * DOMAIN: finite inputs with |x| <= 65504 (beyond that the hi half is infinite); x below 2^-3 in magnitude carries an absolute error of up to
 * 2^-24 |w| per product (the lo half is an fp16 subnormal), everything else a relative 3 * 2^-22 per product.
 * No split-K, no atomics, a fixed K order: the bits of an output row depend on that row of x (and res) and on the weights alone -- not on
 * `rows`, not on the row's position.  Columns [cout, out_ld) of out are never written.
 * act: DSM_ACT_NONE, DSM_ACT_GELU (0.5 v (1 + erf(v / sqrt 2)), dsm_gelu_rows' form) or DSM_ACT_QUICK_GELU (v sigmoid(1.702 v), ds_quick_gelu's form);
 * an activation and a residual exclude each other.  bias and res may be NULL.
 * Geometry: dsm_gemm_split_supported(rows, k, cout) -- rows >= 1, k and cout positive multiples of 32 -- otherwise DS_E_SHAPE.
 * DS_E_ARG: NULL a / x / w_split / out, ldx < k, out_ld < cout, res_ld < cout (with res), res == out (res must not overlap out), res with an
 * activation, an unknown act, shift outside [0, 126], a non-zero reserved field;  DS_E_ALIGN: a pointer not 16-byte aligned, ldx / out_ld /
 * res_ld (with res) not a multiple of 4.  No workspace, no allocation, no synchronisation. */
#define DSM_ACT_NONE 0
#define DSM_ACT_GELU 1
#define DSM_ACT_QUICK_GELU 2

typedef struct dsm_gemm_split_args {
    const float* x; int ldx; long long rows; int k;
    const void* w_split; int shift; int cout;
    const float* bias; const float* res; int res_ld; int act;
    float* out; int out_ld;
    int reserved[3];     /* must be 0 */
} dsm_gemm_split_args;

DSM_API int dsm_gemm_split(const dsm_gemm_split_args* a, void* stream);
DSM_API int dsm_gemm_split_supported(long long rows, int k, int cout);

/* ---------------------------------------------------------------------------------------------------------------------------------------
 * FIR resampling of the NCSN++ networks (csrc/metrics/fir_resample.hip; added without a version step: nothing existing changed): the
 * depthwise forms of the reference's Conv2d.forward (networks_edm.py:56-82) for a separable 4-tap resample_filter, on fp32 NHWC rows
 * x [n * h * w][ld_x] -> out [n * ho * wo][out_ld], columns [c, ld) neither read nor written.
 *
 *     f2d[i][j] = taps[i] taps[j] / (sum taps)^2                                   (formed in fp32, as the reference's buffer is)
 *     down:  fir[y, x] = sum_{i, j < 4} f2d[i][j] x[2y + i - pad, 2x + j - pad]     zero outside the image, not renormalised at the border;
 *            ho = (h + 2 pad - 4) / 2 + 1 (likewise wo); pad = 1: conv2d(stride 2, padding 1); pad = 0: the second half of fused_resample
 *     up:    fir[Y, X] = sum 4 f2d[i][j] x[y, x] over Y = 2y + i - 1, X = 2x + j - 1   conv_transpose2d(4 f2d, stride 2, padding 1); ho = 2h
 *     out[m, ch] = (fir + bias[ch] + res[m, ch]) * out_scale                         bias [c] and res [n * ho * wo][res_ld] may be NULL
 *
 * One fp32 FMA per tap in a fixed order (16 down, 4 up), then the epilogue's three operations.  res may be `out` itself (element-wise).
 * DS_E_ARG: NULL a / x / out, x == out, n, h, w or c <= 0, up not 0 / 1, pad not 0 / 1 (up: not 1), ld_x < c, out_ld < c, res_ld < c (with res),
 * taps whose sum is zero or not finite, a non-zero reserved field;  DS_E_ALIGN: c, ld_x, out_ld or res_ld (with res) not a multiple of 4, a
 * pointer not 16-byte aligned;  DS_E_SHAPE: down with h + 2 pad - 4 or w + 2 pad - 4 negative or odd, more than 2^31 - 1 rows.
 * dsm_fir_resample_supported(up, pad, h, w, c): 1 where a call of this geometry launches (host logic only). */
typedef struct dsm_fir_args {
    const float* x; int ld_x;
    int n, h, w, c;          /* the INPUT geometry */
    int up;                  /* 0 = down (stride 2), 1 = up (x 2) */
    int pad;
    float taps[4];
    const float* bias; const float* res; int res_ld;
    float out_scale;
    float* out; int out_ld;
    int reserved[3];         /* must be 0 */
} dsm_fir_args;

DSM_API int dsm_fir_resample(const dsm_fir_args* a, void* stream);
DSM_API int dsm_fir_resample_supported(int up, int pad, int h, int w, int c);

/* out [outer][h + 2p][w + 2p][inner] = x [outer][h][w][inner] inside a ring of p zeros (NHWC: outer = n, inner = c; channel-planar: outer = n c,
 * inner = 1).  Whole 16-byte quads when inner is a multiple of 4 (pointers 16-byte aligned then, else 4-byte: DS_E_ALIGN).  DS_E_ARG: NULL
 * pointer, x == out, a non-positive size, p < 0;  DS_E_SHAPE: a side or p above 32768, more than 2^31 - 1 output pixels. */
DSM_API int dsm_zero_border(const float* x, float* out, long long outer, int h, int w, int inner, int p, void* stream);

/* Dynamic thresholding of DPM-Solver++ (solver_utils.py:77-86) for samples beyond the LDS form of libdsamd's ds_dynamic_threshold (more than
 * 38 144 values: images of 128 pixels and above; csrc/metrics/threshold_large.hip; added without a version step: nothing existing changed).
 * x0, out: [n][per] fp32, out may be x0.  out = clamp(x0, -s, s) / s per sample with s = max(quantile_p(|x0|), 1), torch.quantile's linear
 * interpolation -- the same radix select, on keys read from global memory.  DS_E_ARG: NULL pointer, n <= 0, per <= 1, p outside [0, 1];
 * DS_E_SHAPE: more than 2^24 values per sample. */
DSM_API int dsm_dynamic_threshold_large(const float* x0, float* out, int n, int per, float p, void* stream);

/* ---------------------------------------------------------------------------------------------------------------------------------------
 * Trajectory analysis (diff-analyzer-main; csrc/metrics/traj.hip; added without a version step: nothing existing changed).
 *
 * dsm_traj_gram: traj is a sampler's stacked fp32 trajectory [n_pts][batch][per], contiguous and read in place (point t of sample b at
 * (t * batch + b) * per).  For the samples b in [b0, b0 + nb):
 *     gram[b - b0][t][s] = sum_e (x[t,b,e] - x[n_pts-1,b,e]) (x[s,b,e] - x[n_pts-1,b,e])          [nb][n_pts][n_pts] fp64
 * with the differences formed in fp64 (exact) and products and sums on v_mfma_f64_16x16x4_f64.  Tiles on and below the diagonal are computed
 * and mirrored: gram[t][s] and gram[s][t] are the same bits.  The contraction over `per` is split over dsm_traj_gram_splits(n_pts, per)
 * workgroups per tile -- a function of these two sizes only -- whose partials go to the workspace and are added in a fixed order: a sample's
 * matrix is the same bits for any batch, b0 and nb, and from run to run.  Any n_pts >= 2, per >= 1, batch >= 1.
 * workspace: dsm_traj_gram_workspace_bytes(n_pts, per, nb) bytes, 8-byte aligned (DS_E_ALIGN); where that is 0 (no split) it is not read and
 * may be NULL.  DS_E_ARG: NULL traj / gram, n_pts < 2, a non-positive size, [b0, b0 + nb) outside the batch, workspace missing or too small;
 * DS_E_SHAPE: n_pts > 32768, nb > 65535, more than 2^39 output elements (the workspace and split queries answer the same codes). */
DSM_API int dsm_traj_gram(const float* traj, int n_pts, int batch, long long per, int b0, int nb, double* gram, void* workspace,
                          long long workspace_bytes, void* stream);
DSM_API long long dsm_traj_gram_workspace_bytes(int n_pts, long long per, int nb);
DSM_API int dsm_traj_gram_splits(int n_pts, long long per);

/* out[r] = sum_e (a[r,e] - b[r,e])^2 for r < rows, or sum_e a[r,e]^2 with b_or_null == NULL; rows of `per` contiguous floats.  Differences and
 * sums in fp64, one workgroup per row, a fixed order.  DS_E_ARG: NULL a / out, rows or per < 1;  DS_E_SHAPE: rows > 2^31 - 1. */
DSM_API int dsm_row_sqdist(const float* a, const float* b_or_null, long long rows, long long per, double* out, void* stream);

#ifdef __cplusplus
}
#endif
