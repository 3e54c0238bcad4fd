/* libdsmetrics.so -- evaluation metrics on the fp64 matrix pipe of the MI355X (gfx950), a SECOND library next to libdsamd.so
 * (include/ds_engine.h): nothing here is part of the sampling engine's ABI, its build hashes or its tile tables.
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
#define DSM_VERSION 1
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

#ifdef __cplusplus
}
#endif
