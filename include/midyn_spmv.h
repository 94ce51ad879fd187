/*
 * midyn_spmv.h -- C-ABI of libmidyn.so for models whose operators are SPARSE (the reference's array_library="scipy_sparse":
 * models/generator_model.py:332-390, models/operator_collections.py:130-230).  The operators never exist as dense arrays:
 * the caller merges the static part and the k operators into one padded row structure of `width` slots per row (ELL), and
 * the device evaluates  out = exp(-F t) o [ (G_d' + sum_j c_j G_j) (exp(F t) o y) ]  (F = i diag(frame_im), G_d' the static
 * part with the frame already subtracted) by gathers: the right-hand side and classic RK4 with one launch per stage.
 *
 * Slot (row r, slot s), s < width:  cols[r * width + s], ops[r * width + s], vals[r * width + s]  (row major).
 *   ops: 0 .. k-1 = operator j (coefficient c_j), k = the static part (coefficient 1);
 *   the slots of a row are GROUPED by operator index (all slots of one index adjacent);
 *   unused slots are (col = r, op = k, val = 0) and come last in their row.
 * midyn_spmv_create checks 0 <= col < n and 0 <= op <= k for every slot and refuses the structure otherwise.
 *
 * Context options (midyn_ctx_set_option; default in brackets):
 *   spmv_lanes [0]   lane mapping of the stage kernels: 1 = lanes are (row, column) pairs (spmv_rows_kernel: one trajectory
 *                    or a few state columns), 2 = lanes are 64 state columns of one row (spmv_cols_kernel: sweeps),
 *                    0 = by the number of state columns B m (profiles/spmv_sweep.md)
 * Counters (midyn_get_counters): "rhs_spmv" counts the stage launches (profile on).
 * Same conventions as midyn.h: complex is interleaved (re, im), matrices row major, 0 = success, text of the last error
 * from midyn_last_error.
 */
#ifndef MIDYN_SPMV_H
#define MIDYN_SPMV_H

#include "midyn.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct midyn_spmv midyn_spmv;
/* frame_im: n doubles or NULL (no frame). */
int midyn_spmv_create(midyn_ctx* ctx, int n, int k, int width, const int* cols, const int* ops,
                      const midyn_complex* vals, const double* frame_im, midyn_spmv** out);
int midyn_spmv_destroy(midyn_spmv* s);
/* info[7] = n, n_pad (rows of the slot-major image), k, width, has_frame, non-zero slots, device bytes of the structure */
int midyn_spmv_info(midyn_spmv* s, long long* info);
/* out [n][m] = rhs(t, y [n][m]); coeffs: k doubles (NULL when k == 0). */
int midyn_spmv_eval_rhs(midyn_spmv* s, const double* coeffs, double t, const midyn_complex* y, int m,
                        midyn_complex* out);
/* times, S[B][R][k] (host OR device pointer), step_rows, step_h, step_save, P, y0, y0_shared, Y_out[B][P][n][m]: exactly as
 * documented for midyn_rk4_solve in midyn.h.  The state buffers (a small multiple of B m n 16 bytes) and the result block
 * are compared with the free device memory before anything is allocated. */
int midyn_spmv_rk4_solve(midyn_spmv* s, int B, int m, int R, const double* times, const double* S,
                         int nsteps, const int* step_rows, const double* step_h, const int* step_save,
                         int P, const midyn_complex* y0, int y0_shared, midyn_complex* Y_out);

#ifdef __cplusplus
}
#endif

#endif /* MIDYN_SPMV_H */
