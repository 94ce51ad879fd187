/*
 * midyn_gentable.h -- C-ABI of libmidyn.so for LMDEs whose generator is a host CALLABLE G(t) (the reference's
 * solve_lmde / scipy_expm_solver with a plain function, solvers/solver_functions.py:220-373,
 * solvers/fixed_step_solvers.py:80-108).  Every time a fixed-step LMDE method evaluates G at is known before the solve
 * starts, so the caller samples G there and streams the samples ("rows") to the library, which does everything else on
 * the device: Magnus 1/2/3 (or RK4) step propagators, expm, and either the propagators applied to the state in step order
 * or the binary-tree products between output times, as midyn_parallel_solve forms them.
 *
 * Usage:   create -> push rows in order (any block sizes) -> finish -> destroy.  Chunks of steps whose rows are all
 * present run asynchronously while the caller samples the next rows; host and device memory for samples is bounded by
 * a few chunks of rows, whatever the number of steps.
 *
 * Context options (midyn_ctx_set_option; defaults in brackets):
 *   gentable_chain [1]   sequential route, n_pad <= 128 and m <= 32: all steps of a chunk applied to the state by ONE
 *                        launch of gen_chain_kernel; 0: one batched zgemm per step (A/B, fallback test)
 *   gentable_chunk [0]   > 0: at most this many steps per chunk (tests of chunk / push boundaries at small sizes)
 * Counters (midyn_get_counters): "gen_chain" counts the launches of gen_chain_kernel (profile on); "gentable_info" ->
 * (chunks of the last solve, steps in its largest chunk); "gentable_staging" -> (bytes of pinned host staging, bytes of
 * device memory for raw rows) of the last solve.
 * Same conventions as midyn.h: complex is interleaved (re, im), matrices row major, 0 = success.
 */
#ifndef MIDYN_GENTABLE_H
#define MIDYN_GENTABLE_H

#include "midyn.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct midyn_gentable midyn_gentable;
/* method: 1..3 = Magnus order, 0 = RK4 step propagators (parallel == 1 only).
 * parallel: 0 = apply the step propagators to y0 in step order, 1 = tree products between output times.
 * step_rows / step_h / step_save / P: as for midyn_expm_solve and midyn_parallel_solve; save slot 0 = y0.
 * step s is ready once every row up to max(step_rows of steps 0..s) has been pushed (a prefix maximum: a zero-length
 * t_eval interval may read an earlier row again, so rows need not be monotone).
 * y0 [n][m] row-major; Y_out [P][n][m]. */
int midyn_gentable_create(midyn_ctx* ctx, int n, int m, int R, int nsteps, const int* step_rows, const double* step_h,
                          const int* step_save, int P, int method, int parallel, const midyn_complex* y0,
                          midyn_gentable** out);
/* rows [row0, row0 + nrows) of the sampled generator, [nrows][n][n] row-major; row0 must equal the rows pushed so far.
 * Copies into the library's pinned staging before returning, so the caller may reuse its buffer. Every step whose rows
 * are all present becomes ready, and full chunks of ready steps are launched asynchronously. */
int midyn_gentable_push(midyn_gentable* g, int row0, int nrows, const midyn_complex* G);
/* (steps per chunk, suggested rows per push, n_pad, route: 0 sequential+chain, 1 sequential+per-step apply, 2 tree) */
int midyn_gentable_info(midyn_gentable* g, long long* info);
/* all R rows pushed: runs the remaining steps, waits, writes Y_out */
int midyn_gentable_finish(midyn_gentable* g, midyn_complex* Y_out);
int midyn_gentable_destroy(midyn_gentable* g);   /* safe at any point, including after an error or mid-stream */

#ifdef __cplusplus
}
#endif

#endif /* MIDYN_GENTABLE_H */
