// midyn_spmv.h -- gather kernels of the sparse-operator route (include/midyn_spmv.h; host side: midyn_spmv.inc).
//
// The operators G_0 .. G_{k-1} and the static part (operator index k, coefficient 1) are merged into ONE padded row
// structure of W slots per row: slot = (column, operator index, value), a row's slots grouped by operator index, unused
// slots (col = row, op = k, val = 0) last.  rhs(t, y) = conj(e(t)) o [ (G_d' + sum_j c_j G_j) (e(t) o y) ], e = exp(i F t).
//
// State columns: column c = b m + j is column j of instance b; every state buffer is [n][ld].  The stage input x is stored
// ALREADY multiplied by e(t_stage) (written so by the epilogue of the stage before), a row's sum is multiplied by
// conj(e(t_stage)) once: a slot costs one gather and one complex multiply-add.  The phases e(t) of the four times of a step
// and the step's coefficients, transposed to [3][k][ld] so that the lanes of a wave read them contiguously, are made once
// per step by spmv_prep_kernel.
//
// Two lane mappings of the same stage:
//   spmv_cols_kernel   lanes = 64 state columns, one row per wave: slot data wave-uniform (row-major image [n][W]), every
//                      gather one contiguous 1 KB read, the coefficient applied once per operator group (uniform branch);
//   spmv_rows_kernel   lanes = (row, column) pairs, column fastest: slot data from the slot-major image [W][n_pad]
//                      (consecutive rows contiguous), for one trajectory or a few columns.
// The RK4 stage update is the epilogue of the product.  Every output element (row, c) of y, acc, xout and the result block
// belongs to exactly one lane; xout is NEVER the buffer gathered from (the host alternates two x buffers): other
// workgroups still read xin while this one writes.  No barrier, no LDS, no exchange between workgroups; every loop is
// bounded by W.
#pragma once
#include <hip/hip_runtime.h>

namespace midyn {

struct SpmvArgs {
    int n, n_pad, k, W;        // rows, rows of the slot-major image, operators (static part = index k), slots per row
    int C, ld, m, P;           // state columns B m, leading dimension of the state buffers, columns per instance, save slots
    const int* len;            // [n] slots in use per row
    const int* cols;           // image of the mapping that runs: [n][W] (columns kernel) or [W][n_pad] (rows kernel)
    const int* ops;
    const double2* vals;
    const double2* ph_in;      // [n] e(t) of the stage input (NULL: no frame)
    const double2* ph_out;     // [n] e(t) of the NEXT stage's input
    const double* coef;        // [k][ld] coefficients of this stage (NULL when k == 0)
    const double2* xin;        // [n][ld] stage input, pre-phased
    double2* xout;             // [n][ld] next stage input (a different buffer from xin)
    double2* y;                // [n][ld] state at the start of the step
    double2* acc;              // [n][ld] y + h/6 (k1 + 2 k2 + ...) so far
    double2* out;              // [B][P][n][m] result block
    double h;
    int save;                  // STAGE 4: slot the new state is stored in (< 1: not saved); STAGE 0: slot of the rhs
};

__device__ __forceinline__ double2 spmv_cmul(const double2 a, const double2 b) {
    return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ double2 spmv_cmul_conj(const double2 a, const double2 b) {   // conj(a) b
    return make_double2(a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x);
}

// The epilogue of a stage for the element (row, c) whose product sum is `kv` (still in the pre-phased picture).
// STAGE 0: a plain right-hand side, stored in the result block.  STAGE 1..4: classic RK4, y' = y + h/6 (k1 + 2 k2 + 2 k3 + k4).
template <int STAGE>
__device__ __forceinline__ void spmv_epilogue(const SpmvArgs& a, const int row, const int c, double2 kv) {
    if (a.ph_in) kv = spmv_cmul_conj(a.ph_in[row], kv);
    const size_t at = (size_t)row * a.ld + c;
    const size_t at_out = (((size_t)(c / a.m) * a.P + (a.save > 0 ? a.save : 0)) * a.n + row) * a.m + c % a.m;
    if (STAGE == 0) {
        a.out[at_out] = kv;
        return;
    }
    const double2 y = a.y[at];
    double2 next;            // the next stage's input, before its phase
    if (STAGE == 1) {
        const double w = a.h * (1.0 / 6);
        a.acc[at] = make_double2(y.x + w * kv.x, y.y + w * kv.y);
        next = make_double2(y.x + 0.5 * a.h * kv.x, y.y + 0.5 * a.h * kv.y);
    } else if (STAGE == 2 || STAGE == 3) {
        const double w = a.h * (1.0 / 3);
        const double2 s = a.acc[at];
        a.acc[at] = make_double2(s.x + w * kv.x, s.y + w * kv.y);
        const double hn = STAGE == 2 ? 0.5 * a.h : a.h;
        next = make_double2(y.x + hn * kv.x, y.y + hn * kv.y);
    } else {
        const double w = a.h * (1.0 / 6);
        const double2 s = a.acc[at];
        next = make_double2(s.x + w * kv.x, s.y + w * kv.y);
        a.y[at] = next;
        if (a.save > 0) a.out[at_out] = next;
    }
    a.xout[at] = a.ph_out ? spmv_cmul(a.ph_out[row], next) : next;
}

// lanes = state columns: grid = (row groups of 4) x (blocks of 64 columns), row group fastest; 256 threads = 4 waves = 4 rows
template <int STAGE>
__global__ __launch_bounds__(256) void spmv_cols_kernel(const SpmvArgs a) {
    const int row_groups = (a.n + 3) >> 2;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int row = (int)(blockIdx.x % (unsigned)row_groups) * 4 + wave;
    const int c_lane = (int)(blockIdx.x / (unsigned)row_groups) * 64 + (int)(threadIdx.x & 63);
    if (row >= a.n) return;
    const bool live = c_lane < a.C;
    const int c = live ? c_lane : a.C - 1;      // lanes past the last column repeat it and store nothing
    const int len = a.len[row];
    const int* cols = a.cols + (size_t)row * a.W;
    const int* ops = a.ops + (size_t)row * a.W;
    const double2* vals = a.vals + (size_t)row * a.W;
    const double2* xin = a.xin + c;
    double2 tot = make_double2(0.0, 0.0), grp = make_double2(0.0, 0.0);
    double cf = 0.0;
    int cur = -1;
    for (int s = 0; s < len; ++s) {
        const int op = ops[s];
        if (op != cur) {                         // wave-uniform: the slots of a row are grouped by operator
            tot.x += cf * grp.x;
            tot.y += cf * grp.y;
            grp = make_double2(0.0, 0.0);
            cur = op;
            cf = op < a.k ? a.coef[(size_t)op * a.ld + c] : 1.0;
        }
        const double2 v = vals[s];
        const double2 x = xin[(size_t)cols[s] * a.ld];
        grp.x += v.x * x.x - v.y * x.y;
        grp.y += v.x * x.y + v.y * x.x;
    }
    tot.x += cf * grp.x;
    tot.y += cf * grp.y;
    if (live) spmv_epilogue<STAGE>(a, row, c, tot);
}

// lanes = (row, column) pairs, column fastest: grid = ceil(n C / 256) blocks of 256 threads
template <int STAGE>
__global__ __launch_bounds__(256) void spmv_rows_kernel(const SpmvArgs a) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)a.n * a.C) return;
    const int row = (int)(e / (unsigned)a.C);
    const int c = (int)(e - (size_t)row * a.C);
    const int len = a.len[row];
    const double2* xin = a.xin + c;
    double2 tot = make_double2(0.0, 0.0);
    for (int s = 0; s < len; ++s) {
        const size_t at = (size_t)s * a.n_pad + row;
        const int op = a.ops[at];
        const double cf = op < a.k ? a.coef[(size_t)op * a.ld + c] : 1.0;
        const double2 v = a.vals[at];
        const double2 x = xin[(size_t)a.cols[at] * a.ld];
        tot.x += cf * (v.x * x.x - v.y * x.y);
        tot.y += cf * (v.x * x.y + v.y * x.x);
    }
    spmv_epilogue<STAGE>(a, row, c, tot);
}

// Once per step (and once per direct evaluation): e(t_q) = exp(i F t_q) of the step's four times (stage inputs at t, t + h/2,
// t + h, and the start of the NEXT step) into ph[4][n], and the coefficient rows rows[0..2] of the table S[B][R][k]
// transposed into coef[3][k][ld] (column c reads instance c / m).
struct SpmvPrepArgs {
    int n, k, C, ld, m, R;
    const double* frame_im;    // [n] or NULL
    const double* S;           // [B][R][k] or NULL
    double2* ph;               // [4][n]
    double* coef;              // [3][k][ld]
    double t[4];
    int rows[3];
};

__global__ void spmv_prep_kernel(const SpmvPrepArgs a);
#ifdef MIDYN_TU_SPMV       // (not a template: defined in the one unit that instantiates the family)
__global__ __launch_bounds__(256) void spmv_prep_kernel(const SpmvPrepArgs a) {
    const size_t stride = (size_t)gridDim.x * 256;
    const size_t first = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (a.frame_im)
        for (size_t i = first; i < (size_t)4 * a.n; i += stride) {
            const int q = (int)(i / (unsigned)a.n);
            const int row = (int)(i - (size_t)q * a.n);
            double s, c;
            sincos(a.frame_im[row] * a.t[q], &s, &c);
            a.ph[i] = make_double2(c, s);
        }
    if (a.S) {
        const size_t per = (size_t)a.k * a.C;
        for (size_t i = first; i < 3 * per; i += stride) {
            const int q = (int)(i / per);
            const size_t r = i - (size_t)q * per;
            const int op = (int)(r / (unsigned)a.C);
            const int c = (int)(r - (size_t)op * a.C);
            a.coef[((size_t)q * a.k + op) * a.ld + c] = a.S[((size_t)(c / a.m) * a.R + a.rows[q]) * a.k + op];
        }
    }
}
#endif

// y0 ([B][n][m], or [n][m] shared by the instances) into the state layout: y = y0, x = e(t_first) o y0, result slot 0 = y0
struct SpmvLoadArgs {
    int n, C, ld, m, P, shared;
    const double2* y0;
    const double2* ph;         // [n] e(t_first) or NULL
    double2* y;                // [n][ld] or NULL (a direct evaluation keeps no y)
    double2* x;
    double2* out;              // [B][P][n][m] or NULL
};

__global__ void spmv_load_kernel(const SpmvLoadArgs a);
#ifdef MIDYN_TU_SPMV
__global__ __launch_bounds__(256) void spmv_load_kernel(const SpmvLoadArgs a) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < (size_t)a.n * a.C; e += stride) {
        const int row = (int)(e / (unsigned)a.C);
        const int c = (int)(e - (size_t)row * a.C);
        const int b = c / a.m, j = c - b * a.m;
        const double2 v = a.y0[((size_t)(a.shared ? 0 : b) * a.n + row) * a.m + j];
        const size_t at = (size_t)row * a.ld + c;
        if (a.y) a.y[at] = v;
        a.x[at] = a.ph ? spmv_cmul(a.ph[row], v) : v;
        if (a.out) a.out[(((size_t)b * a.P) * a.n + row) * a.m + j] = v;
    }
}
#endif

// ---- the instantiations that exist: midyn_tu_spmv.hip defines MIDYN_TU_SPMV -------------------------------------------
#ifdef MIDYN_TU_SPMV
#define MIDYN_SPMV_EXTERN
#else
#define MIDYN_SPMV_EXTERN extern
#endif
#define MIDYN_X(S_)                                                                          \
    MIDYN_SPMV_EXTERN template __global__ void spmv_cols_kernel<S_>(const SpmvArgs);         \
    MIDYN_SPMV_EXTERN template __global__ void spmv_rows_kernel<S_>(const SpmvArgs);
MIDYN_X(0) MIDYN_X(1) MIDYN_X(2) MIDYN_X(3) MIDYN_X(4)
#undef MIDYN_X

}  // namespace midyn
