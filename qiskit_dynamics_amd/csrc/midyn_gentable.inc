// midyn_gentable.inc -- part of midyn.hip (one translation unit; included in order): LMDEs whose generator is a host callable
// (include/midyn_gentable.h).  The caller samples G at the times of the fixed-step schedule and pushes the samples (rows) in
// order; every chunk of steps whose rows are all present runs asynchronously while the caller samples the next rows:
//   1. the rows the chunk reads, [lo, hi], go from the library's pinned ring through one of two pinned staging halves to
//      one of two device buffers (a half is refilled only after the event of its previous copy has completed),
//   2. gentable_gather_kernel writes h_i G[row(i, point)] zero-padded to n_pad for every step i and quadrature point,
//   3. the step propagators: Magnus 1/2/3 + batched expm, or RK4 (form_step_propagators, midyn_parallel.inc),
//   4. applied: tree products between output times (tree_apply_chunk), or in step order -- gen_chain_kernel (all steps of
//      the chunk in one launch) or one batched zgemm per step (n_pad > 128, m > 32, or ctx option gentable_chain = 0).
// Host and device memory for rows is bounded by a few chunk spans of rows, whatever the number of steps.
// -------------------------------------------------------------------------------------------------

// out[i][r][c] = scale h[i] G[rows[i] - row_lo][r][c] for r, c < n, zero on the padding up to np.  raw: [span][n][n].
MIDYN_GLOBAL __launch_bounds__(256) void gentable_gather_kernel(const double2* raw, int row_lo, const int* rows,
                                                                const double* h, double scale, int nb, int n, int np,
                                                                double2* out) {
    const size_t mat = (size_t)np * np;
    const size_t total = (size_t)nb * mat;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        const int i = (int)(idx / mat);
        const int rem = (int)(idx - (size_t)i * mat);
        const int r = rem / np, c = rem - (rem / np) * np;
        double2 v = make_double2(0.0, 0.0);
        if (r < n && c < n) {
            const double f = scale * h[i];
            const double2 g = raw[((size_t)(rows[i] - row_lo) * n + r) * n + c];
            v = make_double2(f * g.x, f * g.y);
        }
        out[idx] = v;
    }
}

// y <- U[i] y for i = 0 .. nb-1 in order, for the state columns [col0, col0 + COLS) of y ([NP][ld]); col0 = COLS blockIdx.x.
// The state is double-buffered in LDS (one barrier per step); U[i] ([NP][NP]) is streamed from global memory once per
// workgroup per step, in panels of 8 k whose loads are issued one panel ahead of the math (the next step's first panel
// during the last panel of a step).  The k index of the products is permuted so that every lane reads a contiguous run
// of its row of U: k-step s of lane quarter q is k = q KQ + s.  A saved state (save[i] >= 0) goes straight from the
// registers to out[save[i]][n][m].
//   COLS = 16: 4 waves, wave w computes rows [w NP/4, (w+1) NP/4) x 16 columns with v_mfma_f64_16x16x4 (4 real MFMAs per
//              complex product: componentwise error bound, like the combine route);
//   COLS = 1:  NP threads, thread r computes row r by VALU FMAs (the state is an LDS broadcast).
template <int NP, int COLS>
__global__ __launch_bounds__(COLS == 1 ? NP : 256) void gen_chain_kernel(const double2* __restrict__ U, int nb,
                                                                        double2* y, int ld, const int* save, int n,
                                                                        int m, double2* out) {
    constexpr int PANEL = 8;
    __shared__ double2 ys[2][NP][COLS];
    const int tid = threadIdx.x;
    const int col0 = blockIdx.x * COLS;
    const size_t mat = (size_t)NP * NP;
    for (int e = tid; e < NP * COLS; e += blockDim.x) {
        const int r = e / COLS, c = e - (e / COLS) * COLS;
        ys[0][r][c] = col0 + c < ld ? y[(size_t)r * ld + col0 + c] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    int cur = 0;
    if constexpr (COLS == 1) {
        constexpr int NPAN = NP / PANEL;
        static_assert(NPAN % 2 == 0, "panel 0 of every step must use buffer 0");
        const int r = tid;
        double2 a[2][PANEL];
        auto load = [&](double2 (&dst)[PANEL], int step, int p) {
            const double2* src = U + (size_t)step * mat + (size_t)r * NP + p * PANEL;
#pragma unroll
            for (int j = 0; j < PANEL; ++j) dst[j] = src[j];
        };
        load(a[0], 0, 0);
        for (int i = 0; i < nb; ++i) {
            double2 acc0 = make_double2(0.0, 0.0), acc1 = make_double2(0.0, 0.0);
#pragma unroll
            for (int p = 0; p < NPAN; ++p) {
                if (p + 1 < NPAN) load(a[(p + 1) & 1], i, p + 1);
                else load(a[0], i + 1 < nb ? i + 1 : i, 0);
#pragma unroll
                for (int j = 0; j < PANEL; j += 2) {
                    const double2 u0 = a[p & 1][j], u1 = a[p & 1][j + 1];
                    const double2 v0 = ys[cur][p * PANEL + j][0], v1 = ys[cur][p * PANEL + j + 1][0];
                    acc0.x = fma(u0.x, v0.x, fma(-u0.y, v0.y, acc0.x));
                    acc0.y = fma(u0.x, v0.y, fma(u0.y, v0.x, acc0.y));
                    acc1.x = fma(u1.x, v1.x, fma(-u1.y, v1.y, acc1.x));
                    acc1.y = fma(u1.x, v1.y, fma(u1.y, v1.x, acc1.y));
                }
            }
            const double2 res = make_double2(acc0.x + acc1.x, acc0.y + acc1.y);
            ys[cur ^ 1][r][0] = res;
            const int sv = save[i];
            if (sv >= 0 && r < n && col0 < m) out[((size_t)sv * n + r) * m + col0] = res;
            __syncthreads();
            cur ^= 1;
        }
        y[(size_t)r * ld + col0] = ys[cur][r][0];
    } else {
        static_assert(COLS == 16, "COLS is 1 or 16");
        constexpr int KQ = NP / 4;          // k-steps of 4 per product
        constexpr int NPAN = KQ / PANEL;
        constexpr int MT = NP / 64;         // 16-row tiles per wave
        static_assert(NPAN % 2 == 0, "panel 0 of every step must use buffer 0");
        const int lane = tid & 63, wave = tid >> 6;
        const int li = lane & 15, q = lane >> 4;
        const int row0 = wave * (NP / 4);
        double2 a[2][MT][PANEL];
        auto load = [&](double2 (&dst)[MT][PANEL], int step, int p) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const double2* src = U + (size_t)step * mat + (size_t)(row0 + mt * 16 + li) * NP + q * KQ + p * PANEL;
#pragma unroll
                for (int j = 0; j < PANEL; ++j) dst[mt][j] = src[j];
            }
        };
        load(a[0], 0, 0);
        for (int i = 0; i < nb; ++i) {
            d4 cre[MT], cim[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) cre[mt] = cim[mt] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int p = 0; p < NPAN; ++p) {
                if (p + 1 < NPAN) load(a[(p + 1) & 1], i, p + 1);
                else load(a[0], i + 1 < nb ? i + 1 : i, 0);
#pragma unroll
                for (int j = 0; j < PANEL; ++j) {
                    const double2 b = ys[cur][q * KQ + p * PANEL + j][li];
                    const double bin = -b.y;
#pragma unroll
                    for (int mt = 0; mt < MT; ++mt) {
                        const double2 u = a[p & 1][mt][j];
                        cre[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(u.x, b.x, cre[mt], 0, 0, 0);
                        cre[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(u.y, bin, cre[mt], 0, 0, 0);
                        cim[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(u.x, b.y, cim[mt], 0, 0, 0);
                        cim[mt] = __builtin_amdgcn_mfma_f64_16x16x4f64(u.y, b.x, cim[mt], 0, 0, 0);
                    }
                }
            }
            const int sv = save[i];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int r = row0 + mt * 16 + q + 4 * g;   // D[row = (lane >> 4) + 4 reg][col = lane & 15]
                    const double2 res = make_double2(cre[mt][g], cim[mt][g]);
                    ys[cur ^ 1][r][li] = res;
                    if (sv >= 0 && r < n && col0 + li < m) out[((size_t)sv * n + r) * m + col0 + li] = res;
                }
            __syncthreads();
            cur ^= 1;
        }
        for (int e = tid; e < NP * COLS; e += blockDim.x) {
            const int r = e / COLS, c = e - (e / COLS) * COLS;
            if (col0 + c < ld) y[(size_t)r * ld + col0 + c] = ys[cur][r][c];
        }
    }
}

template __global__ void gen_chain_kernel<64, 1>(const double2*, int, double2*, int, const int*, int, int, double2*);
template __global__ void gen_chain_kernel<64, 16>(const double2*, int, double2*, int, const int*, int, int, double2*);
template __global__ void gen_chain_kernel<128, 1>(const double2*, int, double2*, int, const int*, int, int, double2*);
template __global__ void gen_chain_kernel<128, 16>(const double2*, int, double2*, int, const int*, int, int, double2*);

enum { GT_ROUTE_CHAIN = 0, GT_ROUTE_PER_STEP = 1, GT_ROUTE_TREE = 2 };

struct midyn_gentable {
    midyn_ctx* ctx = nullptr;
    int n = 0, m = 0, R = 0, nsteps = 0, P = 0, method = 1, parallel = 0;
    int np = 0, ld = 0, npts = 1, route = GT_ROUTE_PER_STEP, cap = 1;
    bool failed = false, finished = false;
    int pushed = 0, next_chunk = 0, cur = 0, largest = 0;
    std::vector<int> save;                     // [nsteps]
    std::vector<int> c0, lo, hi, ready;        // per chunk: first step (c0 has nchunks + 1 entries), rows read, rows needed
    int ring_rows = 0, span_rows = 0;
    double2* ring = nullptr;                   // pinned, rows [row % ring_rows]
    double2* staging[2] = {nullptr, nullptr};  // pinned, span_rows rows each
    hipEvent_t ev[2] = {nullptr, nullptr};
    bool ev_live[2] = {false, false};
    DevBuf d_raw[2], d_rows, d_h, d_save, X, G[3], W[4], d_offs, d_y[2], d_tmp, d_out;
    ExpmWork w;
    std::vector<int> loc, round_start;
    std::vector<long long> offs;
};

static void gentable_release(midyn_gentable* g) {
    if (g->ctx) {
        hipSetDevice(g->ctx->device);
        hipStreamSynchronize(g->ctx->stream);   // nothing in flight may still read what is freed below
    }
    for (int h = 0; h < 2; ++h) {
        if (g->ev[h]) hipEventDestroy(g->ev[h]);
        if (g->staging[h]) hipHostFree(g->staging[h]);
        g->ev[h] = nullptr;
        g->staging[h] = nullptr;
    }
    if (g->ring) hipHostFree(g->ring);
    g->ring = nullptr;
}

// one chunk: rows -> device, propagators, application (asynchronous except for the norm read of the expm and the
// offset table of the tree)
static int gentable_run_chunk(midyn_gentable* g, int c) {
    midyn_ctx* ctx = g->ctx;
    const int a = g->c0[c], nb = g->c0[c + 1] - a;
    const int np = g->np;
    const size_t nn = (size_t)g->n * g->n, mat = (size_t)np * np;
    const int span = g->hi[c] - g->lo[c] + 1;
    const int half = c & 1;
    // -- 1. rows [lo, hi] -> staging half -> device (the half's previous copy must have completed)
    if (g->ev_live[half]) HIPCHK(ctx, hipEventSynchronize(g->ev[half]));
    for (int r = g->lo[c]; r <= g->hi[c]; ++r)
        memcpy(g->staging[half] + (size_t)(r - g->lo[c]) * nn, g->ring + (size_t)(r % g->ring_rows) * nn,
               nn * sizeof(double2));
    HIPCHK(ctx, hipMemcpyAsync(g->d_raw[half].p, g->staging[half], (size_t)span * nn * sizeof(double2),
                               hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipEventRecord(g->ev[half], ctx->stream));
    g->ev_live[half] = true;
    // -- 2. + 3. h_i G at every point, step propagators -> X[0..nb)
    const double* hvec = g->d_h.as<double>() + a;
    const double2* raw = g->d_raw[half].as<double2>();
    const int row_lo = g->lo[c];
    auto gen = [&](int gi, double scale, double2* out) {
        hipLaunchKernelGGL(gentable_gather_kernel, dim3(grid_for((size_t)nb * mat)), dim3(256), 0, ctx->stream, raw,
                           row_lo, g->d_rows.as<int>() + (size_t)gi * g->nsteps + a, hvec, scale, nb, g->n, np, out);
        HIPCHK(ctx, hipGetLastError());
        return 0;
    };
    double2* Xb = g->X.as<double2>();
    CHK(form_step_propagators(ctx, np, nb, g->method, gen, g->G, g->W, g->w, Xb));
    // -- 4. apply
    const int* save = g->save.data() + a;
    if (g->route == GT_ROUTE_TREE) {
        CHK(tree_apply_chunk(ctx, np, g->ld, nb, g->cap, save, Xb, g->d_offs, g->d_y, g->cur, g->n, g->m, g->P,
                             g->d_out.as<double2>(), g->loc, g->offs, g->round_start));
    } else if (g->route == GT_ROUTE_CHAIN) {
        ProfScope ps(ctx, KC_GEN_CHAIN);
        const int* dsave = g->d_save.as<int>() + a;
        double2* y = g->d_y[g->cur].as<double2>();
#define MIDYN_CHAIN(NP_, COLS_)                                                                                         \
    do {                                                                                                                \
        note_variant("gen_chain_kernel", {NP_, COLS_});                                                                 \
        hipLaunchKernelGGL((gen_chain_kernel<NP_, COLS_>), dim3((g->m + COLS_ - 1) / COLS_), dim3(COLS_ == 1 ? NP_ : 256), \
                           0, ctx->stream, (const double2*)Xb, nb, y, g->ld, dsave, g->n, g->m, g->d_out.as<double2>()); \
    } while (0)
        if (np == 64 && g->m == 1) MIDYN_CHAIN(64, 1);
        else if (np == 64) MIDYN_CHAIN(64, 16);
        else if (g->m == 1) MIDYN_CHAIN(128, 1);
        else MIDYN_CHAIN(128, 16);
#undef MIDYN_CHAIN
        HIPCHK(ctx, hipGetLastError());
    } else {
        const size_t inst_elems = (size_t)g->n * g->m;
        for (int i = 0; i < nb; ++i) {
            CHK(dev_zgemm(ctx, np, g->ld, np, Xb + (size_t)i * mat, np, g->d_y[g->cur].as<double2>(), g->ld,
                          g->d_y[g->cur ^ 1].as<double2>(), g->ld, 1.0, 0.0, nullptr));
            g->cur ^= 1;
            if (save[i] >= 0) {
                hipLaunchKernelGGL(gather_state_kernel, dim3(grid_for(inst_elems)), dim3(256), 0, ctx->stream,
                                   g->d_y[g->cur].as<double2>(), 1, g->n, g->m, g->ld, g->P, save[i],
                                   g->d_out.as<double2>());
                HIPCHK(ctx, hipGetLastError());
            }
        }
    }
    return 0;
}

static int gentable_create(midyn_ctx* ctx, int n, int m, int R, int nsteps, const int* step_rows, const double* step_h,
                           const int* step_save, int P, int method, int parallel, const midyn_complex* y0,
                           midyn_gentable* g) {
    g->ctx = ctx;
    g->n = n;
    g->m = m;
    g->R = R;
    g->nsteps = nsteps;
    g->P = P;
    g->method = method;
    g->parallel = parallel;
    g->np = round_up(n, 64);
    g->ld = round_up(m, 64);
    g->npts = method == 0 ? 3 : method;
    const int np = g->np;
    const size_t nn = (size_t)n * n, mat = (size_t)np * np;
    g->route = parallel ? GT_ROUTE_TREE
                        : (ctx->gentable_chain && np <= 128 && m <= 32 ? GT_ROUTE_CHAIN : GT_ROUTE_PER_STEP);
    // steps per chunk: the expm workspace bound, the caller's cap, and ~128 MB per staging half
    long long cap = expm_chunk(ctx, np, std::max(1, nsteps));
    if (ctx->gentable_chunk > 0) cap = std::min<long long>(cap, ctx->gentable_chunk);
    cap = std::min<long long>(cap, std::max<long long>(1, ((size_t)128 << 20) / ((size_t)g->npts * nn * sizeof(double2))));
    g->cap = (int)std::max<long long>(1, cap);
    // chunks, the rows each reads, and when it is ready (prefix maximum of the rows up to its last step, + 1)
    g->save.assign(step_save, step_save + nsteps);
    int pref = -1;
    for (int s0 = 0; s0 < nsteps; s0 += g->cap) {
        const int e = std::min(nsteps, s0 + g->cap);
        int l = R, h = -1;
        for (int s = s0; s < e; ++s)
            for (int gi = 0; gi < g->npts; ++gi) {
                l = std::min(l, step_rows[3 * s + gi]);
                h = std::max(h, step_rows[3 * s + gi]);
            }
        pref = std::max(pref, h);
        g->c0.push_back(s0);
        g->lo.push_back(l);
        g->hi.push_back(h);
        g->ready.push_back(pref + 1);
        g->largest = std::max(g->largest, e - s0);
        g->span_rows = std::max(g->span_rows, h - l + 1);
    }
    const int nchunks = (int)g->lo.size();
    g->c0.push_back(nsteps);
    // ring: when row r arrives, the chunks not yet run are those with ready > r (a suffix); they read rows >= their lo
    std::vector<int> sufmin(nchunks + 1, R);
    for (int c = nchunks - 1; c >= 0; --c) sufmin[c] = std::min(sufmin[c + 1], g->lo[c]);
    g->ring_rows = 1;
    for (int r = 0, c = 0; r < R; ++r) {
        while (c < nchunks && g->ready[c] <= r) ++c;
        if (c < nchunks) g->ring_rows = std::max(g->ring_rows, r - sufmin[c] + 1);
    }
    g->span_rows = std::max(1, g->span_rows);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipHostMalloc((void**)&g->ring, (size_t)g->ring_rows * nn * sizeof(double2), hipHostMallocDefault));
    for (int h = 0; h < 2; ++h) {
        HIPCHK(ctx, hipHostMalloc((void**)&g->staging[h], (size_t)g->span_rows * nn * sizeof(double2), hipHostMallocDefault));
        HIPCHK(ctx, hipEventCreateWithFlags(&g->ev[h], hipEventDisableTiming));
        CHK(g->d_raw[h].alloc(ctx, (size_t)g->span_rows * nn * sizeof(double2)));
    }
    // step tables ([point][step]), workspace, state, results
    const int ns = std::max(1, nsteps);
    std::vector<int> rows_t((size_t)3 * ns);
    for (int s = 0; s < nsteps; ++s)
        for (int gi = 0; gi < 3; ++gi) rows_t[(size_t)gi * nsteps + s] = step_rows[3 * s + gi];
    CHK(g->d_rows.alloc(ctx, rows_t.size() * sizeof(int)));
    CHK(g->d_h.alloc(ctx, (size_t)ns * sizeof(double)));
    CHK(g->d_save.alloc(ctx, (size_t)ns * sizeof(int)));
    if (nsteps > 0) {
        HIPCHK(ctx, hipMemcpy(g->d_rows.p, rows_t.data(), rows_t.size() * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(ctx, hipMemcpy(g->d_h.p, step_h, (size_t)nsteps * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(ctx, hipMemcpy(g->d_save.p, step_save, (size_t)nsteps * sizeof(int), hipMemcpyHostToDevice));
    }
    const int cp = std::max(1, std::min(g->cap, g->largest));
    g->cap = cp;
    CHK(g->X.alloc(ctx, (g->route == GT_ROUTE_TREE ? 2 : 1) * (size_t)cp * mat * sizeof(double2)));
    const int n_g = method == 0 ? 3 : (method == 1 ? 0 : method);
    const int n_w = method == 0 ? 3 : (method == 2 ? 2 : (method == 3 ? 4 : 0));
    for (int i = 0; i < n_g; ++i) CHK(g->G[i].alloc(ctx, (size_t)cp * mat * sizeof(double2)));
    for (int i = 0; i < n_w; ++i) CHK(g->W[i].alloc(ctx, (size_t)cp * mat * sizeof(double2)));
    if (g->route == GT_ROUTE_TREE) CHK(g->d_offs.alloc(ctx, (size_t)3 * cp * sizeof(long long)));
    g->loc.assign(cp, 0);
    const size_t stv = (size_t)np * g->ld, inst_elems = (size_t)n * m;
    CHK(g->d_y[0].alloc(ctx, stv * sizeof(double2)));
    CHK(g->d_y[1].alloc(ctx, stv * sizeof(double2)));
    CHK(g->d_tmp.alloc(ctx, inst_elems * sizeof(double2)));
    CHK(g->d_out.alloc(ctx, (size_t)P * inst_elems * sizeof(double2)));
    HIPCHK(ctx, hipMemsetAsync(g->d_out.p, 0, g->d_out.bytes, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(g->d_y[0].p, 0, stv * sizeof(double2), ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(g->d_y[1].p, 0, stv * sizeof(double2), ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(g->d_tmp.p, y0, inst_elems * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(scatter_state_kernel, dim3(grid_for(inst_elems)), dim3(256), 0, ctx->stream, g->d_tmp.as<double2>(),
                       1, 1, n, m, g->ld, (const double2*)nullptr, g->d_y[0].as<double2>(), (double2*)nullptr);
    hipLaunchKernelGGL(gather_state_kernel, dim3(grid_for(inst_elems)), dim3(256), 0, ctx->stream, g->d_y[0].as<double2>(),
                       1, n, m, g->ld, P, 0, g->d_out.as<double2>());
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // y0 is the caller's (pageable) buffer
    ctx->last_gentable[0] = nchunks;
    ctx->last_gentable[1] = g->largest;
    ctx->last_gentable[2] = (double)(g->ring_rows + 2.0 * g->span_rows) * nn * sizeof(double2);
    ctx->last_gentable[3] = 2.0 * g->span_rows * nn * sizeof(double2);
    return 0;
}

extern "C" int midyn_gentable_create(midyn_ctx* ctx, int n, int m, int R, int nsteps, const int* step_rows,
                                     const double* step_h, const int* step_save, int P, int method, int parallel,
                                     const midyn_complex* y0, midyn_gentable** out) {
    if (!ctx || !out || !y0 || (nsteps > 0 && (!step_rows || !step_h || !step_save)))
        return fail(ctx, "midyn_gentable_create: NULL argument");
    *out = nullptr;
    if (n <= 0 || m <= 0 || R <= 0 || P < 1 || nsteps < 0) return fail(ctx, "midyn_gentable_create: bad sizes");
    if (n > 4096) return fail(ctx, "midyn_gentable_create: n > 4096 is not supported");
    if (parallel != 0 && parallel != 1) return fail(ctx, "midyn_gentable_create: parallel must be 0 or 1");
    if (method < 0 || method > 3) return fail(ctx, "midyn_gentable_create: method must be 0 (RK4) or a Magnus order 1..3");
    if (method == 0 && !parallel)
        return fail(ctx, "midyn_gentable_create: RK4 step propagators (method 0) need parallel == 1");
    for (int i = 0; i < 3 * nsteps; ++i)
        if (step_rows[i] < 0 || step_rows[i] >= R) return fail(ctx, "midyn_gentable_create: step_rows out of range");
    for (int i = 0; i < nsteps; ++i) {
        if (step_save[i] < -1 || step_save[i] >= P) return fail(ctx, "midyn_gentable_create: save slot out of range");
        if (!std::isfinite(step_h[i])) return fail(ctx, "midyn_gentable_create: non-finite step size");
    }
    midyn_gentable* g = new midyn_gentable();
    const int st = gentable_create(ctx, n, m, R, nsteps, step_rows, step_h, step_save, P, method, parallel, y0, g);
    if (st != 0) {
        const std::string msg = ctx->err;
        gentable_release(g);
        delete g;
        return fail(ctx, msg);
    }
    *out = g;
    return 0;
}

extern "C" int midyn_gentable_push(midyn_gentable* g, int row0, int nrows, const midyn_complex* G) {
    if (!g) return fail(nullptr, "midyn_gentable_push: NULL handle");
    midyn_ctx* ctx = g->ctx;
    if (g->failed) return fail(ctx, "midyn_gentable_push: the object failed earlier; only midyn_gentable_destroy is accepted");
    if (g->finished) return fail(ctx, "midyn_gentable_push: the solve has finished");
    if (!G || nrows < 0) return fail(ctx, "midyn_gentable_push: bad argument");
    if (row0 != g->pushed) {
        g->failed = true;
        return fail(ctx, "midyn_gentable_push: out-of-order push (row0 = " + std::to_string(row0) + ", " +
                             std::to_string(g->pushed) + " rows pushed so far)");
    }
    if ((long long)row0 + nrows > g->R) {
        g->failed = true;
        return fail(ctx, "midyn_gentable_push: rows beyond R = " + std::to_string(g->R));
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)g->n * g->n;
    const double2* src = reinterpret_cast<const double2*>(G);
    for (int i = 0; i < nrows; ++i) {
        memcpy(g->ring + (size_t)(g->pushed % g->ring_rows) * nn, src + (size_t)i * nn, nn * sizeof(double2));
        ++g->pushed;
        while (g->next_chunk < (int)g->lo.size() && g->ready[g->next_chunk] <= g->pushed) {
            const int st = gentable_run_chunk(g, g->next_chunk);
            if (st != 0) {
                g->failed = true;
                return st;
            }
            ++g->next_chunk;
        }
    }
    return 0;
}

extern "C" int midyn_gentable_info(midyn_gentable* g, long long* info) {
    if (!g || !info) return fail(g ? g->ctx : nullptr, "midyn_gentable_info: NULL argument");
    info[0] = g->cap;
    info[1] = g->lo.empty() ? g->R : std::max(1, std::min(g->R, g->ready[0]));
    info[2] = g->np;
    info[3] = g->route;
    return 0;
}

extern "C" int midyn_gentable_finish(midyn_gentable* g, midyn_complex* Y_out) {
    if (!g) return fail(nullptr, "midyn_gentable_finish: NULL handle");
    midyn_ctx* ctx = g->ctx;
    if (g->failed) return fail(ctx, "midyn_gentable_finish: the object failed earlier; only midyn_gentable_destroy is accepted");
    if (!Y_out) return fail(ctx, "midyn_gentable_finish: NULL argument");
    if (g->pushed != g->R) {
        g->failed = true;
        return fail(ctx, "midyn_gentable_finish: only " + std::to_string(g->pushed) + " of " + std::to_string(g->R) +
                             " rows pushed");
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (g->next_chunk != (int)g->lo.size()) {   // (every chunk is ready once all rows are in: run as they became ready)
        g->failed = true;
        return fail(ctx, "midyn_gentable_finish: internal: chunks left after the last row");
    }
    const hipError_t e1 = hipStreamSynchronize(ctx->stream);
    const hipError_t e2 = e1 == hipSuccess ? hipMemcpy(Y_out, g->d_out.p, g->d_out.bytes, hipMemcpyDeviceToHost) : e1;
    if (e2 != hipSuccess) {
        g->failed = true;
        return fail(ctx, std::string("midyn_gentable_finish: ") + hipGetErrorString(e2));
    }
    g->finished = true;
    return 0;
}

extern "C" int midyn_gentable_destroy(midyn_gentable* g) {
    if (!g) return 0;
    gentable_release(g);
    delete g;
    return 0;
}
