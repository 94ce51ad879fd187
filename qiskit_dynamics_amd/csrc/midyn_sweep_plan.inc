// midyn_sweep_plan.inc -- part of midyn.hip (one translation unit; included in order): the series helpers of the expm ACTION
// and midyn_expm_plan, the device-resident state of a fixed-step Magnus/expm solve (include/midyn.h: midyn_expm_plan_*).
//
// Reference: solvers/fixed_step_solvers.py:80-108 (scipy_expm_solver), :345-363 (Magnus terms), :406-459 (the fixed-step
// template); a parameter scan calls it once per parameter set with the SAME model and time grid (solver_classes.py:556-590).
//
// A plan holds what such a scan re-uses: the frame-phase table of the time grid, the step tables, y0, the result block, the
// exchange slots and flag words of the one-launch sweep kernels, the Gauss-point phase table -- everything but the coefficient
// table S.  midyn_expm_plan_run(plan, S) uploads S, takes the norm bounds of every step over the instances (ONE small kernel,
// 3 nsteps doubles back through pinned memory), chooses the series of every step on the host, uploads them, fills the slot
// coefficient table and launches; midyn_expm_plan_fetch waits, re-runs on the one-workgroup kernel if a partner wait gave up,
// and copies the saved states out.  midyn_expm_solve on the sweep route IS create + run + fetch + destroy (one code path; round 5
// measured 0.36 ms of host time around a 1.74 ms cfg 5 shard launch, most of it buffers and tables that do not change between
// solves: VERDICT round 5 item 2c).  Solves the one-launch sweep kernels do not take run through midyn_expm_solve itself at
// midyn_expm_plan_run (the plan then only keeps the arguments).
// -------------------------------------------------------------------------------------------------
struct ActionScheme {
    int p;
    double theta;
};
static const ActionScheme ACTION_SCHEMES[] = {{2, 8.0e-6}, {3, 2.0e-4}, {4, 1.5e-3}, {5, 6.0e-3}, {6, 1.6e-2},
                                              {8, 6.5e-2}, {10, 0.16}, {12, 0.3},   {15, 0.62},  {20, 1.35}};

static void action_choose(double bound, int* p_out, int* s_out) {
    long long best_cost = -1;
    for (const ActionScheme& sc : ACTION_SCHEMES) {
        const int s = bound > sc.theta ? (int)std::ceil(bound / sc.theta) : 1;
        const long long cost = (long long)sc.p * s;
        if (best_cost < 0 || cost <= best_cost) {
            best_cost = cost;
            *p_out = sc.p;
            *s_out = s;
        }
    }
}

static int stack_seg_norms(midyn_stack* s) {
    if (!s->seg_norm1.empty()) return 0;
    midyn_ctx* ctx = s->ctx;
    DevBuf cs;
    CHK(dev_norm1(ctx, s->ops, s->n_pad, s->nseg, cs, s->seg_norm1));
    return 0;
}

static int stack_seg_aux_norms(midyn_stack* s) {
    if (!s->seg_herm1.empty()) return 0;
    midyn_ctx* ctx = s->ctx;
    DevBuf cs;
    CHK(dev_norm1(ctx, s->ops, s->n_pad, s->nseg, cs, s->seg_norminf, 1));
    CHK(dev_norm1(ctx, s->ops, s->n_pad, s->nseg, cs, s->seg_herm1, 2));
    return 0;
}

// the per-segment norms step_bounds_kernel reads: [1-norm | infinity norm | 1-norm of the Hermitian part]
static int stack_norm_table(midyn_stack* s, std::vector<double>* nrm) {
    CHK(stack_seg_norms(s));
    CHK(stack_seg_aux_norms(s));
    *nrm = s->seg_norm1;
    nrm->insert(nrm->end(), s->seg_norminf.begin(), s->seg_norminf.end());
    nrm->insert(nrm->end(), s->seg_herm1.begin(), s->seg_herm1.end());
    return 0;
}

// Bessel functions J_0..J_K of the first kind at x > 0 by Miller's backward recurrence (normalised with
// J_0 + 2 sum J_2k = 1); K is chosen by the caller, the recurrence starts far enough above it.
static std::vector<double> bessel_j(double x, int K) {
    const int M = 2 * ((std::max(K, (int)std::ceil(x)) + 40) / 2 + 8);
    std::vector<double> j(M + 2, 0.0);
    j[M] = 1e-280;
    for (int k = M; k >= 1; --k) {
        j[k - 1] = (2.0 * k / x) * j[k] - j[k + 1];
        if (std::fabs(j[k - 1]) > 1e250)
            for (int q = k - 1; q <= M; ++q) j[q] *= 1e-250;
    }
    double norm = j[0];
    for (int k = 2; k <= M; k += 2) norm += 2.0 * j[k];
    j.resize(K + 1);
    for (double& v : j) v /= norm;
    return j;
}

// ---- Chebyshev series for a nearly skew-Hermitian Omega (Hamiltonian models exactly, Lindbladians with weak
// dissipation): with B = Omega / rho, rho >= the numerical radius,
//     expm(Omega) y = J_0(rho) phi_0 + 2 sum_k J_k(rho) phi_k,   phi_0 = y, phi_1 = B y,
//     phi_{k+1} = 2 B phi_k + phi_{k-1}          (phi_k = i^k T_k(B / i) y, Bessel J_k),
// which needs about rho + 10 rho^(1/3) + 10 applications of Omega where the scaled Taylor series needs ~15 rho
// (cfg 4 without a frame, rho = 10.8: 36 instead of 160), no orthogonalisation, sweeps included.  rho comes from
// the larger of the 1-norm and infinity-norm triangle bounds; the series is only used when the Hermitian part
// is small enough that the polynomials cannot grow:  K sqrt(2 ||herm(Omega)|| / rho) <= 0.7.
//
// The series of one step, the one policy of every expm action route and of the sweep plan: the scaled Taylor series (deg, sc)
// is always set -- a caller that cannot run the Chebyshev series falls back to it -- and `cheb` says that the Chebyshev series
// (K, reps, rho, coef) runs instead.
struct StepSeries {
    int deg = 2, sc = 1;        // Taylor: degree, repetitions (action_choose)
    bool cheb = false;
    int reps = 1, K = 0;
    double rho = 0.0;           // bound of the whole Omega; every repetition applies expm(Omega / reps)
    std::vector<double> coef;   // J_k(rho / reps), k = 0..K
};
// taylor_bound >= ||Omega||_1 chooses the Taylor series; rho_bound / herm: the step's bounds of Omega and of its Hermitian part
// (step_bounds_kernel); the Chebyshev series (only when allow_cheb) is for rho = max(cheb_at_least, rho_bound).
// equal_cost: the caller's kernel runs a Chebyshev term for the price of a Taylor term (the one-launch sweep kernels: the
// recurrence's second addend is a register) -- the series is taken as soon as it has fewer terms; elsewhere the Chebyshev
// epilogue reads one more vector per term and the series must be a fifth shorter
static int step_series(midyn_ctx* ctx, int magnus_order, double taylor_bound, double rho_bound, double herm, double cheb_at_least,
                       bool allow_cheb, bool equal_cost, StepSeries* out) {
    *out = StepSeries();
    if (!std::isfinite(taylor_bound)) return fail(ctx, "midyn_expm_solve: non-finite generator norm");
    action_choose(taylor_bound, &out->deg, &out->sc);
    const long long taylor_products = (long long)out->deg * out->sc;
    if (!allow_cheb || !ctx->chebyshev || magnus_order > 2) return 0;
    const double rho = std::max(cheb_at_least, rho_bound);
    if (!(rho > 0.0) || !std::isfinite(rho)) return 0;
    const int reps = std::max(1, (int)std::ceil(rho / 128.0));  // Bessel table accurate to a few 1e-15 up to here
    const double arg = rho / reps;
    const int kmax = (int)(arg + 10.0 * std::cbrt(arg) + 40.0);
    std::vector<double> coef = bessel_j(arg, kmax);
    int K = kmax;
    if (ctx->cheb_tail) {
        // the series ends where everything behind it is below the unit roundoff: ||phi_k|| <= ||y||, so the dropped terms of
        // all `reps` repetitions change the step's result by at most 2 reps sum_{k > K} |J_k| <= 2^-53 -- the backward error
        // the Taylor schemes above (Al-Mohy-Higham thetas) and the reference's Pade approximants (scipy.linalg.expm) are
        // built for.  (Rounds 2-5 cut at |J_k| < 1e-18, a hundred times below what fp64 resolves: one or two terms more per
        // step -- cfg 4: 36 instead of 34; option cheb_tail = 0 restores that rule.)
        double tail = 0.0;
        while (K > 1 && 2.0 * (double)reps * (tail + std::fabs(coef[K])) <= 1.1102230246251565e-16) tail += std::fabs(coef[K--]);
    } else {
        while (K > 1 && std::fabs(coef[K]) < 1e-18) --K;
    }
    if (K >= kmax) return 0;
    const bool stable = (double)K * std::sqrt(2.0 * herm / rho) <= 0.7;
    const bool shorter = equal_cost && ctx->cheb_tail ? (long long)reps * K < taylor_products
                                                      : (long long)reps * (K + 1) * 10 < taylor_products * 8;
    if (!stable || !(shorter || ctx->chebyshev >= 2)) return 0;
    coef.resize(K + 1);
    out->cheb = true;
    out->reps = reps;
    out->K = K;
    out->rho = rho;
    out->coef = std::move(coef);
    return 0;
}

// -------------------------------------------------------------------------------------------------
// midyn_expm_plan
// -------------------------------------------------------------------------------------------------
constexpr int EXPM_PLAN_STRIDE = 232;      // Bessel coefficients per step at most: rho / reps <= 128 -> K < 128 + 10 cbrt(128) + 40

struct midyn_expm_plan {
    midyn_stack* stack = nullptr;
    int B = 0, m = 0, R = 0, nsteps = 0, P = 0, order = 1;
    bool y0_shared = false, has_save = false;
    bool sweep = false;             // the one-launch sweep kernels take this solve (else: midyn_expm_solve at every run)
    std::vector<double> times, hs;
    std::vector<int> rows, save;
    std::vector<midyn_complex> y0;  // host copy: slot 0 of every instance, and the argument of the generic route
    std::vector<midyn_complex> host_result;   // generic route: what midyn_expm_solve returned
    // ---- sweep route: device-resident state
    DevBuf d_S, d_times, d_E, d_y0, d_out, d_static, d_dyn, d_dt, d_stash, d_cab, d_ring, d_nrm, d_bounds;
    const double* dev_hs = nullptr;     // inside d_static: [hs] doubles, then [rows | save] ints
    const int* dev_rows = nullptr;
    const int* dev_save = nullptr;
    double2* out_target = nullptr;      // where the running launch writes its saved states: d_out, or the caller's mapped host block
    bool in_flight = false;             // a launch is on the stream
    bool two_workgroups = false;        // ... and it is a two-workgroup (or split) launch whose partner waits may have given up
    bool have_run = false;
    // result blocks of the caller that hipPointerGetAttributes has shown to be device-writable host memory (the query costs
    // 30-40 us, twice per block: a scan re-uses a handful of pinned blocks).  midyn.h: a block accepted once stays pinned while
    // it is handed to this plan.
    struct MappedBlock {
        const void* host;
        size_t bytes;
        void* dev;
    };
    std::vector<MappedBlock> mapped;
    std::vector<int> Kv, repv;          // series of the last run (host copies: the re-run after a give-up)
    std::vector<double> parv;
    int stride = 0;
};

// the shapes the one-launch sweep kernels exist for (the stack's ELL layout is examined by expm_plan_sweep_route)
static bool expm_sweep_shape(const midyn_stack* s, int B, int m, int magnus_order, int nsteps) {
    const midyn_ctx* ctx = s->ctx;
    return ctx->expm_action && ctx->ell_sweep && m == 1 && magnus_order >= 1 && magnus_order <= 2 && (B > 1 || magnus_order == 2) &&
           ctx->krylov < 2 && nsteps > 0 &&
           ((s->n_pad % SWEEP_THREADS == 0 && s->n_pad <= SWEEP_THREADS * SWEEP_MAX_RPT && s->n_pad != 3 * SWEEP_THREADS) ||
            s->n_pad == 256 || s->n_pad == 512);
}

static int expm_plan_sweep_route(midyn_stack* s, int B, int m, int magnus_order, int nsteps, bool* yes) {
    *yes = false;
    if (!expm_sweep_shape(s, B, m, magnus_order, nsteps)) return 0;
    bool ell_ok = false;
    CHK(stack_ell_usable(s, &ell_ok));
    *yes = s->ell_state == 1 && s->sp_w > 0 && s->sp_w <= SWEEP_MAX_SLOTS;
    return 0;
}

extern "C" int midyn_expm_plan_destroy(midyn_expm_plan* p) {
    if (!p) return 0;
    if (p->stack && p->stack->ctx) {
        hipSetDevice(p->stack->ctx->device);
        hipStreamSynchronize(p->stack->ctx->stream);
    }
    delete p;
    return 0;
}

// the plan the last one-shot midyn_expm_solve left in its stack (ctx option expm_plan_cache)
static void stack_drop_sweep_plan(midyn_stack* s) {
    if (s->sweep_plan) midyn_expm_plan_destroy(s->sweep_plan);
    s->sweep_plan = nullptr;
}

// Is the cached plan of `s` the plan of this one-shot solve?  Same shapes, time grid, step tables and initial states, made under
// the options in force now (any midyn_ctx_set_option call since then retires it: the route choices of a plan are made when it
// is made).  The comparison reads the plan's host copies: 10 KB for cfg 5 plus y0 (64 KB shared; per-instance initial states are
// compared up to 1 MB -- beyond that the comparison would cost what the plan saves, and the plan is not kept).
constexpr size_t EXPM_PLAN_CACHE_Y0_BYTES = 1u << 20;
static bool expm_plan_matches(const midyn_expm_plan* p, const midyn_stack* s, int B, int m, int R, const double* times, int nsteps,
                              const int* step_rows, const double* step_h, const int* step_save, int P, int magnus_order,
                              const midyn_complex* y0, int y0_shared) {
    if (!p || p->stack != s || s->sweep_plan_epoch != s->ctx->options_epoch || !p->sweep) return false;
    if (p->B != B || p->m != m || p->R != R || p->nsteps != nsteps || p->P != P || p->order != magnus_order ||
        p->y0_shared != (y0_shared != 0) || p->has_save != (step_save != nullptr))
        return false;
    const size_t y0_elems = (size_t)(y0_shared ? 1 : B) * s->n * m;
    if (p->y0.size() != y0_elems || y0_elems * sizeof(midyn_complex) > EXPM_PLAN_CACHE_Y0_BYTES) return false;
    return memcmp(p->times.data(), times, (size_t)R * sizeof(double)) == 0 &&
           memcmp(p->hs.data(), step_h, (size_t)nsteps * sizeof(double)) == 0 &&
           memcmp(p->rows.data(), step_rows, (size_t)3 * nsteps * sizeof(int)) == 0 &&
           (!step_save || memcmp(p->save.data(), step_save, (size_t)nsteps * sizeof(int)) == 0) &&
           memcmp(p->y0.data(), y0, y0_elems * sizeof(midyn_complex)) == 0;
}

static int expm_plan_create_impl(midyn_stack* s, int B, int m, int R, const double* times, int nsteps, const int* step_rows,
                                 const double* step_h, const int* step_save, int P, int magnus_order, const midyn_complex* y0,
                                 int y0_shared, midyn_expm_plan** out) {
    midyn_ctx* ctx = s->ctx;
    if (B <= 0 || m <= 0 || R <= 0 || nsteps < 0 || P <= 0) return fail(ctx, "midyn_expm_plan_create: bad sizes");
    if (!times || !step_rows || !step_h || !y0) return fail(ctx, "midyn_expm_plan_create: NULL argument");
    if (magnus_order < 1 || magnus_order > 3) return fail(ctx, "midyn_expm_plan_create: magnus_order must be 1, 2 or 3");
    for (int i = 0; i < 3 * nsteps; ++i)
        if (step_rows[i] < 0 || step_rows[i] >= R) return fail(ctx, "midyn_expm_plan_create: step_rows out of range");
    if (step_save)
        for (int st = 0; st < nsteps; ++st)
            if (step_save[st] >= P || step_save[st] == 0)     // (slot 0 is y0 itself, midyn.h: the host writes it while the kernel runs)
                return fail(ctx, "midyn_expm_solve: save slot out of range (slots 1..P-1; slot 0 always holds y0)");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    midyn_expm_plan* p = new midyn_expm_plan();
    struct Guard {
        midyn_expm_plan* p;
        ~Guard() { if (p) midyn_expm_plan_destroy(p); }
    } guard{p};
    p->stack = s;
    p->B = B;
    p->m = m;
    p->R = R;
    p->nsteps = nsteps;
    p->P = P;
    p->order = magnus_order;
    p->y0_shared = y0_shared != 0;
    p->has_save = step_save != nullptr;
    p->times.assign(times, times + R);
    p->hs.assign(step_h, step_h + nsteps);
    p->rows.assign(step_rows, step_rows + 3 * (size_t)nsteps);
    if (step_save) p->save.assign(step_save, step_save + nsteps);
    const size_t vec = (size_t)s->n * m, y0_elems = (size_t)(y0_shared ? 1 : B) * vec;
    p->y0.assign(y0, y0 + y0_elems);
    CHK(expm_plan_sweep_route(s, B, m, magnus_order, nsteps, &p->sweep));
    if (p->sweep) {
        std::vector<double> nrm;
        CHK(stack_norm_table(s, &nrm));
        const int np = s->n_pad;
        if (s->k > 0) CHK(p->d_S.alloc(ctx, (size_t)B * R * s->k * sizeof(double)));
        CHK(p->d_y0.alloc(ctx, y0_elems * sizeof(double2)));
        CHK(p->d_out.alloc(ctx, (size_t)B * P * vec * sizeof(double2)));
        // static step tables in ONE upload: [hs] doubles, then [rows | save] ints
        const size_t n_int = (size_t)nsteps * (3 + (step_save ? 1 : 0));
        std::vector<double> pack((size_t)nsteps + (n_int + 1) / 2);
        int* const h_rows = reinterpret_cast<int*>(pack.data() + nsteps);
        std::copy(step_h, step_h + nsteps, pack.data());
        std::copy(step_rows, step_rows + 3 * (size_t)nsteps, h_rows);
        if (step_save) std::copy(step_save, step_save + nsteps, h_rows + 3 * (size_t)nsteps);
        CHK(p->d_static.alloc(ctx, pack.size() * sizeof(double)));
        HIPCHK(ctx, hipMemcpyAsync(p->d_static.p, pack.data(), pack.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        p->dev_hs = p->d_static.as<double>();
        p->dev_rows = reinterpret_cast<const int*>(p->d_static.as<double>() + nsteps);
        p->dev_save = step_save ? p->dev_rows + 3 * (size_t)nsteps : nullptr;
        HIPCHK(ctx, hipMemcpyAsync(p->d_y0.p, y0, y0_elems * sizeof(double2), hipMemcpyHostToDevice, ctx->stream));
        CHK(p->d_nrm.alloc(ctx, nrm.size() * sizeof(double)));
        HIPCHK(ctx, hipMemcpyAsync(p->d_nrm.p, nrm.data(), nrm.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        CHK(p->d_bounds.alloc(ctx, (size_t)3 * nsteps * sizeof(double)));
        // per-run series tables: [coef (EXPM_PLAN_STRIDE per step) | par] doubles, then [K | reps] ints
        CHK(p->d_dyn.alloc(ctx, ((size_t)nsteps * (EXPM_PLAN_STRIDE + 1) + (size_t)nsteps) * sizeof(double)));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));       // (pack / nrm are stack temporaries)
        CHK(make_phase_rows(s, times, R, p->d_times, p->d_E));
        if (magnus_order == 2) {
            if (s->has_frame) {
                CHK(p->d_dt.alloc(ctx, (size_t)nsteps * np * sizeof(double2)));
                const size_t cells = (size_t)nsteps * np;
                hipLaunchKernelGGL(sweep_dtable_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, ctx->stream,
                                   p->d_E.as<double2>(), p->dev_rows, nsteps, np, p->d_dt.as<double2>());
                HIPCHK(ctx, hipGetLastError());
            }
            CHK(p->d_stash.alloc(ctx, (size_t)B * 2 * np * sizeof(double2)));
        }
        // exchange slots + flag words of the two-workgroup kernels (and the larger ring of the four-way split kernel on request)
        const size_t duo_bytes = (size_t)B * 3 * np * sizeof(double2) + (size_t)B * 2 * DUO_FLAG_WORDS * sizeof(int);
        const size_t split_bytes = ctx->ell_sweep_split ? (size_t)B * 4 * magnus_order * 2 * np * sizeof(unsigned long long) : 0;
        CHK(p->d_ring.alloc(ctx, std::max(duo_bytes, split_bytes)));
        if (s->sp_flip) CHK(p->d_cab.alloc(ctx, (size_t)B * nsteps * s->sp_w * sizeof(double2)));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    guard.p = nullptr;
    *out = p;
    return 0;
}

// one launch of ell_sweep_kernel (one workgroup per instance): the route of large shards, and the re-run after a give-up
static int expm_plan_launch_single(midyn_expm_plan* p, const SweepArgs& a, int packed, int packed1, size_t lds) {
    midyn_stack* s = p->stack;
    midyn_ctx* ctx = s->ctx;
    const int threads = s->n_pad < SWEEP_THREADS ? s->n_pad : SWEEP_THREADS;   // 256 / 512 rows: one row per thread
    const int rpt = s->n_pad / threads;
    using SweepFn = void (*)(const SweepArgs);
#define MIDYN_SWEEP_ROW(O_, P_)                                                                                        \
    {ell_sweep_kernel<O_, 1, 1024, P_>, ell_sweep_kernel<O_, 2, 1024, P_>, nullptr,          \
     ell_sweep_kernel<O_, 4, 1024, P_>, ell_sweep_kernel<O_, 1, 256, P_>, ell_sweep_kernel<O_, 1, 512, P_>}
    static const SweepFn table[2][4][SWEEP_MAX_RPT + 2] = {
        {MIDYN_SWEEP_ROW(1, 0), MIDYN_SWEEP_ROW(1, 1), MIDYN_SWEEP_ROW(1, 2), MIDYN_SWEEP_ROW(1, 3)},
        {MIDYN_SWEEP_ROW(2, 0), MIDYN_SWEEP_ROW(2, 1), MIDYN_SWEEP_ROW(2, 2), MIDYN_SWEEP_ROW(2, 3)}};
#undef MIDYN_SWEEP_ROW
    const int which = threads == 256 ? SWEEP_MAX_RPT : (threads == 512 ? SWEEP_MAX_RPT + 1 : rpt - 1);
    const SweepFn fn = table[p->order - 1][packed1][which];
    static DeviceOnce sweep_attr[2][4][SWEEP_MAX_RPT + 2];
    if (sweep_attr[p->order - 1][packed1][which].needed(ctx->device)) {
        HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
        sweep_attr[p->order - 1][packed1][which].done(ctx->device);
    }
    (void)packed;
    ctx->last_sweep[2] = 1;
    ctx->last_sweep[3] = packed1;
    note_variant("ell_sweep_kernel", {p->order, rpt, threads, packed1});
    SweepArgs a1 = a;
    if (packed1 == 3) a1.pk = s->sp_flip_xs;       // (per slot, not per element)
    // (form 3 keeps its per-slot tables behind the vectors in the dynamic LDS: the vectors start at LDS address 0)
    const size_t lds1 = lds + (packed1 == 3 ? SWEEP_MAX_SLOTS * (sizeof(double2) + sizeof(int)) : 0);
    {
        ProfScope ps(ctx, KC_RESIDENT);
        hipLaunchKernelGGL(fn, dim3(p->B), dim3(threads), lds1, ctx->stream, a1);
    }
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

// The arguments every sweep kernel shares, from the plan's device tables; `force_single`: straight to the one-workgroup kernel.
static int expm_plan_launch(midyn_expm_plan* p, bool force_single) {
    midyn_stack* s = p->stack;
    midyn_ctx* ctx = s->ctx;
    const int B = p->B, nsteps = p->nsteps, magnus_order = p->order;
    const double* const d_coef = p->d_dyn.as<double>();
    const double* const d_par = d_coef + (size_t)nsteps * EXPM_PLAN_STRIDE;
    const int* const d_K = reinterpret_cast<const int*>(d_par + nsteps);
    const int* const d_rep = d_K + nsteps;
    SweepArgs a{};
    a.val = s->sp_val;
    a.col = s->sp_col;
    a.tags = s->sp_tags;
    a.wsp = s->sp_w;
    a.wre = s->sp_wre;
    a.wre_loc = s->sp_wre_loc;
    a.wim_loc = s->sp_wim_loc;
    a.n = s->n;
    a.n_pad = s->n_pad;
    a.has_static = s->has_static;
    a.k = s->k;
    a.nseg = s->nseg;
    a.S = s->k > 0 ? p->d_S.as<double>() : nullptr;
    a.inst_stride = (long long)p->R * s->k;
    a.E = s->has_frame ? p->d_E.as<double2>() : nullptr;
    a.rows = p->dev_rows;
    a.hs = p->dev_hs;
    a.save = p->dev_save;
    a.nsteps = nsteps;
    a.ser_K = d_K;
    a.ser_reps = d_rep;
    a.ser_par = d_par;
    a.coef = d_coef;
    a.stride = EXPM_PLAN_STRIDE;
    a.y0 = p->d_y0.as<double2>();
    a.y0_shared = p->y0_shared ? 1 : 0;
    a.out = p->out_target;
    a.P = p->P;
    if (magnus_order == 2) {
        a.Dt = a.E ? p->d_dt.as<double2>() : nullptr;
        a.stash = p->d_stash.as<double2>();
    }
    // packed element forms (stack_ell_layout): 1 = column | sign, 2 = LDS address of the operand (one sign per slot)
    const int packed = ctx->ell_sweep_packed ? s->sp_packed : 0;
    a.pk = packed ? s->sp_pk : nullptr;
    a.mag = packed ? s->sp_mag : nullptr;
    const size_t lds_old = (size_t)magnus_order * s->n_pad * sizeof(double2);           // split kernel (below)
    // ... 3 = no elements at all: one signed magnitude and one flip mask per slot (one workgroup per instance:
    // ell_sweep_kernel<.., 3>; two: ell_flip_duo_kernel)
    const int packed1 = (packed == 2 && s->sp_flip && s->sp_w <= 64 && ctx->ell_sweep_flip) ? 3 : packed;
    const size_t lds = packed == 2 ? (size_t)((s->n_pad + 2047) / 2048) * 65536
                                   : (size_t)magnus_order * (s->n_pad + 1) * sizeof(double2);
    if (lds > 150 * 1024 || lds_old > 150 * 1024)
        return fail(ctx, "midyn_expm_solve: the sweep kernel's staged vectors do not fit its 150 KB of LDS");
    {
        double terms = 0.0;
        for (int st = 0; st < nsteps; ++st) terms += (double)p->repv[st] * std::abs(p->Kv[st]);
        ctx->last_sweep[0] = terms;
        ctx->last_sweep[1] = s->sp_w;
        ctx->last_sweep[3] = packed;
    }
    p->two_workgroups = false;
    if (force_single) {
        CHK(expm_plan_launch_single(p, a, packed, packed1, lds));
        p->in_flight = true;
        return 0;
    }
    // small shards: 4 or 2 workgroups per instance when that still fits one workgroup per CU
    int nsplit = 1;
    // (measured on cfg 5, ms per step, one / four workgroups per instance: 1 instance 0.29 / 0.18, 8: 0.32 / 0.20,
    // 32: 0.33 / 0.24; two workgroups per instance at 128 instances: 0.41 against 0.36 -- only on request)
    // (the packed forms of the one-workgroup kernel are faster than the split kernel at every shard size: 18-20 us per
    // term against 18 / 20 / 26 us at 16 / 32 / 64 instances x 4 workgroups, tools/sweep2_probe.hip)
    if (ctx->ell_sweep_split && (!packed || ctx->ell_sweep_split >= 3))
        for (int cand : {4, 2})
            if (nsplit == 1 && (cand == 4 || ctx->ell_sweep_split >= 2) && s->n_pad % (SWEEP_THREADS * cand) == 0 &&
                s->n_pad / (SWEEP_THREADS * cand) <= 2 && (long long)B * cand <= ctx->num_cu)
                nsplit = cand;
    ctx->last_sweep[2] = nsplit;
    if (nsplit > 1) ctx->last_sweep[3] = 0;
    bool launched = false;
    // Small shards of a stack with a packed element form (cfg 5: 128 instances per GPU of an 8-GPU run would leave
    // half of the CUs idle): TWO workgroups per instance, the partner's half of every operand vector arriving while
    // the slots that stay inside the own half are being applied (ell_sweep_duo_kernel).
    const int np_ = s->n_pad;
    const bool duo_shape = nsplit == 1 && ctx->ell_sweep_duo && packed && (np_ & (np_ - 1)) == 0 && np_ >= 512 &&
                           np_ <= 2 * SWEEP_THREADS * 2 && 2ll * B <= ctx->num_cu;
    const size_t ring_bytes = (size_t)B * 3 * np_ * sizeof(double2), flag_bytes = (size_t)B * 2 * DUO_FLAG_WORDS * sizeof(int);
    // ... and when every slot of the stack also has ONE flip mask (column = row ^ flip: sums of Pauli strings without Z
    // factors -- cfg 5): the kernel that reads no operator elements at all (ell_flip_duo_kernel, midyn_flip.h)
    if (duo_shape && packed == 2 && s->sp_flip && s->sp_w <= 64 && ctx->ell_sweep_flip && p->d_cab.p) {
        const int half = np_ / 2;
        // (measured and dropped in the last session of round 5: halves of 2048 rows as 512 threads x 4 rows -- two waves per
        // SIMD with 218 registers, bit-identical results -- 12.5 against 11.0 us per term, 11.6 against 10.8 with the two LDS
        // buffers: the slot loops need the four waves per SIMD to cover the LDS latency; profiles/r05_cfg5_duo.md)
        const int th = half < SWEEP_THREADS ? half : SWEEP_THREADS;
        const int rpt_d = half / th;
        using FlipFn = void (*)(const FlipDuoArgs);
#define MIDYN_FLIP_ROW(O_) {ell_flip_duo_kernel<O_, 1, 256>, ell_flip_duo_kernel<O_, 1, 512>, ell_flip_duo_kernel<O_, 1, 1024>, ell_flip_duo_kernel<O_, 2, 1024>}
        static const FlipFn ftable[2][4] = {MIDYN_FLIP_ROW(1), MIDYN_FLIP_ROW(2)};
#undef MIDYN_FLIP_ROW
        const int shape = th == 256 ? 0 : (th == 512 ? 1 : (rpt_d == 1 ? 2 : 3));
        const FlipFn ffn = ftable[magnus_order - 1][shape];
        note_variant("ell_flip_duo_kernel", {magnus_order, rpt_d, th});
        const size_t flds = magnus_order == 2 ? 2 * 65536 : 2 * 32768;     // two operand buffers (FLIP_BUF apart, midyn_flip.h)
        static DeviceOnce fattr[2][4];
        if (fattr[magnus_order - 1][shape].needed(ctx->device)) {
            HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(ffn), hipFuncAttributeMaxDynamicSharedMemorySize, 2 * 65536));
            fattr[magnus_order - 1][shape].done(ctx->device);
        }
        // the slot coefficients of every (instance, step), once per run, for the scalar loads of the kernel
        const size_t cab_cells = (size_t)B * nsteps * s->sp_w;
        hipLaunchKernelGGL(flip_cab_kernel, dim3((unsigned)((cab_cells + 255) / 256)), dim3(256), 0, ctx->stream, a.S, a.inst_stride,
                           s->k, s->has_static, a.rows, nsteps, s->sp_flip_tags, s->sp_flip_mag, s->sp_w, magnus_order, B,
                           p->d_cab.as<double2>());
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemsetAsync(static_cast<char*>(p->d_ring.p) + ring_bytes, 0, flag_bytes, ctx->stream));
        FlipDuoArgs fa{};
        fa.n = s->n;
        fa.n_pad = np_;
        fa.nsteps = nsteps;
        fa.wsp = s->sp_w;
        fa.n_loc = s->sp_wre_loc + (s->sp_wim_loc - s->sp_wre);
        fa.n_re_loc = s->sp_wre_loc;
        fa.meta = s->sp_flip_meta;
        fa.cab = reinterpret_cast<const flip_d2*>(p->d_cab.p);
        fa.E = a.E;
        fa.Dt = a.Dt;
        fa.rows = a.rows;
        fa.hs = a.hs;
        fa.save = a.save;
        fa.ser_K = a.ser_K;
        fa.ser_reps = a.ser_reps;
        fa.ser_par = a.ser_par;
        fa.coef = a.coef;
        fa.stride = a.stride;
        fa.y0 = a.y0;
        fa.y0_shared = a.y0_shared;
        fa.out = a.out;
        fa.P = a.P;
        fa.ring = p->d_ring.as<double2>();
        fa.flags = reinterpret_cast<int*>(static_cast<char*>(p->d_ring.p) + ring_bytes);
        fa.err = ctx->d_sync_err;
        fa.spin_limit = ctx->resident_spin_limit;
        fa.protocol = ctx->exchange_protocol;
        fa.part_major = (B % 8 == 0) ? 1 : 0;
        fa.ablate = ctx->ablate;
        void* params[1] = {&fa};
        ProfScope ps(ctx, KC_RESIDENT);
        const hipError_t le = hipLaunchCooperativeKernel(reinterpret_cast<const void*>(ffn), dim3(2 * B), dim3(th), params,
                                                         (unsigned)flds, ctx->stream);
        if (le == hipSuccess) {
            launched = true;
            ctx->last_sweep[2] = 2;
            ctx->last_sweep[3] = 3;     // element form 3: none (flip masks)
            ctx->last_sweep[4] = s->sp_w - fa.n_loc;
        } else {
            (void)hipGetLastError();    // refused: the kernels below
        }
    }
    if (!launched && duo_shape) {
        // (measured and dropped: 2048 rows per workgroup as 512 threads x 4 rows with 256 registers each -- 16.9 against 17.2 us
        // per term in the same build, profiles/r05_cfg5_duo.md)
        const int half = np_ / 2;
        const int th = half < SWEEP_THREADS ? half : SWEEP_THREADS;
        const int rpt_d = half / th;
        using DuoFn = void (*)(const SweepDuoArgs);
#define MIDYN_DUO_ROW(O_, P_)                                                                                                        \
    {ell_sweep_duo_kernel<O_, 1, 256, P_>, ell_sweep_duo_kernel<O_, 1, 512, P_>, ell_sweep_duo_kernel<O_, 1, 1024, P_>,                \
     ell_sweep_duo_kernel<O_, 2, 1024, P_>}
        static const DuoFn dtable[2][2][4] = {{MIDYN_DUO_ROW(1, 1), MIDYN_DUO_ROW(1, 2)}, {MIDYN_DUO_ROW(2, 1), MIDYN_DUO_ROW(2, 2)}};
#undef MIDYN_DUO_ROW
        const int shape = th == 256 ? 0 : (th == 512 ? 1 : (rpt_d == 1 ? 2 : 3));
        const DuoFn dfn = dtable[magnus_order - 1][packed - 1][shape];
        note_variant("ell_sweep_duo_kernel", {magnus_order, rpt_d, th, packed});
        static DeviceOnce dattr[2][2][4];
        if (dattr[magnus_order - 1][packed - 1][shape].needed(ctx->device)) {
            HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(dfn), hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024));
            dattr[magnus_order - 1][packed - 1][shape].done(ctx->device);
        }
        // payload slots (three half-written vectors per instance) and the flag words of every (instance, half)
        HIPCHK(ctx, hipMemsetAsync(static_cast<char*>(p->d_ring.p) + ring_bytes, 0, flag_bytes, ctx->stream));
        SweepDuoArgs da{};
        da.a = a;
        da.a.stash = nullptr;               // (half the rows per thread: the series vectors stay in registers)
        da.ring = p->d_ring.as<double2>();
        da.flags = reinterpret_cast<int*>(static_cast<char*>(p->d_ring.p) + ring_bytes);
        da.ablate = ctx->ablate;
        da.err = ctx->d_sync_err;
        da.spin_limit = ctx->resident_spin_limit;
        da.protocol = ctx->exchange_protocol;
        da.part_major = (B % 8 == 0) ? 1 : 0;   // partners on one XCD under the observed round-robin dispatch
        void* params[1] = {&da};
        ProfScope ps(ctx, KC_RESIDENT);
        const hipError_t le = hipLaunchCooperativeKernel(reinterpret_cast<const void*>(dfn), dim3(2 * B), dim3(th), params,
                                                         (unsigned)lds, ctx->stream);
        if (le == hipSuccess) {
            launched = true;
            ctx->last_sweep[2] = 2;
            ctx->last_sweep[3] = packed;
            ctx->last_sweep[4] = s->sp_w - (s->sp_wre_loc + (s->sp_wim_loc - s->sp_wre));   // slots that cross the halves
        } else {
            (void)hipGetLastError();    // refused: one workgroup per instance below
        }
    }
    if (nsplit > 1 && !launched) {
        const int rpt_s = s->n_pad / (SWEEP_THREADS * nsplit);
        using SplitFn = void (*)(const SweepSplitArgs);
        static const SplitFn stable[2][2] = {{ell_sweep_split_kernel<1, 1>, ell_sweep_split_kernel<1, 2>},
                                             {ell_sweep_split_kernel<2, 1>, ell_sweep_split_kernel<2, 2>}};
        const SplitFn sfn = stable[magnus_order - 1][rpt_s - 1];
        note_variant("ell_sweep_split_kernel", {magnus_order, rpt_s});
        static DeviceOnce sattr[2][2];
        if (sattr[magnus_order - 1][rpt_s - 1].needed(ctx->device)) {
            HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(sfn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                            140 * 1024));
            sattr[magnus_order - 1][rpt_s - 1].done(ctx->device);
        }
        const size_t split_bytes = (size_t)B * 4 * magnus_order * 2 * s->n_pad * sizeof(unsigned long long);
        if (p->d_ring.bytes < split_bytes) CHK(p->d_ring.alloc(ctx, split_bytes));    // (option switched on after the plan was made)
        HIPCHK(ctx, hipMemsetAsync(p->d_ring.p, 0xFF, split_bytes, ctx->stream));
        SweepSplitArgs sa{};
        sa.a = a;
        sa.nsplit = nsplit;
        sa.ring = p->d_ring.as<unsigned long long>();
        sa.err = ctx->d_sync_err;
        sa.spin_limit = ctx->resident_spin_limit;
        void* params[1] = {&sa};
        ProfScope ps(ctx, KC_RESIDENT);
        sa.part_major = (B % 8 == 0) ? 1 : 0;   // partners on one XCD under the observed round-robin dispatch
        const hipError_t le = hipLaunchCooperativeKernel(reinterpret_cast<const void*>(sfn), dim3(B * nsplit),
                                                         dim3(SWEEP_THREADS), params, (unsigned)lds_old, ctx->stream);
        if (le == hipSuccess) launched = true;
        else (void)hipGetLastError();   // refused: one workgroup per instance below
    }
    if (launched) {
        HIPCHK(ctx, hipGetLastError());
        p->two_workgroups = true;
    } else {
        CHK(expm_plan_launch_single(p, a, packed, packed1, lds));
    }
    p->in_flight = true;
    return 0;
}

// Is `ptr` host memory the device can write (hipHostMalloc / registered)?  Then *dev = its device address.
static bool expm_plan_mapped_host(const void* ptr, size_t bytes, void** dev) {
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, ptr) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    if (at.type != hipMemoryTypeHost || !at.devicePointer) return false;
    // (the end of the block must be mapped too)
    hipPointerAttribute_t at2{};
    if (hipPointerGetAttributes(&at2, static_cast<const char*>(ptr) + bytes - 1) != hipSuccess || at2.type != hipMemoryTypeHost) {
        (void)hipGetLastError();
        return false;
    }
    *dev = at.devicePointer;
    return true;
}

// ---- host blocks of the library (midyn_host_alloc / midyn_host_free, midyn.h): page-locked, device-writable memory for results.
// A block that came from here is recognised by its address alone -- no hipPointerGetAttributes (30-40 us per query, two per
// block) -- and cannot go stale: midyn_host_free removes it before the memory goes back to the runtime.
struct HostBlocks {
    std::mutex mu;
    std::map<const char*, std::pair<size_t, char*>> blocks;     // base -> (bytes, device address of the base)
};
static HostBlocks& host_blocks() {
    static HostBlocks* hb = new HostBlocks();      // (never destroyed: finalizers of the binding may run during process exit)
    return *hb;
}
static bool host_block_lookup(const void* ptr, size_t bytes, void** dev) {
    HostBlocks& hb = host_blocks();
    std::lock_guard<std::mutex> lock(hb.mu);
    const char* q = static_cast<const char*>(ptr);
    auto it = hb.blocks.upper_bound(q);
    if (it == hb.blocks.begin()) return false;
    --it;
    if (q < it->first || q + bytes > it->first + it->second.first) return false;
    *dev = it->second.second + (q - it->first);
    return true;
}

extern "C" int midyn_host_alloc(size_t bytes, void** out) {
    if (!out || bytes == 0) return fail(nullptr, "midyn_host_alloc: bad argument");
    void* h = nullptr;
    if (hipHostMalloc(&h, bytes, hipHostMallocPortable | hipHostMallocMapped) != hipSuccess || !h) {     // (every device of the process may write it)
        (void)hipGetLastError();
        return fail(nullptr, "midyn_host_alloc: hipHostMalloc failed");
    }
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess || !d) {
        (void)hipGetLastError();
        hipHostFree(h);
        return fail(nullptr, "midyn_host_alloc: the block has no device address");
    }
    HostBlocks& hb = host_blocks();
    {
        std::lock_guard<std::mutex> lock(hb.mu);
        hb.blocks[static_cast<const char*>(h)] = {bytes, static_cast<char*>(d)};
    }
    *out = h;
    return 0;
}

extern "C" int midyn_host_free(void* ptr) {
    if (!ptr) return 0;
    HostBlocks& hb = host_blocks();
    {
        std::lock_guard<std::mutex> lock(hb.mu);
        auto it = hb.blocks.find(static_cast<const char*>(ptr));
        if (it == hb.blocks.end()) return fail(nullptr, "midyn_host_free: not a block of midyn_host_alloc");
        hb.blocks.erase(it);
    }
    return hipHostFree(ptr) == hipSuccess ? 0 : fail(nullptr, "midyn_host_free: hipHostFree failed");
}

static bool expm_plan_block(midyn_expm_plan* p, const void* ptr, size_t bytes, void** dev) {
    if (host_block_lookup(ptr, bytes, dev)) return true;
    for (const auto& blk : p->mapped)
        if (blk.host == ptr && blk.bytes >= bytes) {
            *dev = blk.dev;
            return true;
        }
    if (!expm_plan_mapped_host(ptr, bytes, dev)) return false;
    if (p->mapped.size() >= 16) p->mapped.erase(p->mapped.begin());
    p->mapped.push_back({ptr, bytes, *dev});
    return true;
}

// MIDYN_TIMING=1: wall-clock marks of a call on stderr, from its entry (where a solve's host time goes; diagnostics only)
struct TimingMarks {
    const char* fn;
    std::chrono::steady_clock::time_point t_entry = std::chrono::steady_clock::now();
    void operator()(const char* what) const {
        static const bool timing = std::getenv("MIDYN_TIMING") != nullptr;
        if (timing)
            std::fprintf(stderr, "[midyn timing] %s %-28s %8.1f us\n", fn, what,
                         std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_entry).count());
    }
};

static int expm_plan_run_impl(midyn_expm_plan* p, const double* S, midyn_complex* Y_direct) {
    midyn_stack* s = p->stack;
    midyn_ctx* ctx = s->ctx;
    const TimingMarks mark{"expm_plan_run"};
    if (s->k > 0 && !S) return fail(ctx, "midyn_expm_plan_run: NULL coefficient table");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int B = p->B, nsteps = p->nsteps, magnus_order = p->order;
    if (!p->sweep) {
        p->host_result.resize((size_t)B * p->P * s->n * p->m);
        CHK(midyn_expm_solve(s, B, p->m, p->R, p->times.data(), S, nsteps, p->rows.data(), p->hs.data(),
                             p->has_save ? p->save.data() : nullptr, p->P, magnus_order, p->y0.data(), p->y0_shared ? 1 : 0,
                             p->host_result.data()));
        p->have_run = true;
        return 0;
    }
    if (p->in_flight) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        (void)take_wait_error(ctx);
        p->in_flight = false;
    }
    // S may live on the host or on the device (midyn_sigtable_data): hipMemcpyDefault resolves it; ordered on the stream
    if (s->k > 0) HIPCHK(ctx, hipMemcpyAsync(p->d_S.p, S, (size_t)B * p->R * s->k * sizeof(double), hipMemcpyDefault, ctx->stream));
    // norm bounds of Omega over the instances for every step (triangle inequality over the segments): the 1-norm bound the
    // Taylor degree is chosen from, and for the Chebyshev series the larger of the 1- and infinity-norm bounds (rho) and the
    // bound of the Hermitian part -- ONE kernel over the device copy of the coefficient table (step_bounds_kernel)
    hipLaunchKernelGGL(step_bounds_kernel, dim3(nsteps), dim3(256), 0, ctx->stream, s->k > 0 ? p->d_S.as<double>() : nullptr, B, p->R,
                       s->k, s->nseg, s->has_static, p->dev_rows, p->dev_hs, magnus_order, p->d_nrm.as<double>(),
                       p->d_bounds.as<double>());
    HIPCHK(ctx, hipGetLastError());
    const size_t n_dyn_dbl = (size_t)nsteps * (EXPM_PLAN_STRIDE + 1) + (size_t)nsteps;    // [coef | par] + [K | reps] as doubles
    const bool pinned_ok = 3 * (size_t)nsteps + n_dyn_dbl <= midyn_ctx::PINNED_DOUBLES;
    std::vector<double> pageable;
    if (!pinned_ok) pageable.resize(3 * (size_t)nsteps + n_dyn_dbl);
    double* const h_bounds = pinned_ok ? ctx->h_pinned : pageable.data();
    double* const h_dyn = h_bounds + 3 * (size_t)nsteps;
    HIPCHK(ctx, hipMemcpyAsync(h_bounds, p->d_bounds.p, (size_t)3 * nsteps * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    mark("table up, norm bounds back");
    // per step a series -- Chebyshev or scaled Taylor, degree, scaling, coefficients -- from the same norm bounds over the
    // instances as the per-launch route of expm_action_solve (which asks for a Chebyshev series a fifth shorter than the Taylor
    // series before it takes it; here one term fewer is enough)
    double* const h_coef = h_dyn;
    double* const h_par = h_coef + (size_t)nsteps * EXPM_PLAN_STRIDE;
    int* const h_K = reinterpret_cast<int*>(h_par + nsteps);
    int* const h_rep = h_K + nsteps;
    p->Kv.assign(nsteps, 0);
    p->repv.assign(nsteps, 1);
    p->parv.assign(nsteps, 1.0);
    StepSeries ser;
    for (int st = 0; st < nsteps; ++st) {
        const double* const nb = h_bounds + 3 * st;     // 1-norm bound, rho, Hermitian part
        // (cfg 5, rho ~ 0.1 per step: 7-8 Chebyshev terms against Taylor degree 9 -- 150 instead of 180 terms per instance)
        CHK(step_series(ctx, magnus_order, nb[0], nb[1], nb[2], nb[0], true, true, &ser));
        double* const row = h_coef + (size_t)st * EXPM_PLAN_STRIDE;
        std::fill(row, row + EXPM_PLAN_STRIDE, 0.0);
        // a negative K = Taylor of degree -K; par = rho (Chebyshev) or sc (Taylor)
        const bool cheb = ser.cheb && ser.K + 1 <= EXPM_PLAN_STRIDE;
        p->Kv[st] = cheb ? ser.K : -ser.deg;
        p->repv[st] = cheb ? ser.reps : ser.sc;
        p->parv[st] = cheb ? ser.rho : (double)ser.sc;
        if (cheb) std::copy(ser.coef.begin(), ser.coef.end(), row);
        h_K[st] = p->Kv[st];
        h_rep[st] = p->repv[st];
        h_par[st] = p->parv[st];
    }
    HIPCHK(ctx, hipMemcpyAsync(p->d_dyn.p, h_dyn, n_dyn_dbl * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (!pinned_ok) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    mark("series tables queued");
    // the saved states go straight into the caller's block when the device can write it (pinned host memory: the binding's result
    // arrays): the stores of a step's result leave while the next step runs, and no copy follows the launch
    p->out_target = p->d_out.as<double2>();
    if (Y_direct && ctx->expm_direct_out) {
        void* dev = nullptr;
        if (expm_plan_block(p, Y_direct, (size_t)B * p->P * s->n * sizeof(double2), &dev)) p->out_target = static_cast<double2*>(dev);
    }
    CHK(expm_plan_launch(p, false));
    p->have_run = true;
    mark("launched");
    return 0;
}

static int expm_plan_fetch_impl(midyn_expm_plan* p, midyn_complex* Y_out) {
    midyn_stack* s = p->stack;
    midyn_ctx* ctx = s->ctx;
    if (!p->have_run) return fail(ctx, "midyn_expm_plan_fetch: the plan has not run");
    if (!Y_out) return fail(ctx, "midyn_expm_plan_fetch: NULL argument");
    const size_t vec = (size_t)s->n * p->m;
    const int B = p->B, P = p->P;
    if (!p->sweep) {
        memcpy(Y_out, p->host_result.data(), p->host_result.size() * sizeof(midyn_complex));
        return 0;
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // Slot 0 of every instance is y0 itself (midyn.h): written here, on the host, while the kernel runs -- and only the slots the
    // kernel produces come back over PCIe (cfg 5 shard: 8.4 of 16.8 MB)
    for (int b = 0; b < B; ++b)
        memcpy(Y_out + (size_t)b * P * vec, p->y0.data() + (p->y0_shared ? 0 : (size_t)b * vec), vec * sizeof(double2));
    if (p->in_flight) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        p->in_flight = false;
        // the partners of an instance wait for each other: a wait that gave up -> one workgroup per instance
        if (p->two_workgroups && take_wait_error(ctx)) {
            ++ctx->resident_fallbacks;
            CHK(expm_plan_launch(p, true));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            p->in_flight = false;
        }
    }
    const bool direct = p->out_target != p->d_out.as<double2>();
    if (direct) {
        void* dev = nullptr;
        const bool same = expm_plan_block(p, Y_out, (size_t)B * P * vec * sizeof(double2), &dev) && dev == (void*)p->out_target;
        if (same) return 0;             // (already there: the kernel wrote this block)
        // another destination than the run's block: copy from the block the kernel wrote
        for (int b = 0; b < B && P > 1; ++b)
            HIPCHK(ctx, hipMemcpy(Y_out + ((size_t)b * P + 1) * vec, p->out_target + ((size_t)b * P + 1) * vec,
                                  (size_t)(P - 1) * vec * sizeof(double2), hipMemcpyDefault));
        return 0;
    }
    if (P > 1)
        HIPCHK(ctx, hipMemcpy2D(Y_out + vec, (size_t)P * vec * sizeof(double2), p->d_out.as<double2>() + vec,
                                (size_t)P * vec * sizeof(double2), (size_t)(P - 1) * vec * sizeof(double2), B, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int midyn_expm_plan_create(midyn_stack* s, int B, int m, int R, const double* times, int nsteps, const int* step_rows,
                                      const double* step_h, const int* step_save, int P, int magnus_order, const midyn_complex* y0,
                                      int y0_shared, midyn_expm_plan** out) {
    if (!s || !out) return fail(s ? s->ctx : nullptr, "midyn_expm_plan_create: NULL argument");
    *out = nullptr;
    return expm_plan_create_impl(s, B, m, R, times, nsteps, step_rows, step_h, step_save, P, magnus_order, y0, y0_shared, out);
}

extern "C" int midyn_expm_plan_run(midyn_expm_plan* p, const double* S, midyn_complex* Y_direct) {
    if (!p) return fail(nullptr, "midyn_expm_plan_run: NULL plan");
    return expm_plan_run_impl(p, S, Y_direct);
}

extern "C" int midyn_expm_plan_fetch(midyn_expm_plan* p, midyn_complex* Y_out) {
    if (!p) return fail(nullptr, "midyn_expm_plan_fetch: NULL plan");
    return expm_plan_fetch_impl(p, Y_out);
}
