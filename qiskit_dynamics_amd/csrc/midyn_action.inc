// midyn_action.inc -- part of midyn.hip (one translation unit; included in order): expm ACTION (Chebyshev / Taylor / Arnoldi, Magnus 1-2) and the midyn_expm_solve dispatch
// -------------------------------------------------------------------------------------------------
// expm ACTION: y <- expm(Omega_m) y without forming the exponential (a10/a11 for states with few
// columns).  The reference computes scipy.linalg.expm(Omega) (n^3 work, ~(7+s) zgemm) and multiplies
// it into y even when y is a single vector; the result only needs  expm(Omega) y = sum_j Omega^j y / j!,
// i.e. products Omega.v, which for
//     order 1:  Omega v = h G(t1) v
//     order 2:  Omega v = h/2 (g1 v + g2 v) + sqrt(3)/12 h^2 (g2 (g1 v) - g1 (g2 v))     (commutator free)
// are exactly the batched RHS contraction of row a2/a7 (all instances of a sweep in ONE MFMA GEMM over
// the operator stack, per-instance coefficients; the streaming kernel for one column).  Scaling:
// y <- (T_p(Omega / s))^s y with (p, s) of least p*s such that bound/s <= theta_p, where
// bound >= ||Omega||_1 follows from the per-segment norms: ||G(t)||_1 <= sum_seg |c_seg| ||A_seg||_1
// (the frame phases have modulus 1).  One instance: G(t_i) is formed once per step (gen_eval) and the
// products run on that single matrix.
// -------------------------------------------------------------------------------------------------
// (series helpers -- ActionScheme, action_choose, the per-segment norms, bessel_j, StepSeries / step_series -- live in
// midyn_sweep_plan.inc, included before this file)
//
// expm_action_solve tries the routes in this order, each a function of its own: the cached sweep plan
// (expm_route_sweep_plan), the small-system kernel (expm_route_tiny), the one-launch sweep of a small dense system
// (expm_route_combine_sweep), one trajectory on a very sparse stack (expm_route_resident), and the per-launch route
// (expm_route_per_launch) for whatever the others decline.  Every route takes each step's series from step_series.

// Arnoldi pays ~6 launches per vector (product, two Gram-Schmidt passes, normalisation) and needs about 1.5 x the
// spectral radius + 20 vectors: its cost in Taylor terms for a step of this norm bound
static long long arnoldi_products(double bound) { return (long long)(6.0 * (1.5 * bound + 20.0)); }

// the saved states of every instance to the caller, once the stream has drained
static int plan_fetch_out(midyn_rk4_plan* p, midyn_complex* Y_out) {
    midyn_ctx* ctx = p->stack->ctx;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(Y_out, p->d_out.p, (size_t)p->B * p->P * p->stack->n * p->m * sizeof(double2), hipMemcpyDeviceToHost));
    return 0;
}

// the Bessel coefficients of the Chebyshev steps for the one-launch kernels: a row of *stride (the longest series + 1) per step
static std::vector<double> cheb_table(const std::vector<StepSeries>& ser, int* stride) {
    int kmax = 0;
    for (const StepSeries& ss : ser)
        if (ss.cheb) kmax = std::max(kmax, ss.K);
    *stride = kmax + 1;
    std::vector<double> t(std::max(ser.size(), (size_t)1) * *stride, 0.0);
    for (size_t st = 0; st < ser.size(); ++st)
        if (ser[st].cheb) std::copy(ser[st].coef.begin(), ser[st].coef.end(), t.begin() + st * *stride);
    return t;
}

// ---- a sweep (or one Magnus-2 trajectory) on a very sparse stack: ONE launch of a sweep kernel, one or two workgroups
// per instance through all steps (csrc/midyn_resident.h, midyn_flip.h) -- the plan object of midyn_sweep_plan.inc, made, run
// once, fetched and destroyed here (the same code path as midyn_expm_plan_*; none of the buffers of the other routes is
// allocated for it)
static int expm_route_sweep_plan(midyn_stack* s, int B, int m, int R, const double* times, const double* S, int nsteps,
                                 const int* step_rows, const double* step_h, const int* step_save, int P, int magnus_order,
                                 const midyn_complex* y0, int y0_shared, midyn_complex* Y_out, const TimingMarks& mark) {
    midyn_ctx* ctx = s->ctx;
    // the plan of the previous one-shot solve, when this one has the same shapes, time grid, step tables and initial
    // states (a scan through Solver.solve / midyn_expm_solve instead of midyn_expm_plan_*: round 6 measured 0.26 ms of host
    // side around a 1.77 ms launch for the one-shot call against 0.04 ms for run + fetch of a kept plan -- most of the
    // difference is this plan's tables and buffers); kept in the stack until a solve that differs, an option change, or the
    // end of the stack
    midyn_expm_plan* ep = nullptr;
    const bool hit = ctx->expm_plan_cache && expm_plan_matches(s->sweep_plan, s, B, m, R, times, nsteps, step_rows, step_h,
                                                               step_save, P, magnus_order, y0, y0_shared);
    ctx->last_plan_cache = hit ? 1 : 0;
    if (hit) {
        ep = s->sweep_plan;
        ep->mapped.clear();     // (blocks vouched for at an earlier call: the caller of the one-shot entry point promised nothing)
    } else {
        stack_drop_sweep_plan(s);
        CHK(expm_plan_create_impl(s, B, m, R, times, nsteps, step_rows, step_h, step_save, P, magnus_order, y0, y0_shared, &ep));
    }
    const size_t y0_bytes = (size_t)(y0_shared ? 1 : B) * s->n * m * sizeof(midyn_complex);
    const bool keep = ctx->expm_plan_cache && y0_bytes <= EXPM_PLAN_CACHE_Y0_BYTES;
    struct PlanGuard {      // (a plan that is not kept, or a solve that failed: nothing stays behind)
        midyn_stack* s;
        midyn_expm_plan* p;
        bool keep, done;
        ~PlanGuard() {
            if (keep && done) {
                s->sweep_plan = p;
                s->sweep_plan_epoch = s->ctx->options_epoch;
            } else {
                if (s->sweep_plan == p) s->sweep_plan = nullptr;
                midyn_expm_plan_destroy(p);
            }
        }
    } plan_guard{s, ep, keep, false};
    mark(hit ? "plan found" : "plan made");
    CHK(expm_plan_run_impl(ep, S, Y_out));
    mark("launched");
    CHK(expm_plan_fetch_impl(ep, Y_out));
    mark("results on the host");
    plan_guard.done = true;
    return 0;
}

// Norm bounds of Omega over the instances for every step (triangle inequality over the segments), [nsteps][3]: the 1-norm
// bound the Taylor degree is chosen from, and for the Chebyshev series the larger of the 1- and infinity-norm bounds (rho) and
// the bound of the Hermitian part -- ONE kernel over the plan's device copy of the coefficient table (step_bounds_kernel).
static int expm_step_bounds(midyn_rk4_plan* p, int magnus_order, std::vector<double>* out) {
    midyn_stack* s = p->stack;
    midyn_ctx* ctx = s->ctx;
    const int nsteps = p->nsteps;
    if (nsteps <= 0) return 0;
    std::vector<double> nrm;
    CHK(stack_norm_table(s, &nrm));
    DevBuf d_nrm, d_rows, d_hs, d_out;
    CHK(d_nrm.alloc(ctx, nrm.size() * sizeof(double)));
    CHK(d_rows.alloc(ctx, (size_t)3 * nsteps * sizeof(int)));
    CHK(d_hs.alloc(ctx, (size_t)nsteps * sizeof(double)));
    CHK(d_out.alloc(ctx, (size_t)3 * nsteps * sizeof(double)));
    HIPCHK(ctx, hipMemcpyAsync(d_nrm.p, nrm.data(), nrm.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_rows.p, p->rows.data(), (size_t)3 * nsteps * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_hs.p, p->hs.data(), (size_t)nsteps * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(step_bounds_kernel, dim3(nsteps), dim3(256), 0, ctx->stream, s->k > 0 ? p->d_S.as<double>() : nullptr,
                       p->B, p->R, s->k, s->nseg, s->has_static, d_rows.as<int>(), d_hs.as<double>(), magnus_order,
                       d_nrm.as<double>(), d_out.as<double>());
    HIPCHK(ctx, hipGetLastError());
    out->resize((size_t)3 * nsteps);
    HIPCHK(ctx, hipMemcpyAsync(out->data(), d_out.p, out->size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// ---- a small system: the whole solve in one persistent launch (tiny_expm_kernel), the series of every step chosen here
// (a negative degree in its step table = a Chebyshev series with that many terms)
static int expm_route_tiny(midyn_rk4_plan* p, int magnus_order, const std::vector<double>& bounds, midyn_complex* Y_out) {
    midyn_ctx* ctx = p->stack->ctx;
    const int nsteps = p->nsteps;
    std::vector<int> deg(nsteps), scv(nsteps);
    std::vector<double> rhov(std::max(nsteps, 1), 1.0);
    std::vector<StepSeries> ser(nsteps);
    for (int st = 0; st < nsteps; ++st) {
        const double* nb = bounds.data() + 3 * st;
        CHK(step_series(ctx, magnus_order, nb[0], nb[1], nb[2], nb[0], true, false, &ser[st]));
        deg[st] = ser[st].cheb ? -ser[st].K : ser[st].deg;
        scv[st] = ser[st].cheb ? ser[st].reps : ser[st].sc;
        if (ser[st].cheb) rhov[st] = ser[st].rho;
    }
    int cheb_stride = 0;
    const std::vector<double> chebv = cheb_table(ser, &cheb_stride);
    DevBuf d_deg, d_sc, d_rho, d_cheb;
    CHK(d_deg.upload(ctx, deg));
    CHK(d_sc.upload(ctx, scv));
    CHK(d_rho.upload(ctx, rhov));
    CHK(d_cheb.upload(ctx, chebv));
    static DeviceOnce attr_set;
    if (attr_set.needed(ctx->device)) {
        HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(tiny_expm_kernel),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, 152 * 1024));
        attr_set.done(ctx->device);
    }
    TinyArgs a = tiny_args(p, 0, nsteps);
    {
        ProfScope ps(ctx, KC_STREAM);
        hipLaunchKernelGGL(tiny_expm_kernel, dim3((p->ncol + 3) / 4), dim3(256), p->tiny_smem, ctx->stream, a,
                           magnus_order, d_deg.as<int>(), d_sc.as<int>(), d_rho.as<double>(), d_cheb.as<double>(),
                           cheb_stride);
    }
    HIPCHK(ctx, hipGetLastError());
    return plan_fetch_out(p, Y_out);
}

// ---- a sweep of a small dense system, Magnus order 1: ONE launch of combine_sweep_kernel<.., MODE 1>, 16 instances per
// workgroup through all steps (csrc/midyn_combine_sweep.h).  The solve is handed over as a flat list of series terms: per
// step the same series as the per-launch route.  *done = false: declined (no COMBINE layout, a series or a save slot the
// list cannot encode, no kernel for the layout).
static int expm_route_combine_sweep(midyn_rk4_plan* p, const std::vector<double>& bounds, midyn_complex* Y_out, bool* done) {
    *done = false;
    midyn_ctx* ctx = p->stack->ctx;
    bool yes = false;
    CHK(combine_sweep_applicable(p, &yes));
    if (!yes) return 0;
    std::vector<int> st_row, st_flag;
    std::vector<double> st_a, st_b, st_c;
    double c_first = 1.0;
    StepSeries ser;
    for (int st = 0; st < p->nsteps; ++st) {
        const double* nb = bounds.data() + 3 * st;
        CHK(step_series(ctx, 1, nb[0], nb[1], nb[2], nb[0], true, false, &ser));
        const bool cheb = ser.cheb;
        const int K = cheb ? ser.K : ser.deg, reps = cheb ? ser.reps : ser.sc;
        const int slot = p->save.empty() ? -1 : p->save[st];
        if ((long long)K * reps > 4096) return 0;       // (a series this long belongs to the Arnoldi route)
        if (slot >= (1 << 23) - 1) return 0;            // (the stage word has 24 bits for the save slot + 1)
        const double h = p->hs[st], c0 = cheb ? ser.coef[0] : 1.0;
        if (st == 0) c_first = c0;
        else st_c.back() = c0;                          // the last term of the step before starts this series
        for (int rep = 0; rep < reps; ++rep)
            for (int j = 1; j <= K; ++j) {
                const bool last = j == K, step_end = last && rep + 1 == reps;
                st_row.push_back(p->rows[3 * st]);
                st_a.push_back(cheb ? h * ((j == 1 ? 1.0 : 2.0) / ser.rho) : h * (1.0 / ((double)ser.sc * (double)j)));
                st_b.push_back(cheb ? 2.0 * ser.coef[j] : 1.0);
                st_c.push_back(c0);
                // (bits 8..: save slot + 1, 0 = none -- built and decoded as an unsigned word)
                st_flag.push_back((int)((last ? 1u : 0u) | (step_end ? 2u : 0u) | (cheb ? 4u : 0u) |
                                        ((step_end && slot >= 0 ? (unsigned)slot + 1u : 0u) << 8)));
            }
    }
    DevBuf d_row, d_flag, d_a, d_b, d_c;
    CHK(d_row.upload(ctx, st_row));
    CHK(d_flag.upload(ctx, st_flag));
    CHK(d_a.upload(ctx, st_a));
    CHK(d_b.upload(ctx, st_b));
    CHK(d_c.upload(ctx, st_c));
    CombineSweepArgs a{};
    a.nstage = (int)st_row.size();
    a.st_row = d_row.as<int>();
    a.st_flag = d_flag.as<int>();
    a.st_a = d_a.as<double>();
    a.st_b = d_b.as<double>();
    a.st_c = d_c.as<double>();
    a.c_first = c_first;
    CHK(combine_sweep_launch(p, a, 1, p->y0_shared, done));
    if (!*done) return 0;
    ctx->last_sweep[0] = (double)st_row.size();
    return plan_fetch_out(p, Y_out);
}

// ---- one trajectory on a very sparse stack, Magnus order 1: the whole solve in ONE launch of ell_resident_kernel<1>
// (operator elements in registers, one exchange round per term instead of one launch; csrc/midyn_resident.h).  Per step the
// same series as the per-launch route.  *done = false: declined (a step the per-launch route gives to Arnoldi, a refused
// launch, or a wait inside the launch that gave up -- the plan's state is then reset for the per-launch route).
static int expm_route_resident(midyn_rk4_plan* p, const std::vector<double>& bounds, midyn_complex* Y_out, bool* done) {
    *done = false;
    midyn_ctx* ctx = p->stack->ctx;
    const int nsteps = p->nsteps;
    std::vector<StepSeries> ser(nsteps);
    std::vector<int> Kv(nsteps), repv(nsteps);      // (a negative K = Taylor of degree -K)
    std::vector<double> hrho(nsteps);
    for (int st = 0; st < nsteps; ++st) {
        const double* nb = bounds.data() + 3 * st;
        CHK(step_series(ctx, 1, nb[0], nb[1], nb[2], nb[0], true, false, &ser[st]));
        const StepSeries& ss = ser[st];
        // the per-launch route would hand a Taylor series this long to Arnoldi (see krylov_min there): leave it there
        if (!ss.cheb && ctx->krylov && (long long)ss.deg * ss.sc >= arnoldi_products(nb[0])) return 0;
        Kv[st] = ss.cheb ? ss.K : -ss.deg;
        repv[st] = ss.cheb ? ss.reps : ss.sc;
        hrho[st] = p->hs[st] / (ss.cheb ? ss.rho : (double)ss.sc);   // alpha_k = (1 | 2) h / (rho / reps) / reps
    }
    int stride = 0;
    const std::vector<double> coefv = cheb_table(ser, &stride);
    DevBuf d_K, d_rep, d_hrho, d_coef;
    CHK(d_K.upload(ctx, Kv));
    CHK(d_rep.upload(ctx, repv));
    CHK(d_hrho.upload(ctx, hrho));
    CHK(d_coef.upload(ctx, coefv));
    EllArgs a = ell_args(p, 0, nsteps);
    a.cheb_K = d_K.as<int>();
    a.cheb_reps = d_rep.as<int>();
    a.cheb_hrho = d_hrho.as<double>();
    a.cheb_coef = d_coef.as<double>();
    a.cheb_stride = stride;
    const int ls = launch_ell(p, a, 1);
    if (ls != 0) return ls == RESIDENT_LAUNCH_REFUSED ? 0 : ls;
    CHK(plan_fetch_out(p, Y_out));
    if (take_wait_error(ctx) == 0) {
        *done = true;
        return 0;
    }
    // a wait inside the launch gave up: the state is undefined -- the per-launch route starts again (and overwrites Y_out)
    CHK(plan_reset_state(p));
    ++ctx->resident_fallbacks;
    return 0;
}

// The per-launch route's work: the plan of the solve, the explicit generators of one instance, the work vectors, and the
// products over them.
struct ActionWork {
    midyn_rk4_plan* const p;
    midyn_ctx* const ctx;
    const int order, np, ld;
    const size_t stv, state_bytes;
    // one instance: explicit G(t_i), products on a single matrix -- unless the stack is block sparse, where
    // the per-segment work lists touch far fewer bytes than one dense n x n matrix
    const bool one;
    // Magnus 2 with a frame, products through the plan and no fused input phase (sweeps, MFMA routes): the
    // producers write the phased copies of their results (see expm_magnus2_terms)
    const bool chain_phases;
    const bool fuse_phase;
    DevBuf Gx[2], U[2], V[2], W, d_cs;
    std::vector<double> h_cs;
    DevBuf TP[4], W2;
    DevBuf kV, kH, kE, kw, khc, kbeta, kerr, kcoef, cheb_buf[2];   // (Arnoldi, Chebyshev: allocated at their first step)
    ExpmWork kwork;
    ActionWork(midyn_rk4_plan* p_, int order_)
        : p(p_), ctx(p_->stack->ctx), order(order_), np(p_->stack->n_pad), ld(p_->ld), stv((size_t)np * ld),
          state_bytes(stv * sizeof(double2)), one(p_->B == 1 && !p_->blocks),
          chain_phases(order_ == 2 && !one && p_->stack->has_frame && !(p_->blocks && p_->ncol <= 8)),
          fuse_phase(!one && p_->blocks && p_->ncol <= 8) {}

    // out = G(point i) . w   (EPI_RHS)  or the fused Taylor update (EPI_TAYLOR) with the given epilogue
    int product(int i, int row, const double2* w_plain, const double2* w_phased, Epilogue epi) {
        if (!one) return plan_rhs_launch(p, row, epi, w_phased);
        epi.e_cur = nullptr;   // gen_eval already applied the frame: G = Delta(t) o C(t)
        epi.e_next = nullptr;
        if (p->stream_path) {
            StreamArgs a{};
            a.ops = Gx[i].as<double2>();
            a.seg_list = ctx->d_one_seg;
            a.n_act = 1;
            a.n_pad = np;
            a.has_static = 1;
            a.coeff = nullptr;
            a.yin = w_plain;
            a.epi = epi;
            return launch_stream(ctx, a);
        }
        GemmArgs g{};
        g.A = Gx[i].as<double2>();
        g.lda = np;
        g.B = w_plain;
        g.ldb = ld;
        g.M = np;
        g.N = ld;
        g.K = np;
        g.seg_list = ctx->d_one_seg;
        g.n_act = 1;
        g.m_cols = p->m;
        g.n_inst = 1;
        g.epi = epi;
        return launch_gemm(ctx, g, KC_RHS_GEMM);
    }
    int rephase(const double2* src, int row, double2* dst) {
        hipLaunchKernelGGL(rephase_kernel, dim3(grid_for(stv)), dim3(256), 0, ctx->stream, src, plan_E(p, row), np, ld, dst);
        HIPCHK(ctx, hipGetLastError());
        return 0;
    }
    // out = conj-phase(G(row) . w) for an UN-phased w: explicit G (one), the block kernels' fused input phase, or
    // a rephase pass into `scratch` followed by the plan's contraction
    int product_plain(int i, int row, const double2* w, double2* scratch, Epilogue epi) {
        if (one) return product(i, row, w, w, epi);
        epi.e_cur = plan_E(p, row);
        if (fuse_phase || !plan_E(p, row)) return plan_rhs_launch(p, row, epi, w, fuse_phase ? plan_E(p, row) : nullptr);
        CHK(rephase(w, row, scratch));
        return plan_rhs_launch(p, row, epi, scratch);
    }

    // ---- Krylov alternative for ONE column and a large norm (Magnus order 1): Arnoldi on G(t1) with
    // classical Gram-Schmidt + one re-orthogonalisation, all on the device (no host round trip per
    // iteration); every few iterations expm(h H_m) of the small Hessenberg matrix (64 x 64 block, the
    // batched-expm machinery) and Saad's a-posteriori estimate beta h_{m+1,m} |e_m^T expm(h H_m) e_1|;
    // y <- beta V_m expm(h H_m) e_1.  The scaled Taylor series needs ~15 products per unit of ||h G||_1,
    // Arnoldi about 1.5 x the spectral radius + 20 in total (cfg 4, no frame: 160 -> ~40 products).
    int krylov_step(double h, int row, double bound, const double2* ycur, double2* ynew, bool* converged) {
        const int KM = 60;
        *converged = false;
        if (!kV.p) {
            CHK(kV.alloc(ctx, (size_t)(KM + 1) * np * sizeof(double2)));
            CHK(kH.alloc(ctx, 64 * 64 * sizeof(double2)));
            CHK(kE.alloc(ctx, 64 * 64 * sizeof(double2)));
            CHK(kw.alloc(ctx, (size_t)np * sizeof(double2)));
            CHK(khc.alloc(ctx, 64 * sizeof(double2)));
            CHK(kbeta.alloc(ctx, 2 * sizeof(double)));
            CHK(kerr.alloc(ctx, 2 * sizeof(double)));
            CHK(kcoef.alloc(ctx, 64 * sizeof(double2)));
        }
        double2* Vb = kV.as<double2>();
        double2* Hm = kH.as<double2>();
        double2* Es = kE.as<double2>();
        double2* wv = kw.as<double2>();
        HIPCHK(ctx, hipMemsetAsync(kH.p, 0, kH.bytes, ctx->stream));
        hipLaunchKernelGGL(krylov_norm_scale_kernel, dim3(1), dim3(1024), 0, ctx->stream, ycur, np, 0, (double2*)nullptr,
                           kbeta.as<double>(), Vb);
        int next_check = std::min(KM, std::max(8, (int)(1.5 * bound) + 14));
        int m = 0;
        bool done = false;
        for (int j = 0; j < KM && !done; ++j) {
            Epilogue e{};
            e.mode = EPI_RHS;
            e.ld = ld;
            e.out = wv;
            CHK(product_plain(0, row, Vb + (size_t)j * np, p->d_yin[0].as<double2>(), e));   // w = G v_j
            for (int pass = 0; pass < 2; ++pass) {                                           // CGS + re-orthogonalisation
                hipLaunchKernelGGL(krylov_dot_kernel, dim3(j + 1), dim3(256), 0, ctx->stream, Vb, np, wv, np, j, pass,
                                   khc.as<double2>(), Hm);
                hipLaunchKernelGGL(krylov_axpy_kernel, dim3(grid_for(np, 64)), dim3(256), 0, ctx->stream, Vb, np,
                                   khc.as<double2>(), 1, j + 1, -1.0, wv, np, wv);
            }
            hipLaunchKernelGGL(krylov_norm_scale_kernel, dim3(1), dim3(1024), 0, ctx->stream, wv, np, j, Hm,
                               kbeta.as<double>() + 1, Vb + (size_t)(j + 1) * np);
            HIPCHK(ctx, hipGetLastError());
            m = j + 1;
            if (m == next_check || m == KM) {
                hipLaunchKernelGGL(krylov_small_kernel, dim3(16), dim3(256), 0, ctx->stream, Hm, m, h, Es);
                CHK(dev_expm_inplace(ctx, kwork, Es, 64, nullptr, nullptr, 1));
                hipLaunchKernelGGL(krylov_err_kernel, dim3(1), dim3(64), 0, ctx->stream, Es, Hm, m, h, kbeta.as<double>(),
                                   kerr.as<double>());
                HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, kerr.p, 2 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
                HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
                const double err = ctx->h_pinned[0], beta = ctx->h_pinned[1];
                if (!std::isfinite(err)) return fail(ctx, "midyn_expm_solve: non-finite Krylov estimate");
                if (err <= 1e-15 * beta) done = true;
                else next_check = std::min(KM, m + 6);
            }
        }
        if (!done) return 0;   // not converged within KM vectors: the caller falls back to the Taylor series
        hipLaunchKernelGGL(krylov_coef_kernel, dim3(1), dim3(64), 0, ctx->stream, Es, m, kbeta.as<double>(),
                           kcoef.as<double2>());
        hipLaunchKernelGGL(krylov_axpy_kernel, dim3(grid_for(np, 64)), dim3(256), 0, ctx->stream, Vb, np,
                           kcoef.as<double2>(), 1, m, 1.0, (const double2*)nullptr, np, ynew);
        HIPCHK(ctx, hipGetLastError());
        *converged = true;
        return 0;
    }
};

// One repetition of a Magnus-2 step: the terms of the step's series of Omega applied to y, 4 products + one combination per
// term, summed into acc (which already holds y, or J_0 y for the Chebyshev series).  Term j (1-based): combination weights,
// addend, accumulator weight and output buffer
//   Taylor:     w = Omega term / (sc j);                       acc += w
//   Chebyshev:  phi_j = (j == 1 ? 1 : 2) Omega phi_{j-1} / rho + phi_{j-2};   acc += 2 J_j phi_j
static int expm_magnus2_terms(ActionWork& aw, const StepSeries& ser, double h, const int* rr, const double2* y, double2* acc) {
    midyn_rk4_plan* const p = aw.p;
    midyn_ctx* const ctx = aw.ctx;
    const int ld = aw.ld, nterm = ser.cheb ? ser.K : ser.deg;
    const size_t stv = aw.stv;
    const double p2 = std::sqrt(3.0) / 12;
    double2* yin[2] = {p->d_yin[0].as<double2>(), p->d_yin[1].as<double2>()};
    const double2* term = y;
    double2 *u1 = aw.U[0].as<double2>(), *u2 = aw.U[1].as<double2>(), *v1 = aw.V[0].as<double2>(), *v2 = aw.V[1].as<double2>(),
            *w = aw.W.as<double2>();
    double2* wb[2] = {aw.W.as<double2>(), ser.cheb ? aw.W2.as<double2>() : aw.W.as<double2>()};
    struct TermSpec {
        double a, b, beta;
        const double2* z;
        double2* out;
    };
    auto term_spec = [&](int j) {
        TermSpec t{};
        if (ser.cheb) {
            const double mult = (j == 1 ? 1.0 : 2.0) / ser.rho;
            t.a = 0.5 * h * mult;
            t.b = p2 * h * h * mult;
            t.beta = 2.0 * ser.coef[j];
            t.out = wb[(j - 1) & 1];
            t.z = j == 1 ? nullptr : (j == 2 ? y : wb[(j - 1) & 1]);
        } else {
            const double f = 1.0 / ((double)ser.sc * j);
            t.a = 0.5 * h * f;
            t.b = p2 * h * h * f;
            t.beta = 1.0;
            t.out = w;
            t.z = nullptr;
        }
        return t;
    };
    if (aw.chain_phases) {
        // Frames, products through the plan, no fused input phase: every product input must be
        // pre-phased.  The producers write the phased copies themselves -- the EPI_RHS epilogue's
        // second output for u1, u2, the combination kernel for the next term -- so a term is
        // 4 products + 1 combination instead of 4 re-phasing passes on top.
        double2 *tp0 = aw.TP[0].as<double2>(), *tp1 = aw.TP[1].as<double2>(), *u1p = aw.TP[2].as<double2>(),
                *u2p = aw.TP[3].as<double2>();
        const double2 *E0 = plan_E(p, rr[0]), *E1 = plan_E(p, rr[1]);
        CHK(aw.rephase(y, rr[0], tp0));
        CHK(aw.rephase(y, rr[1], tp1));
        for (int j = 1; j <= nterm; ++j) {
            Epilogue e{};
            e.mode = EPI_RHS;
            e.ld = ld;
            Epilogue e2 = e;
            e.e_cur = E0;  // u1 = g1 term, and E1 o u1 for v1
            e.out = u1;
            e.e_next = E1;
            e.yin_next = u1p;
            e2.e_cur = E1;  // u2 = g2 term, and E0 o u2 for v2
            e2.out = u2;
            e2.e_next = E0;
            e2.yin_next = u2p;
            CHK(plan_rhs_launch_pair(p, rr[0], e, tp0, rr[1], e2, tp1));   // independent: one launch
            e.e_next = e2.e_next = nullptr;
            e.yin_next = e2.yin_next = nullptr;
            e.e_cur = E1;  // v1 = g2 u1
            e.out = v1;
            e2.e_cur = E0;  // v2 = g1 u2
            e2.out = v2;
            CHK(plan_rhs_launch_pair(p, rr[1], e, u1p, rr[0], e2, u2p));
            const TermSpec ts = term_spec(j);
            hipLaunchKernelGGL(magnus2_term_kernel, dim3(grid_for(stv)), dim3(256), 0, ctx->stream, u1, u2, v1,
                               v2, ts.a, ts.b, stv, ts.out, acc, E0, E1, ld, tp0, tp1, ts.z, ts.beta);
            HIPCHK(ctx, hipGetLastError());
        }
        return 0;
    }
    for (int j = 1; j <= nterm; ++j) {
        Epilogue e{};
        e.mode = EPI_RHS;
        e.ld = ld;
        if (!aw.one && !aw.fuse_phase && !p->stack->has_frame) {
            // no frame, products through the plan: the two independent products of a level share a launch
            Epilogue e2 = e;
            e.out = u1;    // u1 = g1 term, u2 = g2 term
            e2.out = u2;
            CHK(plan_rhs_launch_pair(p, rr[0], e, term, rr[1], e2, term));
            e.out = v1;    // v1 = g2 u1, v2 = g1 u2
            e2.out = v2;
            CHK(plan_rhs_launch_pair(p, rr[1], e, u1, rr[0], e2, u2));
        } else {
            // u1 = g1 term, u2 = g2 term
            e.out = u1;
            CHK(aw.product_plain(0, rr[0], term, yin[0], e));
            e.out = u2;
            CHK(aw.product_plain(1, rr[1], term, yin[1], e));
            // v1 = g2 u1, v2 = g1 u2
            e.out = v1;
            CHK(aw.product_plain(1, rr[1], u1, yin[0], e));
            e.out = v2;
            CHK(aw.product_plain(0, rr[0], u2, yin[1], e));
        }
        const TermSpec ts = term_spec(j);
        hipLaunchKernelGGL(magnus2_term_kernel, dim3(grid_for(stv)), dim3(256), 0, ctx->stream, u1, u2, v1,
                           v2, ts.a, ts.b, stv, ts.out, acc, (const double2*)nullptr,
                           (const double2*)nullptr, ld, (double2*)nullptr, (double2*)nullptr, ts.z, ts.beta);
        HIPCHK(ctx, hipGetLastError());
        term = ts.out;
    }
    return 0;
}

// ---- per launch: every product is one launch over all instances (the batched RHS contraction, or the products on the
// explicit G(t_i) of one instance).  Per step: the Chebyshev series (Magnus 1), Arnoldi (one column, large norms), or the
// scaled Taylor series; Magnus 2: the Taylor or Chebyshev series of Omega (expm_magnus2_terms).
static int expm_route_per_launch(ActionWork& aw, const std::vector<double>& bounds, midyn_complex* Y_out) {
    midyn_rk4_plan* const p = aw.p;
    midyn_stack* const s = p->stack;
    midyn_ctx* const ctx = aw.ctx;
    const int order = aw.order, np = aw.np, ld = aw.ld;
    const size_t stv = aw.stv, state_bytes = aw.state_bytes;
    // (the work vectors of the Magnus-2 terms: allocated here -- the one-launch routes that take most sweeps never touch them,
    // and nine pool look-ups with their stream drains are 0.1 ms of a 3 ms solve)
    if (order == 2) {
        for (int i = 0; i < 2; ++i) {
            CHK(aw.U[i].alloc(ctx, state_bytes));
            CHK(aw.V[i].alloc(ctx, state_bytes));
        }
        CHK(aw.W.alloc(ctx, state_bytes));
        HIPCHK(ctx, hipMemsetAsync(aw.W.p, 0, state_bytes, ctx->stream));
        if (aw.chain_phases)
            for (int i = 0; i < 4; ++i) {
                CHK(aw.TP[i].alloc(ctx, state_bytes));
                HIPCHK(ctx, hipMemsetAsync(aw.TP[i].p, 0, state_bytes, ctx->stream));
            }
    }
    double2* y = p->d_y.as<double2>();
    double2* acc = p->d_acc.as<double2>();
    double2* yin[2] = {p->d_yin[0].as<double2>(), p->d_yin[1].as<double2>()};
    StepSeries ser;
    for (int st = 0; st < p->nsteps; ++st) {
        const double h = p->hs[st];
        const int* rr = p->rows.data() + 3 * st;
        const double* nb = bounds.data() + 3 * st;
        // ---- norm bound over the instances -> the step's series
        double bound = nb[0];
        if (aw.one) {
            for (int i = 0; i < order; ++i)
                CHK(launch_gen_eval(s, s->k > 0 ? p->d_S.as<double>() + (size_t)rr[i] * s->k : nullptr, plan_E(p, rr[i]),
                                    1.0, aw.Gx[i].as<double2>()));
            // The generators exist explicitly: their exact 1-norms can replace the triangle bound.  That
            // costs a stream synchronisation, so only when the products it may save are worth > 1 ms.
            CHK(step_series(ctx, order, bound, 0.0, 0.0, 0.0, false, false, &ser));   // (the Taylor series of the triangle bound)
            const double product_s = std::max(5e-6, (double)np * np * 16.0 / 5e12);
            if ((double)ser.deg * ser.sc * (order == 1 ? 1 : 4) * product_s > 1e-3) {
                double gn[2] = {0.0, 0.0};
                for (int i = 0; i < order; ++i) {
                    CHK(dev_norm1(ctx, aw.Gx[i].as<double2>(), np, 1, aw.d_cs, aw.h_cs));
                    gn[i] = aw.h_cs[0];
                }
                const double ah = std::fabs(h), p2 = std::sqrt(3.0) / 12;
                bound = std::min(bound, order == 1 ? ah * gn[0] : 0.5 * ah * (gn[0] + gn[1]) + 2 * p2 * ah * ah * gn[0] * gn[1]);
            }
        }
        // Taylor from the refined bound; the Chebyshev series at least for the triangle bound at order 1 (the larger of the
        // two), for the refined bound at order 2, and at order 1 only without krylov = 2
        CHK(step_series(ctx, order, bound, nb[1], nb[2], order == 1 ? nb[0] : bound, order == 2 || ctx->krylov < 2, false, &ser));
        bool stepped = false;
        // Arnoldi, when the Chebyshev series is not taken: with the microsecond products of a block-sparse stack both it and
        // the Taylor series are launch bound and the series wins unless it is several times longer (cfg 4, 100 steps: Taylor
        // 160 terms 0.100 s, Arnoldi 28 vectors 0.113 s); with dense streamed products (tens of microseconds each) Arnoldi
        // wins from 64 terms
        const long long krylov_min = ctx->krylov >= 2 ? 0 : (p->blocks ? arnoldi_products(bound) : 64);
        if (!ser.cheb && (aw.one || p->blocks) && p->stream_path && order == 1 && ctx->krylov &&
            (long long)ser.deg * ser.sc >= krylov_min) {
            bool conv = false;
            CHK(aw.krylov_step(h, rr[0], bound, y, acc, &conv));
            if (conv) {
                std::swap(y, acc);
                stepped = true;
            }
        }
        // ---- the series, `nrep` repetitions of `nterm` terms; Magnus 1: one launch per term -- the EPI_CHEB epilogue forms
        // phi_{k+1}, adds 2 J_{k+1} phi_{k+1} to the accumulator and writes the pre-phased input of the next product, EPI_TAYLOR
        // the same for the Taylor term -- Magnus 2: expm_magnus2_terms
        if (ser.cheb && order == 1 && !aw.cheb_buf[0].p)
            for (int i = 0; i < 2; ++i) CHK(aw.cheb_buf[i].alloc(ctx, state_bytes));
        if (ser.cheb && order == 2 && !aw.W2.p) {
            CHK(aw.W2.alloc(ctx, state_bytes));
            HIPCHK(ctx, hipMemsetAsync(aw.W2.p, 0, state_bytes, ctx->stream));
        }
        double2* P2[2] = {aw.cheb_buf[0].as<double2>(), aw.cheb_buf[1].as<double2>()};
        const int nrep = ser.cheb ? ser.reps : ser.sc, nterm = ser.cheb ? ser.K : ser.deg;
        const double rr_ = ser.rho / ser.reps;
        for (int rep = 0; rep < nrep && !stepped; ++rep) {
            if (ser.cheb) {
                hipLaunchKernelGGL(scale_copy_kernel, dim3(grid_for(stv)), dim3(256), 0, ctx->stream, y, ser.coef[0], stv, acc);
                HIPCHK(ctx, hipGetLastError());
            } else {
                HIPCHK(ctx, hipMemcpyAsync(acc, y, state_bytes, hipMemcpyDeviceToDevice, ctx->stream));
            }
            if (order == 1) {
                int cur = 0;
                if (aw.one) HIPCHK(ctx, hipMemcpyAsync(yin[0], y, state_bytes, hipMemcpyDeviceToDevice, ctx->stream));
                else CHK(aw.rephase(y, rr[0], yin[0]));
                for (int k = 0; k < nterm; ++k) {
                    Epilogue e{};
                    e.mode = ser.cheb ? EPI_CHEB : EPI_TAYLOR;
                    e.ld = ld;
                    if (ser.cheb) {
                        e.alpha = (k == 0 ? 1.0 : 2.0) * h / (rr_ * ser.reps);
                        e.beta = 2.0 * ser.coef[k + 1];
                        e.z = k == 0 ? nullptr : (k == 1 ? y : P2[k & 1]);
                        e.out = P2[k & 1];
                    } else {
                        e.h = h / ((double)ser.sc * (k + 1));
                    }
                    e.e_cur = plan_E(p, rr[0]);
                    e.e_next = plan_E(p, rr[0]);
                    e.acc = acc;
                    e.yin_next = yin[cur ^ 1];
                    CHK(aw.product(0, rr[0], yin[cur], yin[cur], e));
                    cur ^= 1;
                }
            } else {
                CHK(expm_magnus2_terms(aw, ser, h, rr, y, acc));
            }
            std::swap(y, acc);
        }
        const int slot = p->save.empty() ? -1 : p->save[st];
        if (slot >= 0) {
            hipLaunchKernelGGL(gather_state_kernel, dim3(grid_for((size_t)p->B * s->n * p->m)), dim3(256), 0, ctx->stream, y,
                               p->B, s->n, p->m, ld, p->P, slot, p->d_out.as<double2>());
            HIPCHK(ctx, hipGetLastError());
        }
    }
    return plan_fetch_out(p, Y_out);
}

static int expm_action_solve(midyn_stack* s, int B, int m, int R, const double* times, const double* S_any, int nsteps,
                             const int* step_rows, const double* step_h, const int* step_save, int P, int magnus_order,
                             const midyn_complex* y0, int y0_shared, midyn_complex* Y_out) {
    midyn_ctx* ctx = s->ctx;
    const TimingMarks mark{"expm_action_solve"};
    bool sweep = false;
    CHK(expm_plan_sweep_route(s, B, m, magnus_order, nsteps, &sweep));
    if (sweep)
        return expm_route_sweep_plan(s, B, m, R, times, S_any, nsteps, step_rows, step_h, step_save, P, magnus_order, y0,
                                     y0_shared, Y_out, mark);
    CHK(stack_seg_norms(s));
    midyn_rk4_plan* p = nullptr;
    CHK(plan_create_impl(s, B, m, R, times, S_any, nsteps, step_rows, step_h, step_save, P, y0, y0_shared, &p));
    struct Guard {
        midyn_rk4_plan* p;
        ~Guard() { midyn_rk4_plan_destroy(p); }
    } guard{p};
    ActionWork aw(p, magnus_order);
    if (aw.one)
        for (int i = 0; i < magnus_order; ++i) CHK(aw.Gx[i].alloc(ctx, (size_t)aw.np * aw.np * sizeof(double2)));
    mark("plan + buffers");
    // every route chooses its series from these bounds: computed once, here, so that a failed allocation, copy or launch
    // is THIS call's error status
    std::vector<double> bounds;
    CHK(expm_step_bounds(p, magnus_order, &bounds));
    mark("norm bounds");
    if (p->tiny) return expm_route_tiny(p, magnus_order, bounds, Y_out);
    if (magnus_order == 1 && ctx->krylov < 2 && nsteps > 0) {
        bool done = false;
        CHK(expm_route_combine_sweep(p, bounds, Y_out, &done));
        if (!done && p->resident_ell) CHK(expm_route_resident(p, bounds, Y_out, &done));
        if (done) return 0;
    }
    return expm_route_per_launch(aw, bounds, Y_out);
}

// The exponential itself (many columns per instance, or Magnus order 3): instances advance together in chunks -- every
// generator evaluation, Magnus combination, expm product and propagation is ONE batched launch over the chunk (a single
// instance per chunk when one n x n expm already fills the device).
static int expm_dense_solve(midyn_stack* s, int B, int m, int R, const double* times, const double* S, int nsteps,
                            const int* step_rows, const double* step_h, const int* step_save, int P, int magnus_order,
                            const midyn_complex* y0, int y0_shared, midyn_complex* Y_out) {
    midyn_ctx* ctx = s->ctx;
    const int np = s->n_pad;
    const int ld = round_up(m, 64);
    const int chunk = expm_chunk(ctx, np, B);
    const size_t mat = (size_t)np * np;          // elements per matrix
    const size_t stv = (size_t)np * ld;          // elements per state block
    DevBuf d_S, d_times, d_E, d_y[2], d_tmp, d_out, G[3], W[4], Om;
    ExpmWork w;
    if (s->k > 0) {
        CHK(d_S.alloc(ctx, (size_t)B * R * s->k * sizeof(double)));
        HIPCHK(ctx, copy_to_device_any(ctx, d_S.p, S, d_S.bytes));  // host or device table
    }
    CHK(make_phase_rows(s, times, R, d_times, d_E));
    CHK(d_y[0].alloc(ctx, chunk * stv * sizeof(double2)));
    CHK(d_y[1].alloc(ctx, chunk * stv * sizeof(double2)));
    const size_t inst_elems = (size_t)s->n * m;
    CHK(d_tmp.alloc(ctx, inst_elems * sizeof(double2)));
    CHK(d_out.alloc(ctx, (size_t)chunk * P * inst_elems * sizeof(double2)));
    CHK(Om.alloc(ctx, chunk * mat * sizeof(double2)));
    for (int i = 0; i < magnus_order; ++i) CHK(G[i].alloc(ctx, chunk * mat * sizeof(double2)));
    if (magnus_order >= 2)
        for (int i = 0; i < (magnus_order == 2 ? 2 : 4); ++i) CHK(W[i].alloc(ctx, chunk * mat * sizeof(double2)));
    auto Erow = [&](int row) -> const double2* {
        return s->has_frame ? d_E.as<double2>() + (size_t)row * np : nullptr;
    };
    const long long cstride = (long long)R * s->k;
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = std::min(chunk, B - b0);
        HIPCHK(ctx, hipMemsetAsync(d_y[0].p, 0, nb * stv * sizeof(double2), ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(d_y[1].p, 0, nb * stv * sizeof(double2), ctx->stream));
        for (int b = 0; b < nb; ++b) {
            const midyn_complex* y0b = y0 + (y0_shared ? 0 : (size_t)(b0 + b) * inst_elems);
            if (b == 0 || !y0_shared) {
                HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // d_tmp is reused
                HIPCHK(ctx, hipMemcpyAsync(d_tmp.p, y0b, inst_elems * sizeof(double2), hipMemcpyHostToDevice,
                                           ctx->stream));
            }
            hipLaunchKernelGGL(scatter_state_kernel, dim3(grid_for(inst_elems)), dim3(256), 0, ctx->stream,
                               d_tmp.as<double2>(), 1, 1, s->n, m, ld, (const double2*)nullptr,
                               d_y[0].as<double2>() + b * stv, (double2*)nullptr);
            hipLaunchKernelGGL(gather_state_kernel, dim3(grid_for(inst_elems)), dim3(256), 0, ctx->stream,
                               d_y[0].as<double2>() + b * stv, 1, s->n, m, ld, P, 0,
                               d_out.as<double2>() + (size_t)b * P * inst_elems);
        }
        HIPCHK(ctx, hipGetLastError());
        int cur = 0;
        const double* coeff_b = s->k > 0 ? d_S.as<double>() + (size_t)b0 * R * s->k : nullptr;
        for (int st = 0; st < nsteps; ++st) {
            const double h = step_h[st];
            const int* rr = step_rows + 3 * st;
            auto cf = [&](int row) { return coeff_b ? coeff_b + (size_t)row * s->k : nullptr; };
            auto gen = [&](int gi, double scale, double2* out) {
                return launch_gen_eval(s, cf(rr[gi]), Erow(rr[gi]), scale, out, nb, cstride);
            };
            double2* Omega = Om.as<double2>();
            CHK(magnus_omega(ctx, np, nb, magnus_order, h, gen, G, W, Omega));
            CHK(dev_expm_inplace(ctx, w, Omega, np, nullptr, nullptr, nb));
            // y <- expm(Omega) y  for every instance of the chunk
            CHK(dev_zgemm_batched(ctx, nb, np, ld, np, Omega, np, (long long)mat, d_y[cur].as<double2>(), ld,
                                  (long long)stv, d_y[cur ^ 1].as<double2>(), ld, (long long)stv, 1.0, 0.0, nullptr));
            cur ^= 1;
            if (step_save && step_save[st] >= 0) {
                for (int b = 0; b < nb; ++b)
                    hipLaunchKernelGGL(gather_state_kernel, dim3(grid_for(inst_elems)), dim3(256), 0, ctx->stream,
                                       d_y[cur].as<double2>() + b * stv, 1, s->n, m, ld, P, step_save[st],
                                       d_out.as<double2>() + (size_t)b * P * inst_elems);
                HIPCHK(ctx, hipGetLastError());
            }
        }
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        HIPCHK(ctx, hipMemcpy(Y_out + (size_t)b0 * P * inst_elems, d_out.p, (size_t)nb * P * inst_elems * sizeof(double2),
                              hipMemcpyDeviceToHost));
    }
    return 0;
}

extern "C" int midyn_expm_solve(midyn_stack* s, int B, int m, int R, const double* times, const double* S,
                                int nsteps, const int* step_rows, const double* step_h, const int* step_save,
                                int P, int magnus_order, const midyn_complex* y0, int y0_shared,
                                midyn_complex* Y_out) {
    if (!s || !Y_out || !y0 || !times || !step_rows || !step_h)
        return fail(s ? s->ctx : nullptr, "midyn_expm_solve: NULL argument");
    midyn_ctx* ctx = s->ctx;
    if (magnus_order < 1 || magnus_order > 3) return fail(ctx, "Only magnus_order 1, 2, and 3 are supported.");
    if (B <= 0 || m <= 0 || R <= 0 || P < 1) return fail(ctx, "midyn_expm_solve: bad sizes");
    if (s->k > 0 && !S) return fail(ctx, "midyn_expm_solve: S is NULL but the stack has operators");
    for (int i = 0; i < 3 * nsteps; ++i)
        if (step_rows[i] < 0 || step_rows[i] >= R) return fail(ctx, "midyn_expm_solve: step_rows out of range");
    // (every route refuses these before it starts any device work; a negative slot: no save)
    for (int st = 0; step_save && st < nsteps; ++st)
        if (step_save[st] >= P) return fail(ctx, "midyn_expm_solve: save slot out of range");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (ctx->expm_action && magnus_order <= 2 && (long long)m * 16 <= s->n_pad) {
        // few columns per instance: expm(Omega) y by matrix-vector products (see expm_action_solve)
        return expm_action_solve(s, B, m, R, times, S, nsteps, step_rows, step_h, step_save, P, magnus_order, y0,
                                 y0_shared, Y_out);
    }
    return expm_dense_solve(s, B, m, R, times, S, nsteps, step_rows, step_h, step_save, P, magnus_order, y0, y0_shared, Y_out);
}
