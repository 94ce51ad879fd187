// midyn_parallel.inc -- part of midyn.hip (one translation unit; included in order): parallel-in-time propagation (row f3)
// -------------------------------------------------------------------------------------------------
// Parallel-in-time propagation (SURVEY section 8 row f3; fixed_step_lmde_solver_parallel_template_jax,
// solvers/fixed_step_solvers.py:524-613, with the step rules of jax_RK4_parallel_solver :222-258 and
// jax_expm_parallel_solver :289-316):
//   1. the propagators of ALL time steps of a chunk are formed by batched launches
//        RK4:   P_i = I + (k1 + 2 k2 + 2 k3 + k4)/6,  k1 = hG(t), k2 = hG(t+h/2)(I + k1/2), ...
//        expm:  P_i = expm(Omega_m(t_i, h_i))
//   2. the propagators between consecutive output times are multiplied by a binary tree, every tree
//      level being ONE batched zgemm over all pairs of all intervals (work T-1 products, depth log2),
//   3. the (few) interval propagators are applied to the state in time order.
// The reference scans all prefix products (associative_scan) and keeps the ones at t_list; only those
// are formed here.  Products are re-associated, so results agree with the sequential methods to
// rounding, not bit for bit (as in the reference, whose tests compare the two the same way).
// -------------------------------------------------------------------------------------------------
// Step 1 for a chunk of nb steps: the step propagators -> X[0..nb).  gen(gi, scale, out) writes scale * h_i G(t) at
// the gi-th evaluation point of every step i of the chunk (the generators carry their step size, so Magnus serves steps
// of different sizes with h = 1: Omega_m is homogeneous in h G).  Shared with midyn_gentable (midyn_gentable.inc).
template <class Gen>
static int form_step_propagators(midyn_ctx* ctx, int np, int nb, int method, Gen&& gen, DevBuf* G, DevBuf* W,
                                 ExpmWork& w, double2* Xb) {
    if (method == 0) {
        double2 *k1 = G[0].as<double2>(), *gh = G[1].as<double2>(), *g1 = G[2].as<double2>();
        double2 *k2 = W[0].as<double2>(), *k3 = W[1].as<double2>(), *k4 = W[2].as<double2>();
        CHK(gen(0, 1.0, k1));
        CHK(gen(1, 1.0, gh));
        CHK(gen(2, 1.0, g1));
        CHK(dev_sqgemm(ctx, nb, np, gh, k1, k2, 0.5, 1.0, gh));  // k2 = hG(t+h/2) (I + k1/2)
        CHK(dev_sqgemm(ctx, nb, np, gh, k2, k3, 0.5, 1.0, gh));  // k3 = hG(t+h/2) (I + k2/2)
        CHK(dev_sqgemm(ctx, nb, np, g1, k3, k4, 1.0, 1.0, g1));  // k4 = hG(t+h)   (I + k3)
        const double2* xs[4] = {k1, k2, k3, k4};
        double al[4] = {1.0 / 6, 1.0 / 3, 1.0 / 3, 1.0 / 6};
        CHK(dev_lincomb(ctx, np, Xb, 4, xs, al, 1.0, nb));
    } else {
        CHK(magnus_omega(ctx, np, nb, method, 1.0, gen, G, W, Xb));  // generators carry h already
        CHK(dev_expm_inplace(ctx, w, Xb, np, nullptr, nullptr, nb));
    }
    return 0;
}

// Steps 2 and 3 for a chunk: X holds 2 x cap matrices (the tree ping-pongs between the halves), step_save the save slots
// of the chunk's steps; the state d_y[cur] ([np][ld]) advances through the chunk, the states at the output times go to
// out[P][n][m].  Shared with midyn_gentable.
static int tree_apply_chunk(midyn_ctx* ctx, int np, int ld, int nb, int cap, const int* step_save, double2* Xb,
                            DevBuf& d_offs, DevBuf* d_y, int& cur, int n, int m, int P, double2* out,
                            std::vector<int>& loc, std::vector<long long>& offs, std::vector<int>& round_start) {
    const size_t mat = (size_t)np * np;
    const size_t inst_elems = (size_t)n * m;
    // -- 2. binary-tree products inside every interval [a, e) between output times
    std::vector<std::pair<int, int>> segs;
    for (int a = 0; a < nb;) {
        int e = a;
        while (e < nb && step_save[e] < 0) ++e;
        e = std::min(nb, e + 1);
        segs.emplace_back(a, e);
        a = e;
    }
    std::fill(loc.begin(), loc.begin() + nb, 0);
    auto slot = [&](int which, int i) { return (long long)((size_t)which * cap + i) * (long long)mat; };
    int longest = 0;
    for (auto& sg : segs) longest = std::max(longest, sg.second - sg.first);
    // all levels' offset tables go to the device in ONE copy (a level has at most half the entries of
    // the one before: fewer than nb products in total)
    offs.clear();
    round_start.clear();
    for (int st = 1; st < longest; st *= 2) {
        round_start.push_back((int)(offs.size() / 3));
        for (auto& sg : segs)
            for (int i = sg.first; i + st < sg.second; i += 2 * st) {
                offs.push_back(slot(loc[i + st], i + st));  // later steps multiply from the left
                offs.push_back(slot(loc[i], i));
                offs.push_back(slot(loc[i] ^ 1, i));
                loc[i] ^= 1;
            }
    }
    round_start.push_back((int)(offs.size() / 3));
    if (!offs.empty()) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));  // the previous chunk may still read d_offs
        HIPCHK(ctx, hipMemcpy(d_offs.p, offs.data(), offs.size() * sizeof(long long), hipMemcpyHostToDevice));
        for (size_t lv = 0; lv + 1 < round_start.size(); ++lv) {
            const int cnt = round_start[lv + 1] - round_start[lv];
            if (cnt > 0)
                CHK(dev_zgemm_batched(ctx, cnt, np, np, np, Xb, np, 0, Xb, np, 0, Xb, np, 0, 1.0, 0.0, nullptr,
                                      d_offs.as<long long>() + (size_t)3 * round_start[lv]));
        }
    }
    // -- 3. apply the interval propagators in time order, store the states at the output times
    for (auto& sg : segs) {
        const double2* Q = Xb + slot(loc[sg.first], sg.first);
        CHK(dev_zgemm(ctx, np, ld, np, Q, np, d_y[cur].as<double2>(), ld, d_y[cur ^ 1].as<double2>(), ld, 1.0,
                      0.0, nullptr));
        cur ^= 1;
        const int sv = step_save[sg.second - 1];
        if (sv >= 0) {
            hipLaunchKernelGGL(gather_state_kernel, dim3(grid_for(inst_elems)), dim3(256), 0, ctx->stream,
                               d_y[cur].as<double2>(), 1, n, m, ld, P, sv, out);
            HIPCHK(ctx, hipGetLastError());
        }
    }
    return 0;
}

extern "C" int midyn_parallel_solve(midyn_stack* s, int B, int m, int R, const double* times, const double* S,
                                    int nsteps, const int* step_rows, const double* step_h, const int* step_save,
                                    int P, int method, const midyn_complex* y0, int y0_shared,
                                    midyn_complex* Y_out) {
    if (!s || !Y_out || !y0 || !times || !step_rows || !step_h || !step_save)
        return fail(s ? s->ctx : nullptr, "midyn_parallel_solve: NULL argument");
    midyn_ctx* ctx = s->ctx;
    if (method < 0 || method > 3) return fail(ctx, "midyn_parallel_solve: method must be 0 (RK4) or a Magnus order 1..3");
    if (B <= 0 || m <= 0 || R <= 0 || P < 1 || nsteps < 0) return fail(ctx, "midyn_parallel_solve: bad sizes");
    if (s->k > 0 && !S) return fail(ctx, "midyn_parallel_solve: S is NULL but the stack has operators");
    for (int i = 0; i < 3 * nsteps; ++i)
        if (step_rows[i] < 0 || step_rows[i] >= R) return fail(ctx, "midyn_parallel_solve: step_rows out of range");
    for (int i = 0; i < nsteps; ++i)
        if (step_save[i] >= P) return fail(ctx, "midyn_parallel_solve: save slot out of range");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int np = s->n_pad;
    const int ld = round_up(m, 64);
    const size_t mat = (size_t)np * np, stv = (size_t)np * ld;
    const int npts = method == 0 ? 3 : method;  // generator evaluations per step
    const int cap = std::max(1, expm_chunk(ctx, np, std::max(1, nsteps)));
    const int k = s->k;
    DevBuf d_S, d_times, d_E, d_rows, d_h, d_C[3], d_Eg[3], X, G[3], W[4], d_offs, d_y[2], d_tmp, d_out;
    ExpmWork w;
    if (k > 0) CHK(d_S.alloc(ctx, (size_t)R * k * sizeof(double)));
    CHK(make_phase_rows(s, times, R, d_times, d_E));
    // step tables, transposed to [point][step] so that a chunk of steps is contiguous
    std::vector<int> rows_t((size_t)3 * std::max(1, nsteps));
    for (int i = 0; i < nsteps; ++i)
        for (int gi = 0; gi < 3; ++gi) rows_t[(size_t)gi * nsteps + i] = step_rows[3 * i + gi];
    CHK(d_rows.alloc(ctx, rows_t.size() * sizeof(int)));
    CHK(d_h.alloc(ctx, (size_t)std::max(1, nsteps) * sizeof(double)));
    if (nsteps > 0) {
        HIPCHK(ctx, hipMemcpy(d_rows.p, rows_t.data(), rows_t.size() * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(ctx, hipMemcpy(d_h.p, step_h, (size_t)nsteps * sizeof(double), hipMemcpyHostToDevice));
    }
    for (int gi = 0; gi < npts; ++gi) {
        if (k > 0) CHK(d_C[gi].alloc(ctx, (size_t)cap * k * sizeof(double)));
        if (s->has_frame) CHK(d_Eg[gi].alloc(ctx, (size_t)cap * np * sizeof(double2)));
    }
    CHK(X.alloc(ctx, 2 * (size_t)cap * mat * sizeof(double2)));
    const int n_g = method == 0 ? 3 : (method == 1 ? 0 : method);
    const int n_w = method == 0 ? 3 : (method == 2 ? 2 : (method == 3 ? 4 : 0));
    for (int i = 0; i < n_g; ++i) CHK(G[i].alloc(ctx, (size_t)cap * mat * sizeof(double2)));
    for (int i = 0; i < n_w; ++i) CHK(W[i].alloc(ctx, (size_t)cap * mat * sizeof(double2)));
    CHK(d_offs.alloc(ctx, (size_t)3 * cap * sizeof(long long)));
    CHK(d_y[0].alloc(ctx, stv * sizeof(double2)));
    CHK(d_y[1].alloc(ctx, stv * sizeof(double2)));
    const size_t inst_elems = (size_t)s->n * m;
    CHK(d_tmp.alloc(ctx, inst_elems * sizeof(double2)));
    CHK(d_out.alloc(ctx, (size_t)P * inst_elems * sizeof(double2)));
    double2* Xb = X.as<double2>();
    std::vector<long long> offs;
    std::vector<int> loc(cap), round_start;
    for (int b = 0; b < B; ++b) {
        if (k > 0)  // host or device table (midyn_sigtable_data)
            HIPCHK(ctx, copy_to_device_any(ctx, d_S.p, S + (size_t)b * R * k, (size_t)R * k * sizeof(double)));
        HIPCHK(ctx, hipMemsetAsync(d_y[0].p, 0, stv * sizeof(double2), ctx->stream));
        HIPCHK(ctx, hipMemsetAsync(d_y[1].p, 0, stv * sizeof(double2), ctx->stream));
        if (b == 0 || !y0_shared)
            HIPCHK(ctx, hipMemcpy(d_tmp.p, y0 + (y0_shared ? 0 : (size_t)b * inst_elems), inst_elems * sizeof(double2),
                                  hipMemcpyHostToDevice));
        hipLaunchKernelGGL(scatter_state_kernel, dim3(grid_for(inst_elems)), dim3(256), 0, ctx->stream,
                           d_tmp.as<double2>(), 1, 1, s->n, m, ld, (const double2*)nullptr, d_y[0].as<double2>(),
                           (double2*)nullptr);
        hipLaunchKernelGGL(gather_state_kernel, dim3(grid_for(inst_elems)), dim3(256), 0, ctx->stream,
                           d_y[0].as<double2>(), 1, s->n, m, ld, P, 0, d_out.as<double2>());
        HIPCHK(ctx, hipGetLastError());
        int cur = 0;
        for (int c0 = 0; c0 < nsteps; c0 += cap) {
            const int nb = std::min(cap, nsteps - c0);
            // -- 1. coefficient / phase rows of the chunk's steps, then all step propagators -> X[0..nb)
            for (int gi = 0; gi < npts; ++gi) {
                const int* rows_g = d_rows.as<int>() + (size_t)gi * nsteps + c0;
                if (k > 0)
                    hipLaunchKernelGGL(gather_rows_kernel, dim3(grid_for((size_t)nb * k)), dim3(256), 0, ctx->stream,
                                       d_S.as<double>(), rows_g, nb, k, d_C[gi].as<double>());
                if (s->has_frame)
                    hipLaunchKernelGGL(gather_rows_kernel, dim3(grid_for((size_t)nb * np * 2)), dim3(256), 0,
                                       ctx->stream, d_E.as<double>(), rows_g, nb, 2 * np, d_Eg[gi].as<double>());
            }
            HIPCHK(ctx, hipGetLastError());
            const double* hvec = d_h.as<double>() + c0;
            auto gen = [&](int gi, double scale, double2* out) {
                return launch_gen_eval(s, k > 0 ? d_C[gi].as<double>() : nullptr,
                                       s->has_frame ? d_Eg[gi].as<double2>() : nullptr, scale, out, nb, k, np, hvec);
            };
            CHK(form_step_propagators(ctx, np, nb, method, gen, G, W, w, Xb));
            CHK(tree_apply_chunk(ctx, np, ld, nb, cap, step_save + c0, Xb, d_offs, d_y, cur, s->n, m, P, d_out.as<double2>(),
                                 loc, offs, round_start));
        }
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        HIPCHK(ctx, hipMemcpy(Y_out + (size_t)b * P * inst_elems, d_out.p, (size_t)P * inst_elems * sizeof(double2),
                              hipMemcpyDeviceToHost));
    }
    return 0;
}
