// midyn_launch.inc -- part of midyn.hip (one translation unit; included in order): kernel launch helpers: tile / split-K choice of the MFMA contraction, streaming and work-list launchers, norms
// -------------------------------------------------------------------------------------------------
// kernel launch helpers
// -------------------------------------------------------------------------------------------------
template <int BM, int BN, int WM, int WN, int BK, int MODE, int MINW = 2, bool SPARSE = false>
static int launch_gemm_mode(midyn_ctx* ctx, const GemmArgs& g) {
    constexpr int THREADS = 64 * WM * WN;
    constexpr size_t SMEM = (size_t)2 * BK * (BM + BN) * sizeof(double2);
    static DeviceOnce attr_set;
    auto kern = zgemm_seg_kernel<BM, BN, WM, WN, BK, MODE, MINW, SPARSE>;
    note_variant("zgemm_seg_kernel", {BM, BN, WM, WN, BK, MODE, MINW, SPARSE ? 1 : 0});
    if (attr_set.needed(ctx->device)) {
        HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)SMEM));
        attr_set.done(ctx->device);
    }
    const int blocks = (g.M / BM) * (g.N / BN) * g.splits;
    hipLaunchKernelGGL(kern, dim3(blocks, g.batch > 1 ? g.batch : 1), dim3(THREADS), SMEM, ctx->stream, g);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

template <int BM, int BN, int WM, int WN, int BK, int MODE>
static int launch_pair_mode(midyn_ctx* ctx, const GemmPair& gp) {
    constexpr int THREADS = 64 * WM * WN;
    constexpr size_t SMEM = (size_t)2 * BK * (BM + BN) * sizeof(double2);
    static DeviceOnce attr_set;
    auto kern = zgemm_seg_pair_kernel<BM, BN, WM, WN, BK, MODE, 2, true>;
    note_variant("zgemm_seg_pair_kernel", {BM, BN, WM, WN, BK, MODE, 2, 1});
    if (attr_set.needed(ctx->device)) {
        HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)SMEM));
        attr_set.done(ctx->device);
    }
    const GemmArgs& g = gp.g[0];
    const int blocks = (g.M / BM) * (g.N / BN) * g.splits;
    hipLaunchKernelGGL(kern, dim3(blocks, 2), dim3(THREADS), SMEM, ctx->stream, gp);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

template <int BM, int BN, int WM, int WN, int BK>
static int launch_pair_cfg(midyn_ctx* ctx, const GemmPair& gp, int uniform_mode) {
    switch (uniform_mode) {
        case 1: return launch_pair_mode<BM, BN, WM, WN, BK, 1>(ctx, gp);
        case 2: return launch_pair_mode<BM, BN, WM, WN, BK, 2>(ctx, gp);
        case 0: return launch_pair_mode<BM, BN, WM, WN, BK, 0>(ctx, gp);
        default: return launch_pair_mode<BM, BN, WM, WN, BK, 3>(ctx, gp);
    }
}

// the panel tiles (32 / 16 rows) exist on the work lists only: no dense instantiation is referenced (16 kernels fewer, round 6)
template <int BM, int BN, int WM, int WN, int BK>
static int launch_gemm_lists_cfg(midyn_ctx* ctx, const GemmArgs& g, int uniform_mode) {
    switch (uniform_mode) {
        case 1: return launch_gemm_mode<BM, BN, WM, WN, BK, 1, 2, true>(ctx, g);
        case 2: return launch_gemm_mode<BM, BN, WM, WN, BK, 2, 2, true>(ctx, g);
        case 0: return launch_gemm_mode<BM, BN, WM, WN, BK, 0, 2, true>(ctx, g);
        default: return launch_gemm_mode<BM, BN, WM, WN, BK, 3, 2, true>(ctx, g);
    }
}

// uniform_mode: 0/1/2 when every active segment has that plane mode (straight-line specialised
// kernel), 3 when the stack is mixed (per-segment run-time flags)
template <int BM, int BN, int WM, int WN, int BK>
static int launch_gemm_cfg(midyn_ctx* ctx, const GemmArgs& g, int uniform_mode) {
    if (g.work_ptr) {  // block-sparse stack: tile lists instead of the full (K tile, segment) loop
        switch (uniform_mode) {
            case 1: return launch_gemm_mode<BM, BN, WM, WN, BK, 1, 2, true>(ctx, g);
            case 2: return launch_gemm_mode<BM, BN, WM, WN, BK, 2, 2, true>(ctx, g);
            case 0: return launch_gemm_mode<BM, BN, WM, WN, BK, 0, 2, true>(ctx, g);
            default: return launch_gemm_mode<BM, BN, WM, WN, BK, 3, 2, true>(ctx, g);
        }
    }
    switch (uniform_mode) {
        case 0: return launch_gemm_mode<BM, BN, WM, WN, BK, 0>(ctx, g);
        case 1: return launch_gemm_mode<BM, BN, WM, WN, BK, 1>(ctx, g);
        case 2: return launch_gemm_mode<BM, BN, WM, WN, BK, 2>(ctx, g);
        case 4:   // 3M: three accumulator sets fit the registers on the 64 x 64 tile only (bigger tiles spill: not built)
            if constexpr (BM == 64 && BN == 64) return launch_gemm_mode<BM, BN, WM, WN, BK, 4>(ctx, g);
            else return launch_gemm_mode<BM, BN, WM, WN, BK, 0>(ctx, g);
        default: return launch_gemm_mode<BM, BN, WM, WN, BK, 3>(ctx, g);
    }
}

// split-K workspace + bookkeeping (g.splits / g.partial)
// `tiles` > 0: the launch has tiles * splits workgroups, at most one per CU, so all of them are co-resident and the
// partials can be summed inside the launch (GemmArgs::sync); 0: separate reduction kernel (launch_reduce)
static int setup_splits(midyn_ctx* ctx, GemmArgs& g, int splits, long long tiles = 0) {
    g.splits = 1;
    g.partial = nullptr;
    g.sync = nullptr;
    g.sync_err = nullptr;
    if (splits <= 1) return 0;
    if (ctx->splitk_inlaunch && tiles > 0 && tiles <= midyn_ctx::SYNC_TILES && tiles * splits <= ctx->num_cu &&
        g.batch <= 1 && !g.batch_offs) {
        g.sync = ctx->d_sync;
        g.sync_err = ctx->d_sync_err;
    }
    const size_t need = (size_t)splits * g.M * g.N * sizeof(double2);
    if (ctx->splitk_bytes < need) {
        if (ctx->splitk_ws) hipFree(ctx->splitk_ws);
        ctx->splitk_ws = nullptr;
        ctx->splitk_bytes = 0;
        HIPCHK(ctx, hipMalloc(&ctx->splitk_ws, need));
        ctx->splitk_bytes = need;
    }
    g.splits = splits;
    g.partial = static_cast<double2*>(ctx->splitk_ws);
    return 0;
}

// sum the split-K partials and run the epilogue (no-op when the launch was not split)
static int launch_reduce(midyn_ctx* ctx, const GemmArgs& g) {
    if (g.splits <= 1 || g.sync) return 0;   // not split, or already reduced inside the launch
    const int splits = g.splits;
    const dim3 rgrid(grid_for((size_t)g.M * g.N, 2048)), rblock(256);
#define MIDYN_REDUCE_S(MODE_, S_) \
    hipLaunchKernelGGL((splitk_reduce_kernel<MODE_, S_>), rgrid, rblock, 0, ctx->stream, g.partial, splits, g.M, g.N, g.epi)
#define MIDYN_REDUCE(MODE_)                                   \
    switch (splits) {                                         \
        case 2: MIDYN_REDUCE_S(MODE_, 2); break;              \
        case 4: MIDYN_REDUCE_S(MODE_, 4); break;              \
        case 8: MIDYN_REDUCE_S(MODE_, 8); break;              \
        case 16: MIDYN_REDUCE_S(MODE_, 16); break;            \
        default: MIDYN_REDUCE_S(MODE_, 0); break;             \
    }
    switch (g.epi.mode) {
        case EPI_RHS: MIDYN_REDUCE(EPI_RHS); break;
        case EPI_RK1: MIDYN_REDUCE(EPI_RK1); break;
        case EPI_RK2: MIDYN_REDUCE(EPI_RK2); break;
        case EPI_RK3: MIDYN_REDUCE(EPI_RK3); break;
        case EPI_RK4: MIDYN_REDUCE(EPI_RK4); break;
        case EPI_TAYLOR: MIDYN_REDUCE(EPI_TAYLOR); break;
        case EPI_CHEB: MIDYN_REDUCE(EPI_CHEB); break;
        default: MIDYN_REDUCE(EPI_PLAIN); break;
    }
#undef MIDYN_REDUCE_S
#undef MIDYN_REDUCE
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

// Block-sparse stacks: which tile lists to run on -- 0: 64-row panels (64 x 64 tiles), 1: 128-row panels
// (128 x 128), 2: 32-row panels (32 x 128), 3: 16-row panels (16 x 128).  A tall panel lists every K tile that
// ANY of its 16-row groups touches, so for scattered patterns the short panels execute far fewer zero tiles:
// cfg 5 (n = 4096, 9 operators), 128 instances -- listed tiles 3584 / 3840 / 4096 / 4352 for 128 / 64 / 32 / 16
// rows, i.e. the listed WORK halves with the panel height; microseconds per contraction for 128 / 512
// instances: 86.5 / 256.7, 55.6 / 152.6, 38.1 / 94.1, 28.2 / 77.0.  Time per unit of listed density relative to
// the 128 x 128 tile (from those runs): 64 rows 1.2, 32 rows 1.55, 16 rows 2.15 -- the weights below, so that
// block-dense patterns keep the big tile.
static const double SPARSE_TILE_WEIGHT[4] = {1.2, 1.0, 1.55, 2.15};
static int sparse_tile(const midyn_ctx* ctx, const midyn_stack* s, int M, int N) {
    // (the 32- and 16-row panels run 128 columns wide, or 64 wide when the state block is not a multiple of 128)
    const bool ok[4] = {true, M % 128 == 0 && N % 128 == 0 && s->gw_ptr[1] != nullptr,
                        M % 32 == 0 && s->gw_ptr[2] != nullptr, s->gw_ptr[3] != nullptr};
    if (ctx->sparse_bm == 64 || ctx->force_tile == 64) return 0;
    if (ctx->sparse_bm == 128 && ok[1]) return 1;
    if (ctx->sparse_bm == 32 && ok[2]) return 2;
    if (ctx->sparse_bm == 16 && ok[3]) return 3;
    int best = 0;
    for (int t = 1; t < 4; ++t)
        if (ok[t] && s->gw_density[t] * SPARSE_TILE_WEIGHT[t] < s->gw_density[best] * SPARSE_TILE_WEIGHT[best]) best = t;
    // narrow state blocks (small shards of a sweep): the 128 x 128 tile would be split 16-32 ways to fill the chip and
    // write 67 MB of partials; 64 x 64 tiles need a quarter of that (symmetry-sector stack, n = 1024: 128 columns 62.2
    // vs 68.3 us, 256 columns 105.1 vs 111.6 us; from 512 columns on the big tile wins)
    if (best == 1 && N <= 256) best = 0;
    return best;
}

// listed work of tile lists t relative to the dense 128 x 128 contraction of the same stack (1.0 = break even)
static double sparse_relative_cost(const midyn_stack* s, int t) { return s->gw_density[t] * SPARSE_TILE_WEIGHT[t]; }

// tile choice: 128x128 (8 waves) when that still gives >= 1 block per CU, else 64x64 (4 waves)
static int launch_gemm(midyn_ctx* ctx, const GemmArgs& g_in, int cls, int uniform_mode = 0,
                       const midyn_stack* sparse = nullptr) {
    const GemmArgs& g0 = g_in;
    if (g0.M % 64 || g0.N % 64 || g0.K % GEMM_BK)
        return fail(ctx, "launch_gemm: dimensions must be padded to 64/64/16");
    if (g0.n_act > 64) {
        // The kernel keeps its (<= 64 entry) segment table in one VGPR: longer lists run as several launches over
        // chunks of 64 segments, each writing raw partial sums next to the split-K partials; one reduction adds
        // all of them in a fixed order and runs the epilogue.
        if (sparse || g0.batch > 1 || g0.batch_offs) return fail(ctx, "launch_gemm: more than 64 segments in a batched/sparse launch");
        ProfScope ps(ctx, cls);
        const int chunks = (g0.n_act + 63) / 64;
        const bool t128c = (g0.M % 128 == 0) && (g0.N % 128 == 0) && ctx->force_tile != 64;
        const long long tiles = t128c ? (long long)(g0.M / 128) * (g0.N / 128) : (long long)(g0.M / 64) * (g0.N / 64);
        const int KTc = g0.K / GEMM_BK;
        int sp = 1;
        if (ctx->split_k)
            while ((long long)sp * 2 * tiles * chunks <= ctx->num_cu && KTc % (sp * 2) == 0 && KTc / (sp * 2) >= 2) sp *= 2;
        GemmArgs gall = g_in;
        gall.work_ptr = gall.work_idx = nullptr;
        gall.ablate = 0;
        CHK(setup_splits(ctx, gall, std::max(2, chunks * sp)));   // workspace for every slab
        int um = uniform_mode == 4 ? 0 : uniform_mode;
        for (int c = 0; c < chunks; ++c) {
            GemmArgs gc = gall;
            gc.seg_list = g0.seg_list + 64 * c;
            gc.n_act = std::min(64, g0.n_act - 64 * c);
            gc.splits = sp;
            gc.partial = gall.partial + (size_t)c * sp * g0.M * g0.N;
            int st = t128c ? launch_gemm_cfg<128, 128, 2, 4, 16>(ctx, gc, um) : launch_gemm_cfg<64, 64, 2, 2, 16>(ctx, gc, um);
            if (st) return st;
        }
        gall.splits = chunks * sp;
        return launch_reduce(ctx, gall);
    }
    GemmArgs g = g_in;
    if (uniform_mode == 0 && !sparse && (ctx->complex_3m >= 2 || (ctx->complex_3m == 1 && !ctx->direct_eval))) uniform_mode = 4;  // dense complex: 3 real MFMAs per product
    g.work_ptr = g.work_idx = nullptr;
    g.ablate = ctx->ablate;
    g.splits = 1;
    g.partial = nullptr;
    ProfScope ps(ctx, cls);
    // ---- tile / split choice -----------------------------------------------------------------
    //  * 128x128x16 (8 waves, 1 workgroup per CU) whenever M and N are multiples of 128, else 64x64x16;
    //  * fewer tiles than CUs: split the K loop over `splits` workgroups per tile (partials in a
    //    workspace, summed + epilogue in splitk_reduce_kernel) so that the whole chip contracts.
    //  force_tile (64 | 128) pins the tile for A/B runs.
    const int KT = g.K / GEMM_BK;
    // `fill`: workgroups per CU the split may create (the 64-tile keeps two workgroups per CU busy)
    auto best_splits = [&](long long tiles, int fill) {
        int sp = 1;
        if (g.batch > 1 || g.batch_offs) return 1;  // the batch dimension already fills the chip
        const long long cap = (long long)fill * ctx->num_cu;
        if (ctx->split_k && tiles < cap)
            while ((long long)sp * 2 * tiles <= cap && KT % (sp * 2) == 0 && KT / (sp * 2) >= 2) sp *= 2;
        if (ctx->force_splits > 0 && KT % ctx->force_splits == 0) sp = ctx->force_splits;
        return sp;
    };
    const bool can128 = (g.M % 128 == 0) && (g.N % 128 == 0) && ctx->force_tile != 64;
    const long long tiles128 = can128 ? (long long)(g.M / 128) * (g.N / 128) : 0;
    const long long tiles64 = (long long)(g.M / 64) * (g.N / 64);
    if (ctx->force_tile == 12864) return fail(ctx, "launch_gemm: force_tile 12864 (the 128 x 64 x 8 tile of round 2's A/B) is no longer built");
    bool t128;
    if (ctx->force_tile == 128 && can128 && uniform_mode != 4) t128 = true;
    else if (ctx->force_tile == 64) t128 = false;
    else if (uniform_mode == 4) t128 = false;  // 3M: three accumulator sets only fit the 32x32 wave tile
    else t128 = can128;  // measured: 128-tile + split-K beats 64-tile without split (n=1024: 49.9 vs 46.4 TF)
    // (tried: 64-tiles with two workgroups per CU for narrow state blocks -- n = 1024: 128 columns 92 vs 99 us,
    //  but n = 4096, 128 columns 41.1 vs 37.1 ms: not a rule)
    int splits = best_splits(t128 ? tiles128 : tiles64, 1);
    // Very small shards of a sweep (the big tile split until every workgroup holds <= 4 K tiles): the partials of a
    // fully split 128 x 128 launch are always 256 tiles x 256 KB = 67 MB and the short K loops pay their pipeline fill
    // nine times per K tile; 64 x 64 tiles with TWO workgroups per CU write a quarter of that and overlap each other's
    // latency.  A/B in one process (tools/bench_tile_choice.py, n = 1024, us per evaluation, big tile vs this rule):
    // 128 instances 96.9 vs 91.5, 256: 171.1 vs 170.0; with 8 K tiles per split the big tile wins (384: 302.5 vs 318.7,
    // 512: 311.0 vs 324.9), so the rule stops at 4.
    if (t128 && !sparse && ctx->force_tile == 0 && ctx->force_splits == 0 && uniform_mode != 4 && splits > 1 &&
        KT / splits <= 4) {
        const int s64 = best_splits(tiles64, 2);
        if (tiles64 * s64 > tiles128 * splits) {
            t128 = false;
            splits = s64;
        }
    }
    if (sparse) {
        // the list of a row panel is shared out by COUNT: one workgroup per CU at most, a share keeps >= 4 tiles
        // (measured on 128-row panels, n = 4096, 112 tiles per panel: 32 panels x 8 splits 87 us, x 16 107 us, x 4 133 us)
        const int t = sparse_tile(ctx, sparse, g.M, g.N);
        const int wide = g.N % 128 == 0 ? 128 : 64;
        const int bm_of[4] = {64, 128, 32, 16}, bn_of[4] = {64, 128, wide, wide};
        g.work_ptr = sparse->gw_ptr[t];
        g.work_idx = sparse->gw_idx[t];
        const long long tiles = (long long)(g.M / bm_of[t]) * (g.N / bn_of[t]);
        splits = 1;
        if (ctx->split_k)
            while ((long long)splits * 2 * tiles <= ctx->num_cu && sparse->gw_avg[t] / (splits * 2) >= 4.0) splits *= 2;
        if (ctx->force_splits > 0) splits = ctx->force_splits;
        CHK(setup_splits(ctx, g, splits, tiles));
        ctx->last_sparse[0] = bm_of[t];
        ctx->last_sparse[1] = bn_of[t];
        ctx->last_sparse[2] = sparse->gw_avg[t] * (g.M / bm_of[t]);
        ctx->last_sparse[3] = splits;
        ctx->last_sparse[4] = 1;
        int sts;
        if (t == 1) sts = launch_gemm_cfg<128, 128, 2, 4, 16>(ctx, g, uniform_mode);
        else if (t == 2 && wide == 128) sts = launch_gemm_lists_cfg<32, 128, 1, 4, 16>(ctx, g, uniform_mode);
        else if (t == 2) sts = launch_gemm_lists_cfg<32, 64, 1, 2, 16>(ctx, g, uniform_mode);
        else if (t == 3 && wide == 128) sts = launch_gemm_lists_cfg<16, 128, 1, 4, 16>(ctx, g, uniform_mode);
        else if (t == 3) sts = launch_gemm_lists_cfg<16, 64, 1, 2, 16>(ctx, g, uniform_mode);
        else sts = launch_gemm_cfg<64, 64, 2, 2, 16>(ctx, g, uniform_mode);
        if (sts) return sts;
        return launch_reduce(ctx, g);
    }
    CHK(setup_splits(ctx, g, splits, t128 ? tiles128 : tiles64));
    if (ctx->profile)    // what this launch executes: per complex MAC and active segment 8 real flops (4M), 6 (3M), 4 (one operator plane)
        ctx->cls_flops[cls] += (double)g.M * g.N * g.K * std::max(g.batch, 1) * g.n_act *
                               (uniform_mode == 4 ? 6.0 : (uniform_mode == 1 || uniform_mode == 2 ? 4.0 : 8.0));
    int st = t128 ? launch_gemm_cfg<128, 128, 2, 4, 16>(ctx, g, uniform_mode)
                  : launch_gemm_cfg<64, 64, 2, 2, 16>(ctx, g, uniform_mode);
    if (st) return st;
    return launch_reduce(ctx, g);
}

// Two independent contractions over the work lists of a block-sparse stack in ONE launch (same stack, same shapes;
// coefficient rows, inputs and epilogues differ).  Tile and split choice as in launch_gemm's sparse branch, with
// twice the workgroups counted against the CUs.
static int launch_gemm_sparse_pair(midyn_ctx* ctx, const GemmArgs& ga, const GemmArgs& gb, int cls, int uniform_mode,
                                   const midyn_stack* sparse) {
    GemmPair gp;
    gp.g[0] = ga;
    gp.g[1] = gb;
    GemmArgs& g = gp.g[0];
    if (g.M % 64 || g.N % 64 || g.K % GEMM_BK || g.n_act > 64 || gb.M != g.M || gb.N != g.N || gb.K != g.K)
        return fail(ctx, "launch_gemm_sparse_pair: unsupported shapes");
    ProfScope ps(ctx, cls);
    const int t = sparse_tile(ctx, sparse, g.M, g.N);
    const int wide = g.N % 128 == 0 ? 128 : 64;
    const int bm_of[4] = {64, 128, 32, 16}, bn_of[4] = {64, 128, wide, wide};
    const long long tiles = (long long)(g.M / bm_of[t]) * (g.N / bn_of[t]);
    int splits = 1;
    if (ctx->split_k)
        while ((long long)splits * 2 * 2 * tiles <= ctx->num_cu && sparse->gw_avg[t] / (splits * 2) >= 4.0) splits *= 2;
    if (ctx->force_splits > 0) splits = ctx->force_splits;
    // one workspace holds the partials of both products
    if (splits > 1) {
        GemmArgs tmp = g;
        tmp.N = 2 * g.N;   // sized for both
        CHK(setup_splits(ctx, tmp, splits));
    }
    for (int i = 0; i < 2; ++i) {
        GemmArgs& q = gp.g[i];
        q.work_ptr = sparse->gw_ptr[t];
        q.work_idx = sparse->gw_idx[t];
        q.ablate = 0;
        q.splits = splits;
        q.sync = nullptr;
        q.sync_err = nullptr;
        q.partial = splits > 1 ? static_cast<double2*>(ctx->splitk_ws) + (size_t)i * splits * g.M * g.N : nullptr;
    }
    ctx->last_sparse[0] = bm_of[t];
    ctx->last_sparse[1] = bn_of[t];
    ctx->last_sparse[2] = sparse->gw_avg[t] * (g.M / bm_of[t]);
    ctx->last_sparse[3] = splits;
    ctx->last_sparse[4] = 2;
    int sts;
    if (t == 1) sts = launch_pair_cfg<128, 128, 2, 4, 16>(ctx, gp, uniform_mode);
    else if (t == 2 && wide == 128) sts = launch_pair_cfg<32, 128, 1, 4, 16>(ctx, gp, uniform_mode);
    else if (t == 2) sts = launch_pair_cfg<32, 64, 1, 2, 16>(ctx, gp, uniform_mode);
    else if (t == 3 && wide == 128) sts = launch_pair_cfg<16, 128, 1, 4, 16>(ctx, gp, uniform_mode);
    else if (t == 3) sts = launch_pair_cfg<16, 64, 1, 2, 16>(ctx, gp, uniform_mode);
    else sts = launch_pair_cfg<64, 64, 2, 2, 16>(ctx, gp, uniform_mode);
    if (sts) return sts;
    CHK(launch_reduce(ctx, gp.g[0]));
    return launch_reduce(ctx, gp.g[1]);
}

// The batched RHS contraction on the planar single-plane kernel (two operator tiles per barrier).
static int launch_gemm_plane(midyn_ctx* ctx, const GemmArgs& g_in, const double* planes, long long seg_stride) {
    GemmArgs g = g_in;
    g.ablate = 0;
    g.splits = 1;
    g.partial = nullptr;
    if (g.M % 128 || g.N % 128 || g.K % GEMM_BK || g.n_act > 64 || g.n_act < 1)
        return fail(ctx, "launch_gemm_plane: unsupported shape");
    ProfScope ps(ctx, KC_RHS_GEMM);
    const long long tiles = (long long)(g.M / 128) * (g.N / 128);
    const int KT = g.K / GEMM_BK;
    int splits = 1;
    if (ctx->split_k && tiles < ctx->num_cu)
        while ((long long)splits * 2 * tiles <= ctx->num_cu && KT % (splits * 2) == 0 && KT / (splits * 2) >= 2) splits *= 2;
    if (ctx->force_splits > 0 && KT % ctx->force_splits == 0) splits = ctx->force_splits;
    CHK(setup_splits(ctx, g, splits));
    constexpr size_t SMEM = (size_t)2 * 2 * 128 * 16 * sizeof(double) + (size_t)2 * 16 * 128 * sizeof(double2);
    static DeviceOnce attr_set;
    auto kern = zgemm_plane_kernel<2, 4>;
    if (attr_set.needed(ctx->device)) {
        HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)SMEM));
        attr_set.done(ctx->device);
    }
    PlaneArgs pa{};
    pa.planes = planes;
    pa.seg_stride = seg_stride;
    pa.g = g;
    hipLaunchKernelGGL(kern, dim3((unsigned)(tiles * splits)), dim3(512), SMEM, ctx->stream, pa);
    HIPCHK(ctx, hipGetLastError());
    return launch_reduce(ctx, g);
}

static int launch_stream(midyn_ctx* ctx, const StreamArgs& a, const double* planes = nullptr) {
    ProfScope ps(ctx, KC_STREAM);
    if (planes) {  // single-plane stack: stream only the non-zero planes (half the bytes)
        if (a.n_pad >= 1024) {
            switch (ctx->stream_variant) {
                case 1: hipLaunchKernelGGL((rhs_stream_plane_kernel<2, 1>), dim3(a.n_pad), dim3(256), 0, ctx->stream, a, planes); break;
                case 2: hipLaunchKernelGGL((rhs_stream_plane_kernel<1, 3>), dim3(a.n_pad), dim3(256), 0, ctx->stream, a, planes); break;
                case 3: hipLaunchKernelGGL((rhs_stream_plane_kernel<2, 9>), dim3(a.n_pad), dim3(256), 0, ctx->stream, a, planes); break;
                case 4: hipLaunchKernelGGL((rhs_stream_plane_kernel<1, 9>), dim3(a.n_pad), dim3(256), 0, ctx->stream, a, planes); break;
                default: hipLaunchKernelGGL((rhs_stream_plane_kernel<2, 3>), dim3(a.n_pad), dim3(256), 0, ctx->stream, a, planes); break;
            }
        } else {
            hipLaunchKernelGGL((rhs_stream_plane_kernel<1, 1>), dim3(a.n_pad), dim3(256), 0, ctx->stream, a, planes);
        }
        HIPCHK(ctx, hipGetLastError());
        return 0;
    }
    if (a.n_pad >= 1024) {
        switch (ctx->stream_variant) {
            case 1: hipLaunchKernelGGL((rhs_stream_kernel<4, 1>), dim3(a.n_pad), dim3(256), 0, ctx->stream, a); break;
            case 2: hipLaunchKernelGGL((rhs_stream_kernel<2, 3>), dim3(a.n_pad), dim3(256), 0, ctx->stream, a); break;
            case 3: hipLaunchKernelGGL((rhs_stream_kernel<4, 9>), dim3(a.n_pad), dim3(256), 0, ctx->stream, a); break;
            case 4: hipLaunchKernelGGL((rhs_stream_kernel<2, 9>), dim3(a.n_pad), dim3(256), 0, ctx->stream, a); break;
            default: hipLaunchKernelGGL((rhs_stream_kernel<4, 3>), dim3(a.n_pad), dim3(256), 0, ctx->stream, a); break;
        }
    } else {
        hipLaunchKernelGGL((rhs_stream_kernel<1, 1>), dim3(a.n_pad), dim3(256), 0, ctx->stream, a);
    }
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

static int launch_stream_multi(midyn_ctx* ctx, const StreamArgs& a, int ncol, int m_cols, long long inst_stride,
                               const double* planes = nullptr) {
    ProfScope ps(ctx, KC_STREAM);
    const dim3 grid(a.n_pad), block(256);
    if (planes) {  // single-plane stack: stream only the non-zero planes
#define MIDYN_MULTI_P(C_)                                                                                       \
    if (a.n_pad >= 1024)                                                                                        \
        hipLaunchKernelGGL((rhs_stream_multi_plane_kernel<C_, 2>), grid, block, 0, ctx->stream, a, planes, ncol, m_cols, \
                           inst_stride);                                                                        \
    else                                                                                                        \
        hipLaunchKernelGGL((rhs_stream_multi_plane_kernel<C_, 1>), grid, block, 0, ctx->stream, a, planes, ncol, m_cols, \
                           inst_stride)
        if (ncol <= 2) { MIDYN_MULTI_P(2); }
        else if (ncol <= 4) { MIDYN_MULTI_P(4); }
        else { MIDYN_MULTI_P(8); }
#undef MIDYN_MULTI_P
        HIPCHK(ctx, hipGetLastError());
        return 0;
    }
#define MIDYN_MULTI(C_)                                                                                        \
    if (a.n_pad >= 512)                                                                                        \
        hipLaunchKernelGGL((rhs_stream_multi_kernel<C_, 2>), grid, block, 0, ctx->stream, a, ncol, m_cols, inst_stride); \
    else                                                                                                       \
        hipLaunchKernelGGL((rhs_stream_multi_kernel<C_, 1>), grid, block, 0, ctx->stream, a, ncol, m_cols, inst_stride)
    if (ncol <= 2) { MIDYN_MULTI(2); }
    else if (ncol <= 4) { MIDYN_MULTI(4); }
    else { MIDYN_MULTI(8); }
#undef MIDYN_MULTI
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

// block-sparse stack, 1..8 columns: only the listed 16 x 16 operator blocks are read
static int launch_blocks(midyn_ctx* ctx, const StreamArgs& a, const midyn_stack* s, int ncol, int m_cols,
                         long long inst_stride) {
    ProfScope ps(ctx, KC_BLOCKS);
    const dim3 grid(a.n_pad / 16), block(256);
#define MIDYN_BLOCKS(C_) \
    hipLaunchKernelGGL((rhs_blocks_kernel<C_>), grid, block, 0, ctx->stream, a, s->blk_ptr, s->blk_idx, ncol, m_cols, inst_stride)
    if (ncol <= 1) { MIDYN_BLOCKS(1); }
    else if (ncol <= 2) { MIDYN_BLOCKS(2); }
    else if (ncol <= 4) { MIDYN_BLOCKS(4); }
    else { MIDYN_BLOCKS(8); }
#undef MIDYN_BLOCKS
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

// plain zgemm on device buffers: C = alpha * A.B + beta * Z; `batch` independent problems whose
// operands are `sa`, `sb`, `sc` elements apart (C and Z share the stride)
static int dev_zgemm_batched(midyn_ctx* ctx, int batch, int M, int N, int K, const double2* A, int lda, long long sa,
                             const double2* B, int ldb, long long sb, double2* C, int ldc, long long sc, double alpha,
                             double beta, const double2* Z, const long long* d_offs = nullptr,
                             bool a_real_only = false) {
    GemmArgs g{};
    g.batch_offs = d_offs;
    g.A = A;
    g.a_seg_stride = 0;
    g.lda = lda;
    g.B = B;
    g.ldb = ldb;
    g.M = M;
    g.N = N;
    g.K = K;
    g.seg_list = ctx->d_one_seg;
    g.n_act = 1;
    g.has_static = 0;
    g.coeff = nullptr;
    g.inst_stride = 0;
    g.m_cols = 1;
    g.n_inst = N;
    g.batch = batch;
    g.batch_a = sa;
    g.batch_b = sb;
    g.batch_c = sc;
    g.epi.mode = EPI_PLAIN;
    g.epi.ld = ldc;
    g.epi.alpha = alpha;
    g.epi.beta = beta;
    g.epi.out = C;
    g.epi.z = Z;
    if (a_real_only) {  // Im A == 0 exactly: the two real MFMAs that would multiply it are skipped
        g.seg_list = ctx->d_one_seg + 1;
        return launch_gemm(ctx, g, KC_ZGEMM, 1);
    }
    return launch_gemm(ctx, g, KC_ZGEMM);
}

static int dev_zgemm(midyn_ctx* ctx, int M, int N, int K, const double2* A, int lda, const double2* B,
                     int ldb, double2* C, int ldc, double alpha, double beta, const double2* Z) {
    return dev_zgemm_batched(ctx, 1, M, N, K, A, lda, 0, B, ldb, 0, C, ldc, 0, alpha, beta, Z);
}

// square [np][np] matrices laid out back to back
static int dev_sqgemm(midyn_ctx* ctx, int batch, int np, const double2* A, const double2* B, double2* C, double alpha,
                      double beta, const double2* Z) {
    const long long st = (long long)np * np;
    return dev_zgemm_batched(ctx, batch, np, np, np, A, np, st, B, np, st, C, np, st, alpha, beta, Z);
}

static int dev_lincomb(midyn_ctx* ctx, int n, double2* out, int nterms, const double2* const* xs,
                       const double* alphas, double gamma, int batch = 1) {
    LinArgs a{};
    a.nterms = nterms;
    for (int i = 0; i < nterms; ++i) {
        a.x[i] = xs[i];
        a.alpha[i] = alphas[i];
    }
    a.gamma = gamma;
    a.n = n;
    a.batch = batch;
    a.out = out;
    ProfScope ps(ctx, KC_ELEM);
    hipLaunchKernelGGL(lincomb_kernel, dim3(grid_for((size_t)n * n * batch)), dim3(256), 0, ctx->stream, a);
    HIPCHK(ctx, hipGetLastError());
    return 0;
}

// simple device buffer holder
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;      // requested size
    size_t cap = 0;        // capacity of the block (>= bytes)
    midyn_ctx* owner = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (!p) return;
        if (owner && cap <= midyn_ctx::POOL_MAX_BLOCK) {
            // a full cache gives up its OLDEST blocks for this one: after a large solve the cache is full of blocks no smaller solve
            // fits (a block serves requests down to half its size), and refusing the new, smaller blocks meant a hipMalloc and a
            // hipFree for every buffer of every following solve (cfg 5: the 128-instance shard after the 1024-instance run, +0.3 ms)
            while (!owner->mem_pool.empty() && owner->mem_pool_bytes + cap > midyn_ctx::POOL_MAX_BYTES) {
                hipFree(owner->mem_pool.front().second);
                owner->mem_pool_bytes -= owner->mem_pool.front().first;
                owner->mem_pool.erase(owner->mem_pool.begin());
            }
            owner->mem_pool.emplace_back(cap, p);
            owner->mem_pool_bytes += cap;
        } else {
            hipFree(p);
        }
        p = nullptr;
        bytes = cap = 0;
    }
    int alloc(midyn_ctx* ctx, size_t b) {
        release();
        bytes = b;
        owner = ctx;
        if (b == 0) return 0;
        const size_t want = (b + 4095) / 4096 * 4096;
        // best fit among cached blocks of capacity in [want, 2 want]
        int best = -1;
        for (int i = 0; i < (int)ctx->mem_pool.size(); ++i) {
            const size_t c = ctx->mem_pool[i].first;
            if (c >= want && c <= 2 * want && (best < 0 || c < ctx->mem_pool[best].first)) best = i;
        }
        if (best >= 0) {
            // a recycled block may still be read by kernels queued before it was released, and the
            // caller may fill it with a host-synchronous (null-stream) copy: drain the stream first
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            cap = ctx->mem_pool[best].first;
            p = ctx->mem_pool[best].second;
            ctx->mem_pool_bytes -= cap;
            ctx->mem_pool.erase(ctx->mem_pool.begin() + best);
            return 0;
        }
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess && !ctx->mem_pool.empty()) {  // out of memory: give the cache back and retry
            (void)hipGetLastError();
            for (auto& blk : ctx->mem_pool) hipFree(blk.second);
            ctx->mem_pool.clear();
            ctx->mem_pool_bytes = 0;
            e = hipMalloc(&p, want);
        }
        if (e != hipSuccess) {
            p = nullptr;
            bytes = 0;
            return fail(ctx, std::string("hipMalloc: ") + hipGetErrorString(e));
        }
        cap = want;
        return 0;
    }
    // alloc + a synchronous copy of a host table (complete on return)
    template <class T>
    int upload(midyn_ctx* ctx, const std::vector<T>& v) {
        CHK(alloc(ctx, v.size() * sizeof(T)));
        HIPCHK(ctx, hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        return 0;
    }
    template <class T>
    T* as() { return static_cast<T*>(p); }
};

// Copy `bytes` from a host OR device pointer into device memory, ordered on the ctx stream and
// complete on return.  (A plain hipMemcpy from a DEVICE source may return before the copy has
// run, and it runs on the null stream, which the non-blocking ctx stream does not wait for: kernels
// launched next would read a half-filled table.)
static hipError_t copy_to_device_any(midyn_ctx* ctx, void* dst, const void* src, size_t bytes) {
    hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDefault, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    return e;
}

// 1-norms of `batch` [np][np] matrices stored back to back (one small D2H copy + stream sync)
// mode 0: 1-norms; 1: infinity norms; 2: 1-norms of the Hermitian parts (A + A^dagger) / 2
static int dev_norm1(midyn_ctx* ctx, const double2* A, int np, int batch, DevBuf& scratch, std::vector<double>& norms,
                     int mode = 0) {
    const int nchunk = std::max(1, std::min(32, np / 128));
    const size_t cnt = (size_t)batch * nchunk * np;
    if (scratch.bytes < cnt * sizeof(double)) CHK(scratch.alloc(ctx, cnt * sizeof(double)));
    if (mode == 0)
        hipLaunchKernelGGL(colsum_kernel, dim3((np + 255) / 256, batch, nchunk), dim3(256), 0, ctx->stream, A, np, nchunk,
                           scratch.as<double>());
    else
        hipLaunchKernelGGL(colsum_mode_kernel, dim3((np + 255) / 256, batch, nchunk), dim3(256), 0, ctx->stream, A, np,
                           nchunk, mode, scratch.as<double>());
    HIPCHK(ctx, hipGetLastError());
    std::vector<double> h_pageable;
    double* h = ctx->h_pinned;
    if (cnt > midyn_ctx::PINNED_DOUBLES) {
        h_pageable.resize(cnt);
        h = h_pageable.data();
    }
    HIPCHK(ctx, hipMemcpyAsync(h, scratch.p, cnt * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    norms.assign(batch, 0.0);
    for (int b = 0; b < batch; ++b)
        for (int c = 0; c < np; ++c) {
            double sum = 0.0;
            for (int z = 0; z < nchunk; ++z) sum += h[((size_t)b * nchunk + z) * np + c];
            norms[b] = std::max(norms[b], sum);
        }
    return 0;
}
