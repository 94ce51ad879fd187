// midyn_core.inc -- part of midyn.hip (one translation unit; included in order): context, options, counters, device-memory pool, operator stack (create / adopt / destroy), block occupancy lists
// -------------------------------------------------------------------------------------------------
// context, errors, profiling
// -------------------------------------------------------------------------------------------------
static thread_local std::string g_last_error;

enum KClass { KC_STREAM = 0, KC_RHS_GEMM, KC_ZGEMM, KC_GEN, KC_ELEM, KC_BLOCKS, KC_BLOCKS_GEMM, KC_RESIDENT, KC_COMBINE, KC_GEN_CHAIN, KC_MIRROR_FINISH, KC_SPMV, KC_COUNT };
static const char* kclass_names[KC_COUNT] = {"rhs_stream", "rhs_gemm", "zgemm", "gen_eval", "elementwise",
                                             "rhs_blocks", "rhs_blocks_gemm",   // block-sparse routes
                                             "rk4_resident",   // whole step ranges of one trajectory in one launch
                                             "rhs_combine",   // sweeps: combine (MFMA over the operator planes) + apply (midyn_combine.h)
                                             "gen_chain",     // callable generators: a chunk of step propagators applied in one launch (midyn_gentable.inc)
                                             "mirror_finish",   // mirrored combine: sum of the U-row partials + their epilogue (midyn_combine_mirror.h)
                                             "rhs_spmv"};       // sparse operators: the stage launches of the gather kernels (midyn_spmv.h)

struct EventPair {
    hipEvent_t a, b;
    int cls;
};

struct midyn_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    bool skip_zero_planes = true;
    int chebyshev = 1;             // expm action, Magnus order 1, nearly skew-Hermitian generator: Chebyshev series
                                   // instead of the scaled Taylor series (1: when shorter, 2: always, 0: never)
    int sparse_bm = 0;             // A/B: pin the row panels of the sparse MFMA route (16 | 32 | 64 | 128; 0 = by list density)
    bool skip_zero_blocks = true;  // block-sparse stacks: contract only the 16 x 16 operator blocks that hold a non-zero
    bool profile = false;
    int force_tile = 0;  // 0 auto, 64, 128
    bool prefer_duo = false;
    int ablate = 0;
    int stream_variant = 0;
    int expm_degree = 0;         // 0: Taylor degree chosen from the norm; else forced (2,4,6,9,12,16)
    int krylov = 1;              // one column, Magnus order 1: Arnoldi instead of the scaled Taylor series
                                 // (1: when the series is long enough to pay for it, 2: always, 0: never)
    bool expm_action = true;     // few state columns: y <- expm(Omega) y as a Taylor series of matrix-vector
                                 // products instead of forming expm(Omega) (Magnus orders 1 and 2)
    bool stream_planes = true;   // single-plane stacks: the one-column kernel streams only non-zero planes
    bool tiny_rk4 = true;        // small systems: whole RK4 solve in one persistent launch (tiny_rk4_kernel)
    bool resident_rk4 = true;    // one trajectory, operators fit the register files: rk4_resident_kernel (midyn_resident.h)
    bool ell_sweep = true;       // sweeps on very sparse stacks, expm action: one workgroup per instance (ell_sweep_kernel)
    int ell_sweep_split = 1;     // ... small shards of stacks WITHOUT a packed element form: 1 = 4 workgroups per instance when 4 B <= CUs,
                                 // 2 = also 2 workgroups (slower), 3 = like 2, packed stacks too, 0 = never
    int expansion_pack = 1;    // midyn_expansion_solve, n <= 32: two step matrices per padded 64 x 64 block (midyn_expansion.inc); 0: one
    int last_expansion_pack = 0;   // (steps per padded matrix of the last midyn_expansion_solve: counter "expansion_pack")
    int expm_plan_cache = 1;   // one-shot midyn_expm_solve on the sweep route keeps its plan in the stack (midyn_sweep_plan.inc); 0: made and destroyed per call
    int gentable_chain = 1;    // midyn_gentable, sequential route, n_pad <= 128 and m <= 32: gen_chain_kernel (one launch per chunk); 0: a zgemm per step
    int gentable_chunk = 0;    // midyn_gentable: > 0 caps the steps per chunk
    int spmv_lanes = 0;        // midyn_spmv: lane mapping of the gather kernels: 1 = (row, column) pairs, 2 = 64 state columns of one row, 0 = by the column count
    double last_gentable[4] = {0, 0, 0, 0};   // last midyn_gentable solve: chunks, steps in the largest chunk, pinned staging bytes, device raw-row bytes
    int last_plan_cache = 0;   // (1: the last one-shot sweep solve found its plan in the stack; counter "expm_plan_cache")
    unsigned long long options_epoch = 1;      // counts midyn_ctx_set_option calls: cached plans are tied to the options they were made under
    int exchange_protocol = 0; // hand-offs between workgroups inside the one-launch kernels: 0 = the measured default (relaxed agent-scope
                               // atomics on data-is-flag words behind s_waitcnt; two-workgroup sweep kernels keep their payload in the L2 the
                               // partners share), 1 = the forms MI355X_MICROARCH.md lists as conforming: RELEASE publishes / ACQUIRE polls
                               // in rk4_resident_kernel / ell_resident_kernel, sc1 stores AND sc1 loads + agent-scope flags in the
                               // two-workgroup kernels on one XCD too (profiles/r06_exchange_protocol.md)
    int expm_direct_out = 1;   // midyn_expm_plan_run / midyn_expm_solve on the sweep route: the kernel writes the saved states straight into the
                               // caller's result block when that is device-writable host memory (pinned); 0: device block + copy
    int cheb_tail = 1;       // Chebyshev series of the expm action: 1 = ends where the dropped terms sum to less than 2^-53 (unit roundoff,
                             // the Taylor schemes' and scipy's standard); 0 = the rule of rounds 2-5, every |J_k| >= 1e-18 kept
    int ell_sweep_flip = 1;  // ... and, when every slot of the stack also has one flip mask (column = row ^ flip: Pauli strings without
                                 // Z factors), the kernel without operator elements (ell_flip_duo_kernel, midyn_flip.h); 0: ell_sweep_duo_kernel
    int ell_sweep_duo = 1;   // ... small shards (2 B <= CUs) of stacks WITH a packed element form: two workgroups per instance,
                                 // the exchange hidden behind the slots that stay inside a half (ell_sweep_duo_kernel)
    bool ell_sweep_packed = true;   // use the packed element forms of a stack (4-byte elements) when it has one
    bool resident_exchange_only = false;       // measurement only: rk4_resident_kernel skips its arithmetic (results wrong)
    unsigned resident_spin_limit = 1u << 21;   // polls a wait inside a one-launch kernel may take before it gives up
    long long resident_fallbacks = 0;          // step ranges re-run on the per-launch route after such a wait gave up
    int combine = 1;             // sweeps (many instances with their own coefficients): COMBINE + APPLY kernel instead of k + 1 GEMMs
                                 // (1: where it is the faster formulation, 2: wherever it applies, 0: never)
    int combine_min_cols = 256;  // ... from this many state columns on
    int combine_mirror = 1;      // ... on stacks that only couple the two row halves, with symmetric / antisymmetric planes: each combined block
                                 // formed once and applied twice (combine_mirror_kernel; 1: the RK4 / rhs route of sweeps with at least two
                                 // mirror waves per SIMD, 2: wherever the stack is eligible, 0: never)
    double last_mirror[2] = {0, 0};   // (1 if the last combine launch was mirrored, the stack's mirror defect in units of epsilon)
    int combine_ablate = 0;      // profiling only (results wrong): 1 = rhs_combine_kernel stores its result and nothing else (no fused RK4 /
                                 // series stage: none of the epilogue's reads, one of its two writes) -- what the epilogue of a launch costs
    int mirror_ablate = 0;       // profiling only (results wrong): mirror_probe_kernel<N> in place of combine_mirror_kernel<0, 2> -- 1 = no global
                                 // loads in the kk loop (the first step's operands every step), 2 = no phase behind the block barrier (no
                                 // cross-wave sum, no store of the partial sums), 3 = both
    int combine_occupancy = 2;   // waves per SIMD the workgroup shape of a small sweep aims at (list splits up to 8); 1: one wave, splits up to 4
    int combine_sweep = 1;       // RK4 sweeps of small dense systems (n_pad <= 256): the whole solve in one launch, 16 instances per
                                 // workgroup (midyn_combine_sweep.h); 1: where it is faster than a launch per stage, 2: wherever it
                                 // applies, 0: never
    double last_combine_sweep[3] = {0, 0, 0};      // last such launch: workgroups, waves per workgroup, row tiles per wave
    double last_combine[7] = {0, 0, 0, 0, 0, 0, 0};   // last launch: listed entries, plane groups (re, im), static planes, (row group, column block) pairs per workgroup, list splits, instances per wave
    bool multi_stream = true;    // 2..8 state columns at n >= 256: multi-column streaming kernel
    bool split_k = true;
    bool combine_first = true;
    bool plane_kernel = false;  // planar two-tiles-per-barrier variant: measured 4 % SLOWER (2.43 vs 2.33 ms), kept opt-in
    // dense complex products by the 3M scheme (3 real MFMAs instead of 4; normwise error bound): 0 never,
    // 1 inside the solver loops and the expm pipeline but NOT for direct evaluations (midyn_eval_rhs,
    // midyn_zgemm: those keep the componentwise accuracy of a BLAS zgemm, which the reference calls), 2 everywhere
    int complex_3m = 1;
    bool direct_eval = false;  // set by the direct-evaluation entry points around their launches
    int force_splits = 0;
    bool pair_launch = true;       // sparse MFMA route: the two independent products of a Magnus-2 level share one launch
    // split-K partials summed and finished inside the contraction launch (siblings wait on per-tile counters) instead of
    // by splitk_reduce_kernel.  Measured SLOWER (B = 512: 339 vs 309 us per evaluation, 64: 66.5 vs 57.7; with full
    // release/acquire fences instead of write-through stores 433 us): the wait for the slowest sibling and the
    // write-through stores cost more than the ~2 us kernel boundary they remove.  Opt-in, bit-identical results.
    bool splitk_inlaunch = false;
    int* d_sync = nullptr;         // per-tile {arrived, departed} counters of the in-launch reduction (zero between launches)
    int* h_sync_err = nullptr;     // host-mapped error word of that wait (device pointer: d_sync_err)
    int* d_sync_err = nullptr;
    static constexpr int SYNC_TILES = 1024;
    void* splitk_ws = nullptr;
    size_t splitk_bytes = 0;
    std::vector<EventPair> pending;
    std::vector<hipEvent_t> pool;
    double cls_ms[KC_COUNT] = {0};
    double cls_n[KC_COUNT] = {0};
    double cls_flops[KC_COUNT] = {0};   // real flops the DENSE contraction launches of a class execute (counter "flops:<class>"; profile on)
    int* d_one_seg = nullptr;  // device int {0, 1}: single-segment lists for plain zgemm (dense A / real-only A)
    // device-memory pool: DevBuf blocks are recycled instead of hipMalloc/hipFree'd (a small solve is a
    // few hundred microseconds of kernels; a dozen allocations per call used to cost milliseconds)
    std::vector<std::pair<size_t, void*>> mem_pool;  // (capacity, block)
    size_t mem_pool_bytes = 0;
    static constexpr size_t POOL_MAX_BYTES = (size_t)2 << 30, POOL_MAX_BLOCK = (size_t)256 << 20;
    double* h_pinned = nullptr;                  // pinned host scratch for small device-to-host results (norms)
    static constexpr size_t PINNED_DOUBLES = 1 << 17;
    int num_cu = 256;
    size_t lds_per_block = 160 * 1024;      // opt-in dynamic LDS a workgroup may declare (hipDeviceProp_t.sharedMemPerBlockOptin; gfx950: 160 KiB)
    hipEvent_t timer_ev[2] = {nullptr, nullptr};  // midyn_ctx_timer
    // the last launch of the sparse MFMA route: tile, listed tiles of the whole stack, split count (reports)
    double last_sparse[5] = {0, 0, 0, 0, 1};   // [4]: contractions in that launch (2 for a paired launch)
    double last_sweep[5] = {0, 0, 1, 0, 0};         // last ell_sweep_kernel launch: series terms per instance over all steps, slots per row, workgroups per instance
};

static int fail(midyn_ctx* ctx, const std::string& msg) {
    g_last_error = msg;
    if (ctx) ctx->err = msg;
    return 1;
}

// Which instantiation of a kernel family a solve picked: with MIDYN_VARIANT_LOG=<file> in the environment the first selection of
// every (family, template arguments) in the process appends one line to that file (tools/variant_census.sh runs the GPU suite
// and the fuzzers under it; instantiations nothing ever selects are candidates for removal).  Off: one relaxed load.
static void note_variant(const char* family, std::initializer_list<int> targs) {
    static const char* path = getenv("MIDYN_VARIANT_LOG");
    if (!path) return;
    static std::mutex mu;
    static std::set<std::string> seen;
    std::string key = family;
    key += "<";
    bool first = true;
    for (int v : targs) {
        if (!first) key += ", ";
        key += std::to_string(v);
        first = false;
    }
    key += ">";
    std::lock_guard<std::mutex> lock(mu);
    if (!seen.insert(key).second) return;
    if (FILE* f = fopen(path, "a")) {
        fprintf(f, "%s\n", key.c_str());
        fclose(f);
    }
}

#define HIPCHK(ctx, expr)                                                                   \
    do {                                                                                    \
        hipError_t _e = (expr);                                                             \
        if (_e != hipSuccess)                                                               \
            return fail((ctx), std::string(#expr) + ": " + hipGetErrorString(_e) + " at " + \
                                   __FILE__ + ":" + std::to_string(__LINE__));              \
    } while (0)

#define CHK(expr)                  \
    do {                           \
        int _s = (expr);           \
        if (_s != 0) return _s;    \
    } while (0)

struct ProfScope {
    midyn_ctx* ctx;
    EventPair ep;
    bool on;
    ProfScope(midyn_ctx* c, int cls) : ctx(c), on(c->profile) {
        if (!on) return;
        auto get = [&]() {
            hipEvent_t e;
            if (!ctx->pool.empty()) {
                e = ctx->pool.back();
                ctx->pool.pop_back();
            } else {
                hipEventCreate(&e);
            }
            return e;
        };
        ep.a = get();
        ep.b = get();
        ep.cls = cls;
        hipEventRecord(ep.a, ctx->stream);
    }
    ~ProfScope() {
        if (!on) return;
        hipEventRecord(ep.b, ctx->stream);
        ctx->pending.push_back(ep);
    }
};

static void drain_events(midyn_ctx* ctx) {
    if (ctx->pending.empty()) return;
    hipStreamSynchronize(ctx->stream);
    for (auto& ep : ctx->pending) {
        float ms = 0.f;
        hipEventElapsedTime(&ms, ep.a, ep.b);
        ctx->cls_ms[ep.cls] += ms;
        ctx->cls_n[ep.cls] += 1;
        ctx->pool.push_back(ep.a);
        ctx->pool.push_back(ep.b);
    }
    ctx->pending.clear();
}

extern "C" const char* midyn_last_error(midyn_ctx* ctx) {
    return ctx ? ctx->err.c_str() : g_last_error.c_str();
}

extern "C" int midyn_ctx_create(int device, midyn_ctx** out) {
    if (!out) return fail(nullptr, "midyn_ctx_create: out is NULL");
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0)
        return fail(nullptr, std::string("midyn_ctx_create: no HIP device available (") +
                                 hipGetErrorString(e) + "); libmidyn has no CPU fallback");
    if (device < 0 || device >= count)
        return fail(nullptr, "midyn_ctx_create: device index out of range");
    midyn_ctx* ctx = new midyn_ctx();
    ctx->device = device;
    HIPCHK(ctx, hipSetDevice(device));
    HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    hipDeviceProp_t prop;
    HIPCHK(ctx, hipGetDeviceProperties(&prop, device));
    ctx->num_cu = prop.multiProcessorCount;
    ctx->lds_per_block = std::max<size_t>(prop.sharedMemPerBlockOptin, prop.sharedMemPerBlock);
    if (getenv("MIDYN_VERBOSE")) fprintf(stderr, "[midyn] device %d: %s, %d CUs, LDS per workgroup %zu (opt-in %zu)\n", device, prop.gcnArchName,
                                         prop.multiProcessorCount, (size_t)prop.sharedMemPerBlock, (size_t)prop.sharedMemPerBlockOptin);
    if (const char* e = getenv("MIDYN_COMPLEX_3M")) ctx->complex_3m = atoi(e);
    HIPCHK(ctx, hipHostMalloc((void**)&ctx->h_pinned, midyn_ctx::PINNED_DOUBLES * sizeof(double), hipHostMallocDefault));
    HIPCHK(ctx, hipMalloc(&ctx->d_one_seg, 2 * sizeof(int)));
    int one_seg[2] = {0, 1};  // [0]: segment 0, dense complex A;  [1]: segment 0, A real-only (mode 1)
    HIPCHK(ctx, hipMemcpy(ctx->d_one_seg, one_seg, sizeof(one_seg), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMalloc(&ctx->d_sync, 2 * midyn_ctx::SYNC_TILES * sizeof(int)));
    HIPCHK(ctx, hipMemset(ctx->d_sync, 0, 2 * midyn_ctx::SYNC_TILES * sizeof(int)));
    HIPCHK(ctx, hipHostMalloc((void**)&ctx->h_sync_err, sizeof(int), hipHostMallocMapped));
    *ctx->h_sync_err = 0;
    HIPCHK(ctx, hipHostGetDevicePointer((void**)&ctx->d_sync_err, ctx->h_sync_err, 0));
    *out = ctx;
    return 0;
}

extern "C" int midyn_ctx_destroy(midyn_ctx* ctx) {
    if (!ctx) return 0;
    hipSetDevice(ctx->device);
    drain_events(ctx);
    for (auto e : ctx->pool) hipEventDestroy(e);
    for (auto e : ctx->timer_ev) if (e) hipEventDestroy(e);
    if (ctx->d_one_seg) hipFree(ctx->d_one_seg);
    if (ctx->d_sync) hipFree(ctx->d_sync);
    if (ctx->h_sync_err) hipHostFree(ctx->h_sync_err);
    if (ctx->h_pinned) hipHostFree(ctx->h_pinned);
    for (auto& blk : ctx->mem_pool) hipFree(blk.second);
    ctx->mem_pool.clear();
    if (ctx->splitk_ws) hipFree(ctx->splitk_ws);
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;
    return 0;
}

// Once-per-(kernel, device) set-up such as hipFuncSetAttribute(MaxDynamicSharedMemorySize): a bit per device in an atomic
// mask that every call site keeps in a function-local static.  The bit is set AFTER the set-up ran, so two host threads
// may both run it (harmless) but none launches before it; devices beyond the mask always run it.
struct DeviceOnce {
    std::atomic<unsigned long long> mask{0};
    bool needed(int device) const { return device < 0 || device >= 64 || !(mask.load(std::memory_order_acquire) & (1ull << device)); }
    void done(int device) { if (device >= 0 && device < 64) mask.fetch_or(1ull << device, std::memory_order_release); }
};

// In-kernel waits (split-K in-launch reduction, the exchange rings of the one-launch kernels) give up after a spin limit
// and set a host-mapped word instead of hanging the GPU: 1 = split-K, 2 = a one-launch kernel.  Call after a stream sync.
// take_wait_error: read and clear the word (the one-launch routes re-run their step range on the per-launch route:
// the reference never fails a solve for scheduling reasons).
// Only code 2 is taken: a pending split-K give-up (code 1) stays in the word for check_wait_error to report.
static int take_wait_error(midyn_ctx* ctx) {
    if (!ctx->h_sync_err) return 0;
    const int which = *ctx->h_sync_err;
    if (which != 2) return 0;
    *ctx->h_sync_err = 0;
    return which;
}

static int check_wait_error(midyn_ctx* ctx) {
    if (ctx->h_sync_err && *ctx->h_sync_err) {
        const int which = *ctx->h_sync_err;
        *ctx->h_sync_err = 0;
        if (which == 2)
            return fail(ctx, "rk4_resident_kernel: a workgroup gave up waiting for the stage input of its neighbours "
                             "(results invalid); set option resident_rk4=0");
        return fail(ctx, "split-K in-launch reduction: a workgroup gave up waiting for its siblings (results invalid); "
                         "set option splitk_inlaunch=0");
    }
    return 0;
}

extern "C" int midyn_ctx_synchronize(midyn_ctx* ctx) {
    if (!ctx) return fail(nullptr, "NULL ctx");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return check_wait_error(ctx);
}

// Options that are plain fields of the context: X(name) -- the field has the option's name.  Switches (any non-zero value
// means on) and integers; the few options with a side condition are spelled out in the two functions below.
#define MIDYN_SWITCH_OPTIONS(X)                                                                                          \
    X(skip_zero_planes) X(skip_zero_blocks) X(prefer_duo) X(stream_planes) X(tiny_rk4) X(resident_rk4) X(ell_sweep)      \
    X(ell_sweep_packed) X(multi_stream) X(expm_action) X(split_k) X(combine_first) X(plane_kernel) X(pair_launch)        \
    X(splitk_inlaunch)
#define MIDYN_INT_OPTIONS(X)                                                                                             \
    X(ell_sweep_duo) X(ell_sweep_flip) X(sparse_bm) X(chebyshev) X(force_tile) X(ablate) X(stream_variant) X(ell_sweep_split) X(combine) X(combine_mirror) X(combine_occupancy) X(combine_ablate) X(mirror_ablate) \
    X(combine_sweep) X(expm_degree) X(krylov) X(force_splits) X(complex_3m) X(cheb_tail) X(expm_direct_out) X(exchange_protocol) X(expansion_pack) X(expm_plan_cache) \
    X(gentable_chain) X(gentable_chunk) X(spmv_lanes)

extern "C" int midyn_ctx_set_option(midyn_ctx* ctx, const char* name, long long value) {
    if (!ctx || !name) return fail(ctx, "midyn_ctx_set_option: NULL argument");
    std::string n(name);
    ++ctx->options_epoch;
#define MIDYN_X(opt_) if (n == #opt_) { ctx->opt_ = value != 0; return 0; }
    MIDYN_SWITCH_OPTIONS(MIDYN_X)
#undef MIDYN_X
#define MIDYN_X(opt_) if (n == #opt_) { ctx->opt_ = (decltype(ctx->opt_))value; return 0; }
    MIDYN_INT_OPTIONS(MIDYN_X)
#undef MIDYN_X
    if (n == "profile") {
        if (!value) drain_events(ctx);
        ctx->profile = value != 0;
    } else if (n == "resident_exchange_only") {
        // measurement only (the kernel skips its arithmetic: results are WRONG): refused unless the process asked for
        // the debug switches, so that no ordinary caller of a shared context can leave it on
        const char* dbg = getenv("MIDYN_DEBUG_OPTIONS");
        if (value != 0 && !(dbg && dbg[0] == '1'))
            return fail(ctx, "midyn_ctx_set_option: resident_exchange_only makes rk4_resident_kernel return wrong results; "
                             "it is accepted only with MIDYN_DEBUG_OPTIONS=1 in the environment");
        ctx->resident_exchange_only = value != 0;
    }
    else if (n == "resident_spin_limit") ctx->resident_spin_limit = value < 0 ? (1u << 21) : (unsigned)std::min<long long>(value, 1ll << 30);
    else if (n == "combine_min_cols") ctx->combine_min_cols = (int)std::max<long long>(value, 128);
    else return fail(ctx, "midyn_ctx_set_option: unknown option " + n);
    return 0;
}

// The present value of an option (what a caller that changes one for a while puts back afterwards).
extern "C" int midyn_ctx_get_option(midyn_ctx* ctx, const char* name, long long* value) {
    if (!ctx || !name || !value) return fail(ctx, "midyn_ctx_get_option: NULL argument");
    std::string n(name);
#define MIDYN_X(opt_) if (n == #opt_) { *value = (long long)ctx->opt_; return 0; }
    MIDYN_SWITCH_OPTIONS(MIDYN_X)
    MIDYN_INT_OPTIONS(MIDYN_X)
    MIDYN_X(profile) MIDYN_X(resident_exchange_only) MIDYN_X(resident_spin_limit) MIDYN_X(combine_min_cols)
#undef MIDYN_X
    return fail(ctx, "midyn_ctx_get_option: unknown option " + n);
}

extern "C" int midyn_get_counters(midyn_ctx* ctx, const char* name, double* out) {
    if (!ctx || !name || !out) return fail(ctx, "midyn_get_counters: NULL argument");
    drain_events(ctx);
    for (int i = 0; i < KC_COUNT; ++i)
        if (std::string(name) == kclass_names[i]) {
            out[0] = ctx->cls_n[i];
            out[1] = ctx->cls_ms[i];
            return 0;
        }
    if (std::string(name).rfind("flops:", 0) == 0) {   // "flops:<class>": (real flops executed by the dense MFMA launches of the class
        for (int i = 0; i < KC_COUNT; ++i)                //  while `profile` was on -- 4M 8, 3M 6, single plane 4 per complex MAC --, 0)
            if (std::string(name).substr(6) == kclass_names[i]) {
                out[0] = ctx->cls_flops[i];
                out[1] = 0;
                return 0;
            }
    }
    if (std::string(name) == "sparse_tile") {   // (BM, BN) of the last sparse MFMA launch
        out[0] = ctx->last_sparse[0];
        out[1] = ctx->last_sparse[1];
        return 0;
    }
    if (std::string(name) == "sparse_pair") {   // contractions per launch of the last sparse MFMA launch (1 or 2)
        out[0] = ctx->last_sparse[4];
        out[1] = 0;
        return 0;
    }
    if (std::string(name) == "sweep_series") {  // last ell_sweep_kernel launch: (series terms per instance, operator slots per row)
        out[0] = ctx->last_sweep[0];
        out[1] = ctx->last_sweep[1];
        return 0;
    }
    if (std::string(name) == "resident_fallbacks") {   // (step ranges a one-launch kernel gave up on and the per-launch route re-ran, 0)
        out[0] = (double)ctx->resident_fallbacks;
        out[1] = 0;
        return 0;
    }
    if (std::string(name) == "sweep_cross") {   // last ell_sweep_duo_kernel launch: (operator slots per row whose operands cross the halves, slots per row)
        out[0] = ctx->last_sweep[4];
        out[1] = ctx->last_sweep[1];
        return 0;
    }
    if (std::string(name) == "sweep_split") {   // ... (workgroups per instance of that launch, element form: 0 general, 1 packed, 2 direct, 3 none -- one flip mask per slot)
        out[0] = ctx->last_sweep[2];
        out[1] = ctx->last_sweep[3];
        return 0;
    }
    if (std::string(name) == "combine_info") {   // last rhs_combine launch: (listed (32-row, 16-column) entries, 100 NRE4 + 10 NIM4 + static planes)
        out[0] = ctx->last_combine[0];
        out[1] = 100 * ctx->last_combine[1] + 10 * ctx->last_combine[2] + ctx->last_combine[3];
        return 0;
    }
    if (std::string(name) == "expm_plan_cache") {  // last one-shot sweep solve: (1 = plan found in the stack, 0 = made)
        out[0] = ctx->last_plan_cache;
        out[1] = 0.0;
        return 0;
    }
    if (std::string(name) == "gentable_info") {   // last midyn_gentable solve: (chunks, steps in its largest chunk)
        out[0] = ctx->last_gentable[0];
        out[1] = ctx->last_gentable[1];
        return 0;
    }
    if (std::string(name) == "gentable_staging") {   // ... (bytes of pinned host staging, bytes of device memory for raw rows)
        out[0] = ctx->last_gentable[2];
        out[1] = ctx->last_gentable[3];
        return 0;
    }
    if (std::string(name) == "expansion_pack") {  // last midyn_expansion_solve: (step matrices per padded 64 x 64 block: 1 or 2, 0)
        out[0] = ctx->last_expansion_pack;
        out[1] = 0;
        return 0;
    }
    if (std::string(name) == "combine_shape") {  // ... ((row group, column block) pairs per workgroup, waves that split the list of one pair)
        out[0] = ctx->last_combine[4];
        out[1] = ctx->last_combine[5];
        return 0;
    }
    if (std::string(name) == "combine_mirror") {   // ... (1 if it was mirrored (combine_mirror_kernel) else 0, the stack's mirror defect in units of eps)
        out[0] = ctx->last_mirror[0];
        out[1] = ctx->last_mirror[1];
        return 0;
    }
    if (std::string(name) == "combine_wave") {   // ... (state columns per wave: 64, or 32 -- wide stacks and small sweeps --, 0)
        out[0] = ctx->last_combine[6];
        out[1] = 0;
        return 0;
    }
    if (std::string(name) == "combine_sweep") {  // last combine_sweep_kernel launch: (workgroups, 10 x waves per workgroup + row tiles per wave)
        out[0] = ctx->last_combine_sweep[0];
        out[1] = 10 * ctx->last_combine_sweep[1] + ctx->last_combine_sweep[2];
        return 0;
    }
    if (std::string(name) == "sparse_list") {   // (listed tiles over all row panels, split count) of that launch
        out[0] = ctx->last_sparse[2];
        out[1] = ctx->last_sparse[3];
        return 0;
    }
    return fail(ctx, std::string("midyn_get_counters: unknown counter ") + name);
}

extern "C" int midyn_reset_counters(midyn_ctx* ctx) {
    if (!ctx) return fail(nullptr, "NULL ctx");
    drain_events(ctx);
    for (int i = 0; i < KC_COUNT; ++i) ctx->cls_ms[i] = ctx->cls_n[i] = ctx->cls_flops[i] = 0;
    return 0;
}

static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
static inline size_t round_up_sz(size_t x, size_t m) { return (x + m - 1) / m * m; }
static inline int grid_for(size_t total, int cap = 4096) {
    size_t b = (total + 255) / 256;
    if (b < 1) b = 1;
    if (b > (size_t)cap) b = cap;
    return (int)b;
}

// -------------------------------------------------------------------------------------------------
// operator stack
// -------------------------------------------------------------------------------------------------
struct midyn_stack {
    midyn_ctx* ctx = nullptr;
    int n = 0, n_pad = 0, k = 0, has_static = 0, has_frame = 0, nseg = 0;
    char* buf = nullptr;  // packed device buffer
    bool owns = false;
    size_t bytes = 0;
    double2* ops = nullptr;     // [nseg][n_pad][n_pad]
    double* frame_im = nullptr; // [n_pad]
    int* flags = nullptr;       // [2*nseg] plane non-zero flags (device)
    int* seg_all = nullptr;     // [nseg] every segment, mode 0 (device)
    int* seg_act = nullptr;     // [nseg] active list with plane modes (device)
    bool all_single_plane = false;  // every active segment is purely real or purely imaginary
    double* planes = nullptr;       // [n_act][n_pad][n_pad] planar copy of the non-zero planes (lazy)
    struct midyn_rk4_plan* eval_plan = nullptr;  // cached buffers of midyn_eval_rhs (keyed by m)
    struct midyn_expm_plan* sweep_plan = nullptr;   // the plan of the last one-shot midyn_expm_solve on the sweep route (ctx option
                                                    // expm_plan_cache): a scan that calls the one-shot entry point with the same time grid
                                                    // and y0 finds its tables, buffers and result block again (midyn_sweep_plan.inc)
    unsigned long long sweep_plan_epoch = 0;        // ctx->options_epoch when it was made
    int eval_m = 0;
    int n_act = 0;
    int uniform_mode = 3;       // plane mode shared by all active segments, or 3 (mixed)
    std::vector<int> h_flags;
    std::vector<int> h_modes;   // per segment: 0 full, 1 real only, 2 imaginary only, 3 zero
    std::vector<double> seg_norm1;  // ||A_seg||_1 per segment (lazy; norm bounds of the expm action)
    std::vector<double> seg_norminf, seg_herm1;  // ||A_seg||_inf and ||(A_seg + A_seg^dagger)/2||_1 (lazy; Chebyshev action)
    // block occupancy (lazy, stack_block_lists): which 16 x 16 blocks of the active segments hold a non-zero
    int blk_state = 0;              // 0 not examined, 1 lists built, -1 not applicable
    double blk_density = 1.0;       // non-zero 16 x 16 blocks / all blocks of the active segments
    size_t blk_nz = 0;              // number of non-zero 16 x 16 blocks
    int2* hull = nullptr;           // [n_act][n_pad/16] column hull (lo, hi) of the non-zero blocks per 16-row group (streaming kernel)
    double hull_fraction = 1.0;     // streamed fraction of the active planes when the hulls are used
    int* blk_ptr = nullptr;         // streaming lists per group of 16 rows: [n_pad/16 + 1]
    int* blk_idx = nullptr;         // entry = (segment << 16) | column chunk
    int* gw_ptr[4] = {nullptr, nullptr, nullptr, nullptr};  // MFMA tile lists per row panel of 64 / 128 / 32 / 16 rows: [M/BM + 1]
    int* gw_idx[4] = {nullptr, nullptr, nullptr, nullptr};  // entry = (K tile << 8) | (seg << 2 | mode)
    double gw_density[4] = {1.0, 1.0, 1.0, 1.0};            // listed tiles / all (panel, K tile, active segment) tiles
    double gw_avg[4] = {0.0, 0.0, 0.0, 0.0};                // average list length per row panel
    std::vector<unsigned char> grp_chunks;  // [n_pad/16][n_pad/64] any non-zero of any active segment (host; empty = not examined / dense)
    // register-resident single-trajectory RK4 (lazy, stack_resident_layout; midyn_resident.h)
    int res_state = 0;              // 0 not examined, 1 layout built, -1 not applicable
    int res_ne = 0;                 // entries per chunk (power of two >= number of active planes)
    bool res_halfq = false;         // no row group uses more than half of the chunk slots
    int* res_buf = nullptr;         // one device allocation: pairs | chunk_ptr | chunk_idx | poll_ptr | poll_idx
    size_t res_off[5] = {0, 0, 0, 0, 0};
    // lane-per-row variant for very sparse stacks (stack_ell_layout; ell_resident_kernel)
    int ell_state = 0;              // 0 not examined, 1 built, -1 not applicable
    int ell_wmax = 0;               // largest number of non-zero plane values in a row
    double* ell_val = nullptr;      // [ell_wmax][n_pad]
    int* ell_meta = nullptr;        // [ell_wmax][n_pad] (column as an index into the polled chunks)
    int* ell_meta_col = nullptr;    // [ell_wmax][n_pad] (column itself; source of the grouped arrays below)
    // the same elements grouped by (segment, plane): slot e of every row belongs to pair sp_tags[e] (ell_sweep_kernel)
    int sp_w = 0, sp_wre = 0;       // slots per row; the first sp_wre of them hold real-plane values
    int sp_wre_loc = 0, sp_wim_loc = 0;   // slots [0, sp_wre_loc) and [sp_wre, sp_wim_loc) keep every row's operand in the row's own half
                                          // of the vector (columns and rows on the same side of n_pad / 2): ell_sweep_duo_kernel
    double* sp_val = nullptr;       // [sp_w][n_pad]
    int* sp_col = nullptr;          // [sp_w][n_pad]
    int* sp_tags = nullptr;         // [sp_w] segment | plane << 8
    int sp_packed = 0;              // 1: every slot holds one magnitude (sp_pk = column | sign << 31, sp_mag), 2: and one sign, no
                                    // unused entry (sp_pk = LDS byte address of the operand, sp_mag signed); ell_sweep2_kernel
    int* sp_pk = nullptr;           // [sp_w][n_pad]
    double* sp_mag = nullptr;       // [sp_w]
    int sp_flip = 0;                // 1: on top of sp_packed 2 every slot has ONE flip mask, column = row ^ flip (ell_flip_duo_kernel); the
                                    // tables below are in the order the slots are applied (local re, local im, crossing re, crossing im)
    int* sp_flip_meta = nullptr;    // [sp_w] flip mask | imaginary-plane slot << 31
    int* sp_flip_xs = nullptr;      // [sp_w] STORAGE order: the flip as a byte offset in the chunked LDS layout (ell_sweep_kernel<.., 3>)
    int* sp_flip_tags = nullptr;    // [sp_w] segment | plane << 8
    double* sp_flip_mag = nullptr;  // [sp_w] signed magnitude
    int* ell_poll = nullptr;        // poll_ptr [n_pad/64 + 1] | poll_idx
    size_t ell_poll_off = 0;
    // COMBINE + APPLY layout of sweeps (lazy, stack_combine_layout; midyn_combine.h)
    int cmb_state = 0;              // 0 not examined, 2 lists known (host side only: cmb_h_*), 1 built (fragments packed), -1 not applicable
    std::vector<int> cmb_h_ptr, cmb_h_idx, cmb_h_rg;   // state 2: the lists the pack step will upload (released by it)
    int cmb_key = -1;               // the context options the layout was built under (skip_zero_planes | skip_zero_blocks << 1)
    int cmb_nre4 = 0, cmb_nim4 = 0; // groups of 4 real / imaginary planes of the time-dependent operators
    int cmb_stat = 0;               // planes of the static operator: bit 0 real, bit 1 imaginary (C input of the combination)
    int cmb_groups = 0;             // row groups of CMB_ROWS rows
    int cmb_planes = 0;             // time-dependent operator planes in the plane groups (the rest of the 4 (NRE4 + NIM4) slots is padding)
    long long cmb_entries = 0;      // listed (row group, kk block) entries
    double cmb_listed = 1.0;        // ... / all of them
    double* cmb_frags = nullptr;    // planes in MFMA A-operand order, [entry][kk % 16][tile][plane group][lane]
    int* cmb_ptr = nullptr;         // [cmb_groups + 1]
    int* cmb_idx = nullptr;         // kk block per entry
    int cmb_plane_col[24] = {0};    // coefficient column per plane slot (-1 padding)
    // ... mirrored form (built with the fragments; midyn_combine_mirror.h)
    int mir_state = 0;              // 1 eligible (lists below), -1 not
    double mir_defect = 0.0;        // max_p max|A_p[U,L] - s_p A_p[L,U]^T| / (eps max|A_p|) (-1: not examined)
    int mir_wpw = 0, mir_nsets = 0; // L row groups per workgroup, sets of them
    int* mir_ptr = nullptr;         // [nsets + 1] | [union position][wpw] fragment entry << 12 | kk block | [set][U block] covered,
    int* mir_ent = nullptr;         //   one allocation
    int* mir_cover = nullptr;
    double2* mir_part = nullptr;    // partial sums of the U rows [nsets][n_pad / 2][ld] (grown on demand)
    size_t mir_part_bytes = 0;
};

static void stack_drop_combine(midyn_stack* s) {
    if (s->cmb_frags) hipFree(s->cmb_frags);
    if (s->cmb_ptr) hipFree(s->cmb_ptr);
    if (s->cmb_idx) hipFree(s->cmb_idx);
    if (s->mir_ptr) hipFree(s->mir_ptr);
    if (s->mir_part) hipFree(s->mir_part);
    s->mir_ptr = s->mir_ent = s->mir_cover = nullptr;
    s->mir_part = nullptr;
    s->mir_part_bytes = 0;
    s->mir_state = 0;
    s->mir_defect = 0.0;
    s->cmb_frags = nullptr;
    s->cmb_ptr = s->cmb_idx = nullptr;
    s->cmb_state = 0;
    s->cmb_entries = 0;
    std::vector<int>().swap(s->cmb_h_ptr);
    std::vector<int>().swap(s->cmb_h_idx);
    std::vector<int>().swap(s->cmb_h_rg);
}

static void stack_drop_sweep_plan(midyn_stack* s);     // (midyn_sweep_plan.inc)
static void stack_drop_resident(midyn_stack* s) {
    stack_drop_sweep_plan(s);       // (its tables point into the layouts dropped here)
    if (s->res_buf) hipFree(s->res_buf);
    s->res_buf = nullptr;
    s->res_state = 0;
    if (s->ell_val) hipFree(s->ell_val);
    if (s->ell_meta) hipFree(s->ell_meta);
    if (s->ell_meta_col) hipFree(s->ell_meta_col);
    s->ell_meta_col = nullptr;
    if (s->sp_val) hipFree(s->sp_val);
    if (s->sp_col) hipFree(s->sp_col);
    if (s->sp_tags) hipFree(s->sp_tags);
    if (s->sp_pk) hipFree(s->sp_pk);
    if (s->sp_mag) hipFree(s->sp_mag);
    if (s->sp_flip_meta) hipFree(s->sp_flip_meta);
    if (s->sp_flip_xs) hipFree(s->sp_flip_xs);
    s->sp_flip_xs = nullptr;
    if (s->sp_flip_tags) hipFree(s->sp_flip_tags);
    if (s->sp_flip_mag) hipFree(s->sp_flip_mag);
    s->sp_flip_meta = nullptr;
    s->sp_flip_tags = nullptr;
    s->sp_flip_mag = nullptr;
    s->sp_flip = 0;
    s->sp_pk = nullptr;
    s->sp_mag = nullptr;
    s->sp_packed = 0;
    s->sp_val = nullptr;
    s->sp_col = nullptr;
    s->sp_tags = nullptr;
    s->sp_w = 0;
    if (s->ell_poll) hipFree(s->ell_poll);
    s->ell_val = nullptr;
    s->ell_meta = nullptr;
    s->ell_poll = nullptr;
    s->ell_state = 0;
    s->grp_chunks.clear();
}

static size_t align256(size_t x) { return (x + 255) / 256 * 256; }

struct PackLayout {
    size_t off_ops, off_frame, off_flags, off_all, off_act, total;
};
static PackLayout pack_layout(int n_pad, int nseg) {
    PackLayout L;
    size_t o = 0;
    L.off_ops = o;
    o = align256(o + (size_t)nseg * n_pad * n_pad * sizeof(double2));
    L.off_frame = o;
    o = align256(o + (size_t)n_pad * sizeof(double));
    L.off_flags = o;
    o = align256(o + (size_t)2 * std::max(nseg, 1) * sizeof(int));
    L.off_all = o;
    o = align256(o + (size_t)std::max(nseg, 1) * sizeof(int));
    L.off_act = o;
    o = align256(o + (size_t)std::max(nseg, 1) * sizeof(int));
    L.total = o;
    return L;
}

extern "C" int midyn_stack_packed_bytes(int n, int k, int has_static, size_t* bytes) {
    if (!bytes || n <= 0 || k < 0) return fail(nullptr, "midyn_stack_packed_bytes: bad argument");
    *bytes = pack_layout(round_up(n, 64), k + (has_static ? 1 : 0)).total;
    return 0;
}

static void stack_bind(midyn_stack* s) {
    PackLayout L = pack_layout(s->n_pad, s->nseg);
    s->bytes = L.total;
    s->ops = reinterpret_cast<double2*>(s->buf + L.off_ops);
    s->frame_im = reinterpret_cast<double*>(s->buf + L.off_frame);
    s->flags = reinterpret_cast<int*>(s->buf + L.off_flags);
    s->seg_all = reinterpret_cast<int*>(s->buf + L.off_all);
    s->seg_act = reinterpret_cast<int*>(s->buf + L.off_act);
}

// derive the active segment list from the plane flags (host copy) and upload both lists
static int stack_finish_lists(midyn_stack* s) {
    midyn_ctx* ctx = s->ctx;
    s->h_flags.assign(2 * std::max(s->nseg, 1), 0);
    if (s->nseg > 0)
        HIPCHK(ctx, hipMemcpy(s->h_flags.data(), s->flags, 2 * s->nseg * sizeof(int), hipMemcpyDeviceToHost));
    std::vector<int> all(std::max(s->nseg, 1), 0), act(std::max(s->nseg, 1), 0);
    s->n_act = 0;
    s->h_modes.assign(std::max(s->nseg, 1), 3);
    int um = -1;
    for (int seg = 0; seg < s->nseg; ++seg) {
        all[seg] = seg << 2;
        const int fr = s->h_flags[2 * seg], fi = s->h_flags[2 * seg + 1];
        if (!fr && !fi) continue;            // exactly zero operator: contributes nothing
        int mode = 0;
        if (fr && !fi) mode = 1;             // real only
        if (!fr && fi) mode = 2;             // imaginary only
        s->h_modes[seg] = mode;
        um = (um == -1 || um == mode) ? mode : 3;
        act[s->n_act++] = (seg << 2) | mode;
    }
    s->uniform_mode = um < 0 ? 0 : um;
    s->all_single_plane = s->n_act > 0;
    for (int seg = 0; seg < s->nseg; ++seg)
        if (s->h_modes[seg] == 0) s->all_single_plane = false;
    HIPCHK(ctx, hipMemcpy(s->seg_all, all.data(), all.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(s->seg_act, act.data(), act.size() * sizeof(int), hipMemcpyHostToDevice));
    return 0;
}

extern "C" int midyn_stack_create(midyn_ctx* ctx, int n, int k, const midyn_complex* ops,
                                  const midyn_complex* static_op, const double* frame_im,
                                  void* dev_buffer, midyn_stack** out) {
    if (!ctx || !out) return fail(ctx, "midyn_stack_create: NULL ctx/out");
    if (n <= 0 || k < 0) return fail(ctx, "midyn_stack_create: n must be > 0 and k >= 0");
    if (k > 0 && !ops) return fail(ctx, "midyn_stack_create: k > 0 but ops is NULL");
    if (k == 0 && !static_op)
        return fail(ctx, "midyn_stack_create: neither static operator nor operators given");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    midyn_stack* s = new midyn_stack();
    s->ctx = ctx;
    s->n = n;
    s->n_pad = round_up(n, 64);
    s->k = k;
    s->has_static = static_op ? 1 : 0;
    s->has_frame = frame_im ? 1 : 0;
    s->nseg = k + s->has_static;
    PackLayout L = pack_layout(s->n_pad, s->nseg);
    if (dev_buffer) {
        s->buf = static_cast<char*>(dev_buffer);
        s->owns = false;
    } else {
        HIPCHK(ctx, hipMalloc(&s->buf, L.total));
        s->owns = true;
    }
    stack_bind(s);
    HIPCHK(ctx, hipMemsetAsync(s->buf, 0, L.total, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const size_t plane = (size_t)s->n_pad * s->n_pad;
    int seg = 0;
    if (static_op) {
        HIPCHK(ctx, hipMemcpy2D(s->ops, (size_t)s->n_pad * sizeof(double2), static_op,
                                (size_t)n * sizeof(double2), (size_t)n * sizeof(double2), n,
                                hipMemcpyHostToDevice));
        seg = 1;
    }
    for (int j = 0; j < k; ++j, ++seg) {
        const char* src = reinterpret_cast<const char*>(ops) + (size_t)j * n * n * sizeof(double2);
        HIPCHK(ctx, hipMemcpy2D(s->ops + seg * plane, (size_t)s->n_pad * sizeof(double2), src,
                                (size_t)n * sizeof(double2), (size_t)n * sizeof(double2), n,
                                hipMemcpyHostToDevice));
    }
    if (frame_im)
        HIPCHK(ctx, hipMemcpy(s->frame_im, frame_im, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    if (s->nseg > 0) {
        hipLaunchKernelGGL(plane_flags_kernel, dim3(grid_for(plane * s->nseg)), dim3(256), 0, ctx->stream,
                           s->ops, plane, s->nseg, s->flags);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    CHK(stack_finish_lists(s));
    *out = s;
    return 0;
}

extern "C" int midyn_stack_adopt(midyn_ctx* ctx, int n, int k, int has_static, int has_frame,
                                 void* dev_buffer, midyn_stack** out) {
    if (!ctx || !out || !dev_buffer) return fail(ctx, "midyn_stack_adopt: NULL argument");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    midyn_stack* s = new midyn_stack();
    s->ctx = ctx;
    s->n = n;
    s->n_pad = round_up(n, 64);
    s->k = k;
    s->has_static = has_static ? 1 : 0;
    s->has_frame = has_frame ? 1 : 0;
    s->nseg = k + s->has_static;
    s->buf = static_cast<char*>(dev_buffer);
    s->owns = false;
    stack_bind(s);
    CHK(stack_finish_lists(s));
    *out = s;
    return 0;
}

extern "C" int midyn_rk4_plan_destroy(struct midyn_rk4_plan* p);

extern "C" int midyn_stack_destroy(midyn_stack* s) {
    if (!s) return 0;
    hipSetDevice(s->ctx->device);
    hipStreamSynchronize(s->ctx->stream);
    if (s->eval_plan) midyn_rk4_plan_destroy(s->eval_plan);
    s->eval_plan = nullptr;
    stack_drop_sweep_plan(s);
    if (s->planes) hipFree(s->planes);
    s->planes = nullptr;
    if (s->hull) hipFree(s->hull);
    s->hull = nullptr;
    stack_drop_resident(s);
    stack_drop_combine(s);
    for (int* q : {s->blk_ptr, s->blk_idx, s->gw_ptr[0], s->gw_idx[0], s->gw_ptr[1], s->gw_idx[1], s->gw_ptr[2], s->gw_idx[2],
                   s->gw_ptr[3], s->gw_idx[3]})
        if (q) hipFree(q);
    if (s->owns && s->buf) hipFree(s->buf);
    delete s;
    return 0;
}

extern "C" int midyn_stack_info(midyn_stack* s, long long* info) {
    if (!s || !info) return fail(nullptr, "midyn_stack_info: NULL argument");
    info[0] = s->n;
    info[1] = s->n_pad;
    info[2] = s->k;
    info[3] = s->has_static;
    info[4] = s->has_frame;
    info[5] = s->nseg;
    info[6] = s->n_act;
    info[7] = (long long)(s->bytes >> 20);
    return 0;
}

extern "C" int midyn_stack_segment_modes(midyn_stack* s, int* modes) {
    if (!s || !modes) return fail(nullptr, "midyn_stack_segment_modes: NULL argument");
    for (int i = 0; i < s->nseg; ++i) modes[i] = s->h_modes[i];
    return 0;
}
