// midyn_combine.inc -- part of midyn.hip: host side of the COMBINE + APPLY sweep contraction (midyn_combine.h):
// lazily built per-stack layout (plane groups, row-group lists of non-zero kk blocks, operator planes in MFMA operand
// order) and the launch.  Reference: OperatorCollection.evaluate_rhs, models/operator_collections.py:101-134 (combine
// the operators with the instance's coefficients, then apply the result to the state).

// Build the layout once per stack, in two steps so that a stack whose sweep ends up on another route pays neither the
// fragment array (up to 1 GiB) nor the pack kernel:
//   pack = false: the plane groups and the row-group lists (one block_map launch + nseg (n_pad / 16)^2 bytes to the host) --
//                 everything the route rules need (cmb_nre4 / nim4 / stat / planes / entries); cmb_state 2
//   pack = true:  + the operator planes in MFMA operand order on the device; cmb_state 1
// cmb_state -1: not applicable (no time-dependent operator, more than 8 planes of each kind / 16 of one kind alone
// (combine_groups_ok), or a fragment array beyond 1 GiB or the device's free memory).
static int stack_mirror_layout(midyn_stack* s);

static int stack_combine_layout(midyn_stack* s, bool pack = true) {
    midyn_ctx* ctx = s->ctx;
    const int key = (ctx->skip_zero_planes ? 1 : 0) | (ctx->skip_zero_blocks ? 2 : 0);
    if (s->cmb_state && s->cmb_key != key) {   // examined under other options (A/B runs): again
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        stack_drop_combine(s);
    }
    if (s->cmb_state == 1 || s->cmb_state == -1 || (s->cmb_state == 2 && !pack)) return 0;
    const int np = s->n_pad, nb = np / 16, groups = np / CMB_ROWS;
    if (s->cmb_state == 0) {
        s->cmb_key = key;
        s->cmb_state = -1;
        if (s->k < 1 || s->n_pad % CMB_ROWS) return 0;
        // planes of the time-dependent operators (segments has_static ...): real ones first, then imaginary ones
        std::vector<int> re, im;
        for (int seg = s->has_static; seg < s->nseg; ++seg) {
            const int mode = ctx->skip_zero_planes ? s->h_modes[seg] : 0;
            if (mode == 0 || mode == 1) re.push_back(seg);
            if (mode == 0 || mode == 2) im.push_back(seg);
        }
        const int nre4 = ((int)re.size() + 3) / 4, nim4 = ((int)im.size() + 3) / 4;
        if (!combine_groups_ok(nre4, nim4)) return 0;
        int stat = 0;
        if (s->has_static) {
            const int mode = ctx->skip_zero_planes ? s->h_modes[0] : 0;
            stat = mode == 0 ? 3 : (mode == 1 ? 1 : (mode == 2 ? 2 : 0));
        }
        for (int p = 0; p < CMB_SLOTS; ++p) s->cmb_plane_col[p] = -1;
        for (size_t i = 0; i < re.size(); ++i) s->cmb_plane_col[i] = re[i] - s->has_static;
        for (size_t i = 0; i < im.size(); ++i) s->cmb_plane_col[4 * nre4 + i] = im[i] - s->has_static;
        // 16 x 16 block occupancy of every segment -> per group of CMB_ROWS rows the kk blocks where ANY plane (or the
        // static operator) holds a non-zero
        std::vector<unsigned char> map;
        if (ctx->skip_zero_blocks) {
            const size_t map_bytes = (size_t)s->nseg * nb * nb;
            DevBuf d_map;
            CHK(d_map.alloc(ctx, map_bytes));
            HIPCHK(ctx, hipMemsetAsync(d_map.p, 0, map_bytes, ctx->stream));
            hipLaunchKernelGGL(block_map_kernel, dim3(nb, s->nseg), dim3(256), 0, ctx->stream, s->ops, np, d_map.as<unsigned char>());
            HIPCHK(ctx, hipGetLastError());
            map.resize(map_bytes);
            HIPCHK(ctx, hipMemcpyAsync(map.data(), d_map.p, map_bytes, hipMemcpyDeviceToHost, ctx->stream));
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        }
        std::vector<int> ptr(groups + 1, 0), idx, ent_rg;
        for (int rg = 0; rg < groups; ++rg) {
            for (int kb = 0; kb < nb; ++kb) {
                bool any = map.empty();
                for (int seg = 0; seg < s->nseg && !any; ++seg) {
                    if (s->h_modes[seg] == 3 && ctx->skip_zero_planes) continue;
                    for (int rb = rg * (CMB_ROWS / 16); rb < (rg + 1) * (CMB_ROWS / 16) && !any; ++rb)
                        any = map[((size_t)seg * nb + rb) * nb + kb] != 0;
                }
                if (any) {
                    idx.push_back(kb);
                    ent_rg.push_back(rg);
                }
            }
            ptr[rg + 1] = (int)idx.size();
        }
        const size_t entries = idx.size();
        const size_t frag_bytes = (entries + 1) * 16 * 2 * (nre4 + nim4) * 64 * sizeof(double);
        if (entries == 0 || frag_bytes > ((size_t)1 << 30)) return 0;
        s->cmb_nre4 = nre4;
        s->cmb_nim4 = nim4;
        s->cmb_stat = stat;
        s->cmb_groups = groups;
        s->cmb_planes = (int)(re.size() + im.size());
        s->cmb_entries = (long long)entries;
        s->cmb_listed = (double)entries / ((double)groups * nb);
        s->cmb_h_ptr.swap(ptr);
        s->cmb_h_idx.swap(idx);
        s->cmb_h_rg.swap(ent_rg);
        s->cmb_state = 2;
        if (!pack) return 0;
    }
    // ---- pack: the planes in MFMA A-operand order --------------------------------------------------------------------------
    const int nq = s->cmb_nre4 + s->cmb_nim4;
    const size_t entries = (size_t)s->cmb_entries;
    const size_t frag_bytes = (entries + 1) * 16 * 2 * nq * 64 * sizeof(double);   // + one padding entry: the kernel's
                                                                                    // look-ahead load past the last entry
    CombinePackArgs pa{};
    for (int p = 0; p < CMB_SLOTS; ++p) {
        const int col = s->cmb_plane_col[p];
        pa.plane_seg[p] = col < 0 ? -1 : col + s->has_static;
        pa.plane_im[p] = col >= 0 && p >= 4 * s->cmb_nre4 ? 1 : 0;
    }
    DevBuf d_rg;
    CHK(d_rg.alloc(ctx, entries * sizeof(int)));
    hipError_t e = hipMalloc(&s->cmb_frags, frag_bytes);
    if (e == hipSuccess) e = hipMalloc(&s->cmb_ptr, s->cmb_h_ptr.size() * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(&s->cmb_idx, entries * sizeof(int));
    if (e != hipSuccess) {
        stack_drop_combine(s);
        s->cmb_state = -1;
        (void)hipGetLastError();
        return 0;   // no memory for the layout: the GEMM routes take the sweep
    }
    // (any failure below: the buffers just allocated are released and the layout is marked unusable -- a retry must not
    // allocate a second set on top of them, ADVICE round 5)
    struct PackGuard {
        midyn_stack* s;
        bool done = false;
        ~PackGuard() {
            if (!done) {
                stack_drop_combine(s);
                s->cmb_state = -1;
            }
        }
    } pack_guard{s};
    HIPCHK(ctx, hipMemsetAsync(s->cmb_frags + entries * 16 * 2 * nq * 64, 0, (size_t)16 * 2 * nq * 64 * sizeof(double), ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(s->cmb_ptr, s->cmb_h_ptr.data(), s->cmb_h_ptr.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(s->cmb_idx, s->cmb_h_idx.data(), entries * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_rg.p, s->cmb_h_rg.data(), entries * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    pa.ops = s->ops;
    pa.seg_stride = (long long)np * np;
    pa.lda = np;
    pa.ent_rg = d_rg.as<int>();
    pa.list_idx = s->cmb_idx;
    pa.nq = nq;
    pa.frags = s->cmb_frags;
    hipLaunchKernelGGL(combine_pack_kernel, dim3((unsigned)entries), dim3(256), 0, ctx->stream, pa);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));   // (the host lists are released below)
    CHK(stack_mirror_layout(s));
    std::vector<int>().swap(s->cmb_h_ptr);
    std::vector<int>().swap(s->cmb_h_idx);
    std::vector<int>().swap(s->cmb_h_rg);
    s->cmb_state = 1;
    pack_guard.done = true;
    return 0;
}

// The mirrored form (midyn_combine_mirror.h), decided once per stack from the host lists of the pack step: eligible when no entry
// of an L row group lies in L columns and none of a U row group in U columns (no static operator), and every plane of every
// time-dependent segment satisfies max|A_p[U,L] - s_p A_p[L,U]^T| <= 16 eps max|A_p| (mirror_defect_kernel).  Sets of wpw L row
// groups share a workgroup; their lists are merged into one walk (union of the kk blocks, the zero padding entry where a row
// group has none).  No memory for the lists: not eligible (the unmirrored kernel takes every launch).
static int stack_mirror_layout(midyn_stack* s) {
    midyn_ctx* ctx = s->ctx;
    s->mir_state = -1;
    s->mir_defect = -1.0;
    const int np = s->n_pad, half = np / 2, hb = half / 16, lgroups = half / CMB_ROWS;
    if (s->cmb_stat != 0 || half % CMB_ROWS || lgroups < 1 || s->k < 1) return 0;
    if (s->cmb_entries >= (1 << 19) || np / 16 > 4096) return 0;     // (entry << 12 | kk block in one int)
    const std::vector<int>& ptr = s->cmb_h_ptr;
    const std::vector<int>& idx = s->cmb_h_idx;
    for (int rg = 0; rg < s->cmb_groups; ++rg)
        for (int e = ptr[rg]; e < ptr[rg + 1]; ++e)
            if ((rg < lgroups) != (idx[e] >= hb)) return 0;     // an entry in a diagonal quadrant
    // the defect of the planes (one pass over the time-dependent segments)
    const int nseg = s->nseg - s->has_static, nchunk = 64;
    {
        DevBuf d_part;
        CHK(d_part.alloc(ctx, (size_t)nseg * nchunk * 4 * sizeof(double)));
        hipLaunchKernelGGL(mirror_defect_kernel, dim3(nchunk, nseg), dim3(256), 0, ctx->stream, s->ops, np, s->has_static, nchunk,
                           d_part.as<double>());
        HIPCHK(ctx, hipGetLastError());
        std::vector<double> part((size_t)nseg * nchunk * 4);
        HIPCHK(ctx, hipMemcpyAsync(part.data(), d_part.p, part.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        double worst = 0.0;
        for (int seg = 0; seg < nseg; ++seg)
            for (int pl = 0; pl < 2; ++pl) {
                double def = 0.0, mx = 0.0;
                for (int c = 0; c < nchunk; ++c) {
                    def = std::max(def, part[((size_t)seg * nchunk + c) * 4 + pl]);
                    mx = std::max(mx, part[((size_t)seg * nchunk + c) * 4 + 2 + pl]);
                }
                if (def > 0.0) worst = std::max(worst, mx > 0.0 ? def / (DBL_EPSILON * mx) : INFINITY);
            }
        s->mir_defect = worst;
        if (!(worst <= 16.0)) return 0;
    }
    int wpw = 8;
    while (lgroups % wpw) wpw /= 2;
    const int nsets = lgroups / wpw;
    std::vector<int> sptr(nsets + 1, 0), skb, sent, cover((size_t)nsets * hb, 0);
    for (int st = 0; st < nsets; ++st) {
        std::vector<int> kbs;
        for (int w = 0; w < wpw; ++w) {
            const int rg = st * wpw + w;
            kbs.insert(kbs.end(), idx.begin() + ptr[rg], idx.begin() + ptr[rg + 1]);
        }
        std::sort(kbs.begin(), kbs.end());
        kbs.erase(std::unique(kbs.begin(), kbs.end()), kbs.end());
        for (int kb : kbs) {
            skb.push_back(kb);
            cover[(size_t)st * hb + (kb - hb)] = 1;
            for (int w = 0; w < wpw; ++w) {
                const int rg = st * wpw + w;
                const int* f = std::lower_bound(idx.data() + ptr[rg], idx.data() + ptr[rg + 1], kb);
                const int e = f != idx.data() + ptr[rg + 1] && *f == kb ? (int)(f - idx.data()) : (int)s->cmb_entries;
                sent.push_back(e << 12 | kb);
            }
        }
        sptr[st + 1] = (int)skb.size();
        if (sptr[st + 1] - sptr[st] > 64) return 0;     // (the kernel keeps a set's walk in the 64 lanes of a register)
    }
    const size_t words = sptr.size() + sent.size() + cover.size();
    if (hipMalloc(&s->mir_ptr, words * sizeof(int)) != hipSuccess) {
        s->mir_ptr = nullptr;
        (void)hipGetLastError();
        return 0;
    }
    s->mir_ent = s->mir_ptr + sptr.size();
    s->mir_cover = s->mir_ent + sent.size();
    HIPCHK(ctx, hipMemcpyAsync(s->mir_ptr, sptr.data(), sptr.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(s->mir_ent, sent.data(), sent.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(s->mir_cover, cover.data(), cover.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    s->mir_wpw = wpw;
    s->mir_nsets = nsets;
    s->mir_state = 1;
    return 0;
}

// Is this contraction (ncol state columns in blocks of `ld`, B instances) one for the COMBINE + APPLY kernel?
static bool combine_wanted(const midyn_ctx* ctx, const midyn_stack* s, int B, int ld) {
    return ctx->combine && B > 1 && s->k > 0 && ld % 128 == 0 && ld >= ctx->combine_min_cols && ctx->ablate == 0 && ctx->force_tile == 0;
}

using CombineFn = void (*)(const CombineArgs);
template <int NRE4, int NIM4>
static CombineFn combine_kernel_stat(int stat) {
    switch (stat) {
        case 0: return rhs_combine_kernel<NRE4, NIM4, 0>;
        case 1: return rhs_combine_kernel<NRE4, NIM4, 1>;
        case 2: return rhs_combine_kernel<NRE4, NIM4, 2>;
        default: return rhs_combine_kernel<NRE4, NIM4, 3>;
    }
}
template <int NRE4, int NIM4>
static CombineFn combine_small_kernel_stat(int stat) {     // 32 instances per wave (stacks of up to two plane groups)
    switch (stat) {
        case 0: return rhs_combine_small_kernel<NRE4, NIM4, 0>;
        case 1: return rhs_combine_small_kernel<NRE4, NIM4, 1>;
        case 2: return rhs_combine_small_kernel<NRE4, NIM4, 2>;
        default: return rhs_combine_small_kernel<NRE4, NIM4, 3>;
    }
}

using MirrorFn = void (*)(const MirrorArgs);
using MirrorFinishFn = void (*)(const double2*, const int*, int, int, int, Epilogue);

// The mirrored launch pair (combine_mirror_kernel + mirror_finish_kernel) when the stack, the options and the shape call for it;
// *done = false: the caller runs the unmirrored kernel (no kernel for the plane layout, no memory for the partial sums).
static int launch_combine_mirror(midyn_ctx* ctx, midyn_stack* s, const CombineArgs& a, int ld, bool* done) {
    *done = false;
    const int mode = a.epi.mode;
    if (s->mir_state != 1 || ctx->combine_mirror == 0 || ctx->combine_ablate || ld % 32) return 0;
    if (mode != EPI_RHS && mode != EPI_RK1 && mode != EPI_RK2 && mode != EPI_RK3 && mode != EPI_RK4) return 0;
    // at least two waves per SIMD without splitting a list (n = 1024 on 256 CUs: from 4096 instances on)
    if (ctx->combine_mirror == 1 && (long long)(s->n_pad / 64) * (ld / 32) < 2ll * 4 * ctx->num_cu) return 0;
    MirrorFn fn = nullptr;
    int slot = 0;
#define MIDYN_CMM(R_, I_, SLOT_) \
    if (s->cmb_nre4 == R_ && s->cmb_nim4 == I_) { fn = combine_mirror_kernel<R_, I_>; slot = SLOT_; }
    MIDYN_CMM(0, 1, 0) MIDYN_CMM(0, 2, 1) MIDYN_CMM(1, 0, 2) MIDYN_CMM(2, 0, 3) MIDYN_CMM(1, 1, 4) MIDYN_CMM(2, 2, 5)
#undef MIDYN_CMM
    if (ctx->mirror_ablate >= 1 && ctx->mirror_ablate <= 3 && slot == 1) {   // profiling only (results wrong)
        fn = ctx->mirror_ablate == 1 ? mirror_probe_kernel<1> : ctx->mirror_ablate == 2 ? mirror_probe_kernel<2> : mirror_probe_kernel<3>;
        slot = 5 + ctx->mirror_ablate;
    }
    if (!fn) return 0;
    MirrorFinishFn fin = mode == EPI_RHS ? mirror_finish_kernel<EPI_RHS> : mode == EPI_RK1 ? mirror_finish_kernel<EPI_RK1>
                       : mode == EPI_RK2 ? mirror_finish_kernel<EPI_RK2> : mode == EPI_RK3 ? mirror_finish_kernel<EPI_RK3>
                       : mirror_finish_kernel<EPI_RK4>;
    const int half = s->n_pad / 2, wpw = s->mir_wpw, nsets = s->mir_nsets;
    // partial sums 2 x wpw x 8 KB + stage input 2 x 8 KB (144 KB with eight waves)
    const size_t lds = ((size_t)2 * wpw + 2) * 16 * 32 * sizeof(double2);
    if (lds > ctx->lds_per_block) return 0;
    const size_t part_bytes = (size_t)nsets * half * ld * sizeof(double2);
    if (part_bytes > s->mir_part_bytes) {
        if (s->mir_part) hipFree(s->mir_part);
        s->mir_part = nullptr;
        s->mir_part_bytes = 0;
        if (hipMalloc(&s->mir_part, part_bytes) != hipSuccess) {
            s->mir_part = nullptr;
            (void)hipGetLastError();
            return 0;
        }
        s->mir_part_bytes = part_bytes;
        // (the kernel writes every element the finishing kernel reads; zeros only so that a profiling launch that leaves the
        //  store out -- mirror_ablate -- works on finite numbers)
        HIPCHK(ctx, hipMemsetAsync(s->mir_part, 0, part_bytes, ctx->stream));
    }
    {
        // once per device and kernel, to the most a launch of it can ask for (eight waves), whatever this stack's wpw is: a
        // stack with fewer waves per workgroup may come first
        static DeviceOnce attr[9];
        if (attr[slot].needed(ctx->device)) {
            const size_t most = std::min(((size_t)2 * 8 + 2) * 16 * 32 * sizeof(double2), (size_t)ctx->lds_per_block);
            HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)most));
            attr[slot].done(ctx->device);
        }
    }
    MirrorArgs m{};
    m.c = a;
    m.c.stat = nullptr;
    m.c.splits = 1;
    m.c.wr = wpw;
    m.set_ptr = s->mir_ptr;
    m.set_ent = s->mir_ent;
    m.wpw = wpw;
    m.nsets = nsets;
    m.half = half;
    m.part = s->mir_part;
    note_variant("combine_mirror_kernel", {s->cmb_nre4, s->cmb_nim4});
    ctx->last_combine[0] = (double)s->cmb_entries;
    ctx->last_combine[1] = s->cmb_nre4;
    ctx->last_combine[2] = s->cmb_nim4;
    ctx->last_combine[3] = s->cmb_stat;
    ctx->last_combine[4] = wpw;
    ctx->last_combine[5] = 1;
    ctx->last_combine[6] = 32;
    ctx->last_mirror[0] = 1;
    ctx->last_mirror[1] = s->mir_defect;
    {
        ProfScope ps(ctx, KC_COMBINE);
        hipLaunchKernelGGL(fn, dim3((unsigned)(nsets * (ld / 32))), dim3(64u * wpw), lds, ctx->stream, m);
    }
    HIPCHK(ctx, hipGetLastError());
    const size_t elems = (size_t)half * ld;
    {
        ProfScope ps(ctx, KC_MIRROR_FINISH);
        hipLaunchKernelGGL(fin, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, ctx->stream,
                           (const double2*)s->mir_part, (const int*)s->mir_cover, nsets, half, ld, a.epi);
    }
    HIPCHK(ctx, hipGetLastError());
    *done = true;
    return 0;
}

// One evaluation  epilogue( sum_kk (G_d + sum_j c_j G_j)[r][kk] yin[kk][col] )  for all rows and the `ld` columns of yin.
static int launch_combine(midyn_ctx* ctx, midyn_stack* s, const double2* yin, int ld, const double* coeff, long long inst_stride,
                          int m_cols, int n_inst, const Epilogue& epi) {
    CombineArgs a{};
    a.frags = s->cmb_frags;
    a.list_ptr = s->cmb_ptr;
    a.list_idx = s->cmb_idx;
    a.stat = s->cmb_stat ? s->ops : nullptr;
    a.lda = s->n_pad;
    a.B = yin;
    a.ldb = ld;
    a.coeff = coeff;
    a.inst_stride = inst_stride;
    a.m_cols = m_cols;
    a.n_inst = n_inst;
    for (int p = 0; p < CMB_SLOTS; ++p) a.plane_col[p] = s->cmb_plane_col[p];
    a.n_row_groups = s->cmb_groups;
    a.epi = epi;
    if (ctx->combine_ablate & 1) {      // measurement only: the contraction with a bare store
        a.epi.mode = EPI_RHS;
        a.epi.out = epi.yin_next ? epi.yin_next : (epi.acc ? epi.acc : epi.out);
        a.epi.yin_next = nullptr;
        a.epi.e_cur = a.epi.e_next = nullptr;
    }
    {
        bool mirrored = false;
        CHK(launch_combine_mirror(ctx, s, a, ld, &mirrored));
        if (mirrored) return 0;
    }
    ctx->last_mirror[0] = 0;
    ctx->last_mirror[1] = s->mir_defect;
    CombineFn fn = nullptr;
#define MIDYN_CMB(R_, I_) \
    if (s->cmb_nre4 == R_ && s->cmb_nim4 == I_) fn = combine_kernel_stat<R_, I_>(s->cmb_stat);
    MIDYN_CMB(0, 1) MIDYN_CMB(0, 2) MIDYN_CMB(1, 0) MIDYN_CMB(2, 0) MIDYN_CMB(1, 1) MIDYN_CMB(1, 2) MIDYN_CMB(2, 1) MIDYN_CMB(2, 2)
    MIDYN_CMB(0, 3) MIDYN_CMB(0, 4) MIDYN_CMB(3, 0) MIDYN_CMB(4, 0)
    MIDYN_CMB(3, 1) MIDYN_CMB(3, 2) MIDYN_CMB(3, 3) MIDYN_CMB(1, 3) MIDYN_CMB(2, 3)
#undef MIDYN_CMB
    if (!fn) return fail(ctx, "launch_combine: no kernel for this plane layout");
    int ng = combine_ng(s->cmb_nre4, s->cmb_nim4, s->cmb_stat);   // 16-instance groups per wave
    const int occ = ctx->combine_occupancy >= 2 ? 2 : 1, max_splits = occ == 2 ? 8 : 4;
    const long long simds = 4ll * ctx->num_cu;
    // Sweeps of so few instances that 64-instance waves, even max_splits of them to a pair, leave SIMDs below the aimed
    // occupancy: 32 instances per wave (twice the pairs; twice the operand loads per MFMA, which a chip half idle can afford)
    if (occ == 2 && ng == 4 && (long long)s->cmb_groups * (ld / 64) * max_splits < occ * simds) {
        CombineFn small = nullptr;
#define MIDYN_CMBS(R_, I_) \
    if (s->cmb_nre4 == R_ && s->cmb_nim4 == I_) small = combine_small_kernel_stat<R_, I_>(s->cmb_stat);
        MIDYN_CMBS(0, 1) MIDYN_CMBS(0, 2) MIDYN_CMBS(1, 0) MIDYN_CMBS(2, 0) MIDYN_CMBS(1, 1)
#undef MIDYN_CMBS
        if (small) {
            fn = small;
            ng = 2;
        }
    }
    // Workgroup shape.  A (row group of 32 rows, block of 16 ng columns) pair is the unit of work; the chip wants at least one
    // wave per SIMD (4 per CU), better two, and one workgroup per CU (workgroups of fewer waves get packed several to a
    // CU while other CUs idle).  Large sweeps: 8 pairs per workgroup, one wave each, over 128 columns so that the waves
    // share their state rows and operator fragments in the L1.  Small sweeps (fewer pairs than 2 x SIMDs): 2, 4 or 8 waves
    // split the kk list of ONE pair and sum through LDS (no partial sums in memory, no second launch).
    const long long pairs = (long long)s->cmb_groups * (ld / (16 * ng));
    // combine_occupancy (occ) waves per SIMD are aimed at: with two, the loads of one wave's step hide behind the other's arithmetic
    int splits = 1;
    while (splits < max_splits && pairs * splits < occ * simds) splits *= 2;
    // the tree through LDS needs (pairs per workgroup) x splits / 2 slots of 2 ng x 4 KB: 128 KB with eight 64-instance waves on
    // one pair -- on a device whose workgroups cannot declare that much, fewer waves split a list (less occupancy, same result)
    while (splits > 1 && (size_t)(8 / splits) * (splits / 2) * 2 * ng * 8 * 64 * sizeof(double) > ctx->lds_per_block) splits /= 2;
    int wpw = 8;                                       // waves per workgroup
    while (wpw > splits && pairs * splits < (long long)wpw * ctx->num_cu) wpw /= 2;
    const int ppw = wpw / splits;                      // pairs per workgroup
    int nwi = 128 / (16 * ng);                         // ... of them along the columns
    if (nwi > ppw) nwi = ppw;
    a.wr = ppw / nwi;
    while (a.wr > 1 && s->cmb_groups % a.wr) a.wr /= 2;
    a.splits = splits;
    const int rgb = (s->cmb_groups + a.wr - 1) / a.wr;
    const unsigned grid = (unsigned)(rgb * (ld / (nwi * 16 * ng)));
    const unsigned threads = 64u * (unsigned)(a.wr * nwi * splits);
    const size_t lds = splits > 1 ? (size_t)(a.wr * nwi) * (splits / 2) * 2 * ng * 8 * 64 * sizeof(double) : 0;
    if (lds > 128 * 1024 || lds > ctx->lds_per_block) return fail(ctx, "launch_combine: workgroup shape beyond the LDS a workgroup may declare");
    if (lds > 48 * 1024) {
        static DeviceOnce attr[256];
        const int slot = ((((s->cmb_nre4 * 5 + s->cmb_nim4) * 4 + s->cmb_stat) << 1) | (ng == 2 && s->cmb_nre4 + s->cmb_nim4 <= 2)) & 255;
        if (attr[slot].needed(ctx->device)) {
            HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024));
            attr[slot].done(ctx->device);
        }
    }
    note_variant(ng == 2 && s->cmb_nre4 + s->cmb_nim4 <= 2 ? "rhs_combine_small_kernel" : "rhs_combine_kernel", {s->cmb_nre4, s->cmb_nim4, s->cmb_stat});
    ctx->last_combine[0] = (double)s->cmb_entries;
    ctx->last_combine[1] = s->cmb_nre4;
    ctx->last_combine[2] = s->cmb_nim4;
    ctx->last_combine[3] = s->cmb_stat;
    ctx->last_combine[4] = a.wr * nwi;
    ctx->last_combine[5] = splits;
    ctx->last_combine[6] = 16 * ng;
    {
        ProfScope ps(ctx, KC_COMBINE);
        hipLaunchKernelGGL(fn, dim3(grid), dim3(threads), lds, ctx->stream, a);
    }
    HIPCHK(ctx, hipGetLastError());
    return 0;
}
