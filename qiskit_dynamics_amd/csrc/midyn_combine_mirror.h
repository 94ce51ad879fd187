// midyn_combine_mirror.h -- the COMBINE + APPLY contraction (midyn_combine.h) for stacks whose operators only couple the two
// halves of the rows (round 7)
//
// Call the first n_pad / 2 rows L and the others U.  In the frame basis of a parity-conserving Hamiltonian model with a frame
// that holds the whole static part, every time-dependent operator maps L to U and U to L only (the diagonal quadrants are
// zero), and the generator -i H has symmetric imaginary planes and antisymmetric real ones:
//
//     A_p[U, L] = s_p A_p[L, U]^T        s_p = +1 (imaginary plane), -1 (real plane)
//
// The frame phases sit outside the contraction (pre-phased stage input, epilogue), so the combined operator of an instance,
// g_b = sum_j c_j[b] A_j, keeps that symmetry.  rhs_combine_kernel forms g_b twice, once for the L rows and once for the U
// rows.  This kernel forms it once, on the listed (L row group, U column block) entries, and applies it twice:
//
//     out[L] += g y[U]                   (direct: the accumulators of rhs_combine_kernel, its fused epilogue)
//     out[U] += s g^T y[L]               (transposed: in-lane sums over the wave's 8 rows of a column, then across the 4 lane
//                                         rows by permlane swaps, across the waves of a workgroup in LDS, and across the
//                                         workgroups that hold the other L row groups by mirror_finish_kernel)
//
// Per (kk, instance) and wave of 32 L rows: 2 P MFMA-FMAs (P planes) for the combination -- half of what the two row halves
// cost on rhs_combine_kernel -- and 2 x 2 x 8 vector FMAs for the two applications (the same number as before).
//
// Workgroup: wpw (8 where the stack has that many L row groups) waves, wave w owns L row group (set * wpw + w) and the SAME 32
// instance columns; they walk the union of their kk block lists in one order and meet at one barrier per 16-column block.
// The 16 state rows y[U block] of a block, the same for all of them, are loaded once per workgroup, one block ahead, into LDS
// (dynamic LDS: partial sums 2 x wpw x 8 KB, then this stage input 2 x 8 KB).  The partial sums of the U rows of a set go
// to part[set][u][col] for the U blocks of its walk only; mirror_finish_kernel adds, in a fixed set order, the sets whose walk
// covers the row's U block (cover[set][U block], built with the walks; no atomics: results are the same from run to run) and
// runs the epilogue of the U rows.  A U row that no set covers gets the epilogue of a zero contraction.
// A wave without an entry for a block of the walk runs the block on the zero padding entry of the fragment array (its MFMAs and
// FMAs add zeros): a wave-uniform branch around the block, which would skip that work, costs 25-61 spilled registers in every
// variant (the look-ahead loads of the next block then have two definitions).  On the parity-sector stacks every L row group
// lists every U block, and no work is wasted.
#pragma once

namespace midyn {

struct MirrorArgs {
    CombineArgs c;           // frags / B / coeff / plane columns / epilogue of rhs_combine_kernel (stat: none, splits: 1)
    const int* set_ptr;      // [nsets + 1]: union positions (16-column blocks) of every set of wpw L row groups
    const int* set_ent;      // [position][wpw]: fragment entry of wave w at that position (the zero padding entry if it has none)
                             // << 12 | kk block (U columns) of the position
    int wpw;                 // waves (L row groups) per workgroup: 8, 4, 2 or 1
    int nsets;               // L row groups / wpw
    int half;                // n_pad / 2
    double2* part;           // [nsets][half][ldb] partial sums of the U rows
};

// x (lanes 0-31) and y (lanes 32-63) summed over the two halves of the wave: lanes 0-31 get x_lo + x_hi, lanes 32-63 y_lo + y_hi
__device__ __forceinline__ double swap_sum32(double x, double y) {
    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(x), (unsigned)__double2loint(y), false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(x), (unsigned)__double2hiint(y), false, false);
    return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
}
// the same between the 16-lane rows 0 / 1 and 2 / 3: even rows get x_even + x_odd, odd rows y_even + y_odd
__device__ __forceinline__ double swap_sum16(double x, double y) {
    const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(x), (unsigned)__double2loint(y), false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(x), (unsigned)__double2hiint(y), false, false);
    return __hiloint2double((int)hi[0], (int)lo[0]) + __hiloint2double((int)hi[1], (int)lo[1]);
}

// The fragment ring of a variant: its stages, and how many kk steps ahead of its MFMAs a step's fragments are loaded.  Four
// stages close inside the four steps of the rolled j4 body without register moves; two steps ahead keep three of them live (a
// third step ahead spills in <0, 2>).  The variants with more than two plane groups have no registers for more than two stages.
constexpr int mirror_ring_depth(int nre4, int nim4) { return nre4 + nim4 <= 2 ? 4 : 2; }
constexpr int mirror_ring_ahead(int nre4, int nim4) { return nre4 + nim4 <= 2 ? 2 : 1; }

// The sum over the waves of a workgroup of a block's transposed partials (buf[w][16 kk][32 instances]), in wave order
// (buf[0] + buf[1] + ..): every wave sums 512 / (waves) elements and stores them to the rows of `part` that start at pout.
// mirror_wave_sum<WP>: WP a compile-time count, all reads of an element issued before the first add (one LDS round trip in
// place of WP; WP double2 registers: used with eight waves by the variants that have them).  mirror_wave_sum_any: any count,
// a read per add.
template <int WP>
__device__ __forceinline__ void mirror_wave_sum(const double2* buf, double2* pout, int ldb, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < 512 / WP; i += 64) {
        const int el = wave * (512 / WP) + i + lane;
        double2 v[WP];
#pragma unroll
        for (int w = 0; w < WP; ++w) v[w] = buf[(unsigned)(w * 16 * 32 + el)];
        double2 s = v[0];
#pragma unroll
        for (int w = 1; w < WP; ++w) {
            s.x += v[w].x;
            s.y += v[w].y;
        }
        pout[(size_t)(el >> 5) * ldb + (el & 31)] = s;
    }
}

__device__ __forceinline__ void mirror_wave_sum_any(const double2* buf, double2* pout, int ldb, int wave, int lane, int wpw) {
    const int per_wave = 512 / wpw;
#pragma clang loop unroll(disable)
    for (int i = 0; i < per_wave; i += 64) {
        const int el = wave * per_wave + i + lane;
        double2 s = buf[(unsigned)el];
        for (int w = 1; w < wpw; ++w) {
            const double2 v = buf[(unsigned)(w * 16 * 32 + el)];
            s.x += v.x;
            s.y += v.y;
        }
        pout[(size_t)(el >> 5) * ldb + (el & 31)] = s;
    }
}

// The body of combine_mirror_kernel<NRE4, NIM4> (ABL = 0).  ABL != 0 is profiling only (mirror_probe_kernel, ctx option
// mirror_ablate; results wrong): bit 0 = every step re-uses the fragments loaded for the first step of the launch (no global
// loads in the kk loop; the operands pass through an empty asm per step, so the combination stays in the loop), bit 1 = no
// phase behind the barrier (no cross-wave sum, no store of the partial sums).
template <int NRE4, int NIM4, int ABL>
__device__ __forceinline__ void combine_mirror_body(const MirrorArgs& m) {
    constexpr int NQ = NRE4 + NIM4, RT = 2, NG = 2;
    constexpr bool RE = NRE4 > 0, IM = NIM4 > 0;
    static_assert(combine_groups_ok(NRE4, NIM4), "plane groups");
    const CombineArgs& a = m.c;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double2* const lds = reinterpret_cast<double2*>(smem_raw);      // partials [2][wpw][16 kk][32 instances], then the stage input
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int set = blockIdx.x % m.nsets;
    const int rg = set * m.wpw + wave;                  // L row group of this wave
    const int col0 = (blockIdx.x / m.nsets) * (NG * 16);
    const int lb = lane & 15, lq = lane >> 4;

    double cb[NG][NQ];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        int in = (col0 + 16 * g + lb) / a.m_cols;
        in = in < a.n_inst ? in : a.n_inst - 1;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int pc = a.plane_col[4 * q + lq];
            cb[g][q] = pc >= 0 ? a.coeff[(long long)in * a.inst_stride + pc] : 0.0;
        }
    }
    d4 ore[RT][NG], oim[RT][NG];
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            ore[t][g] = d4{0.0, 0.0, 0.0, 0.0};
            oim[t][g] = d4{0.0, 0.0, 0.0, 0.0};
        }
    const double2* __restrict__ yb = a.B + col0;
    // the transposed operand: the state at this lane's 8 L rows (16 t + lq + 4 r of the row group), both instance groups
    double2 yl[RT][4][NG];
#pragma unroll
    for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int g = 0; g < NG; ++g)
                yl[t][r][g] = yb[(size_t)(rg * CMB_ROWS + 16 * t + lq + 4 * r) * a.ldb + (unsigned)(16 * g + lb)];

    // The fragments run through a register ring of DEPTH stages: a step's loads are issued AHEAD steps before its MFMAs.
    // The 16 state rows y[U block] of a block are the same for every wave of the workgroup: they reach LDS once per
    // workgroup, one block ahead (each wave loads one pair of rows at the start of the block before and stores it ahead of that
    // block's barrier, which publishes it: the stage-input buffer of the other parity was last read before the barrier of the
    // block before), and a step reads its row from there (the four lane rows read the same address: a broadcast).
    constexpr int DEPTH = mirror_ring_depth(NRE4, NIM4), AHEAD = mirror_ring_ahead(NRE4, NIM4);
    double afr[DEPTH][RT][NQ];
    double2 yv[NG];
    // fragment loads of step k16 of the block (fragment entry ent) into stage b
    auto load = [&](int ent, int k16, int b, bool first = false) {
        if ((ABL & 1) && !first) {
#pragma unroll
            for (int t = 0; t < RT; ++t)
#pragma unroll
                for (int q = 0; q < NQ; ++q) asm volatile("" : "+v"(afr[0][t][q]));
            __builtin_amdgcn_sched_barrier(0);
            return;
        }
        const double* __restrict__ fn = a.frags + ((size_t)ent * 16 + k16) * (RT * NQ * 64);
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
            for (int q = 0; q < NQ; ++q) afr[b][t][q] = fn[(unsigned)((t * NQ + q) * 64 + lane)];
        __builtin_amdgcn_sched_barrier(0);
    };
    // this wave's pair of the 16 state rows of kk block kb (lanes 0-31: row 2 wave, lanes 32-63: row 2 wave + 1; slot
    // wave * 64 + lane of a stage-input buffer); stacks with fewer than 8 waves per workgroup fill the other pairs in stage_rest
    auto stage_load = [&](int kb, int pair) {
        return yb[(size_t)(kb * 16 + 2 * pair + (lane >> 5)) * a.ldb + (unsigned)(lane & 31)];
    };
    auto stage_rest = [&](int kb, double2* ybuf) {
        for (int pair = wave + m.wpw; pair < 8; pair += m.wpw) ybuf[(unsigned)(pair * 64 + lane)] = stage_load(kb, pair);
    };
    // transposed partials of two kk steps, per instance group: this lane's 8 rows summed
    double tre[2][NG], tim[2][NG];
    auto compute = [&](int bb, int kq, const double2* yrow) {
        const int b = (ABL & 1) ? 0 : bb;
#pragma unroll
        for (int g = 0; g < NG; ++g) yv[g] = yrow[(unsigned)(16 * g + lb)];
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            tre[kq][g] = 0.0;
            tim[kq][g] = 0.0;
        }
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            if (RE) {   // real planes, antisymmetric: out[U] -= g_re^T y[L]
                d4 gre[NG];
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    gre[g] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                    for (int q = 0; q < NRE4; ++q)
                        gre[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(afr[b][t][q], cb[g][q], gre[g], 0, 0, 0);
                }
#pragma unroll
                for (int g = 0; g < NG; ++g)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        ore[t][g][r] = fma(gre[g][r], yv[g].x, ore[t][g][r]);
                        oim[t][g][r] = fma(gre[g][r], yv[g].y, oim[t][g][r]);
                        tre[kq][g] = fma(-gre[g][r], yl[t][r][g].x, tre[kq][g]);
                        tim[kq][g] = fma(-gre[g][r], yl[t][r][g].y, tim[kq][g]);
                    }
            }
            if (IM) {   // imaginary planes, symmetric: out[U] += i g_im^T y[L]
                d4 gim[NG];
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    gim[g] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                    for (int q = 0; q < NIM4; ++q)
                        gim[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(afr[b][t][NRE4 + q], cb[g][NRE4 + q], gim[g], 0, 0, 0);
                }
#pragma unroll
                for (int g = 0; g < NG; ++g)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        ore[t][g][r] = fma(-gim[g][r], yv[g].y, ore[t][g][r]);
                        oim[t][g][r] = fma(gim[g][r], yv[g].x, oim[t][g][r]);
                        tre[kq][g] = fma(-gim[g][r], yl[t][r][g].y, tre[kq][g]);
                        tim[kq][g] = fma(gim[g][r], yl[t][r][g].x, tim[kq][g]);
                    }
            }
        }
    };

    // the cross-wave sum of a block's transposed partials (in buf) and their store to the rows of U block kb of `part`
    auto wave_sum = [&](const double2* buf, int kb) {
        if (ABL & 2) return;
        double2* const pout = m.part + ((size_t)set * m.half + (kb * 16 - m.half)) * a.ldb + col0;
        if (NQ <= 2 && m.wpw == 8) mirror_wave_sum<8>(buf, pout, a.ldb, wave, lane);
        else mirror_wave_sum_any(buf, pout, a.ldb, wave, lane, m.wpw);
    };
    const int p0 = m.set_ptr[set], p1 = m.set_ptr[set + 1];
    double2* const ylds = lds + (size_t)2 * m.wpw * (16 * 32);      // stage input: [2][16 kk][32 instances]
    if (p1 > p0) {
        // the walk (at most 64 blocks: stack_mirror_layout) in lane (position - p0) of two registers, read with v_readlane (loads
        // of the next block's entry inside the loop are vector loads -- the loop stores -- and drained the look-ahead loads)
        const int pl = p0 + lane < p1 ? p0 + lane : p1 - 1;
        const int walk = m.set_ent[pl * m.wpw + wave];
        int ent_c = __builtin_amdgcn_readlane(walk, 0), kb_c = ent_c & 4095;
        ent_c >>= 12;
#pragma unroll
        for (int k = 0; k < AHEAD; ++k) load(ent_c, k, k, k == 0);
        // the first block's state rows: the only ones not loaded a block ahead
        ylds[(unsigned)(wave * 64 + lane)] = stage_load(kb_c, wave);
        stage_rest(kb_c, ylds);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
        for (int pos = p0; pos < p1; ++pos) {
            // the next block's entry (the look-ahead past the last block re-reads the last one)
            const int pn = (pos + 1 < p1 ? pos + 1 : pos) - p0;
            const int wn = __builtin_amdgcn_readlane(walk, pn), ent_n = wn >> 12, kb_n = wn & 4095;
            const int par = (pos - p0) & 1;
            double2* const buf = lds + (size_t)par * (m.wpw * 16 * 32);
            const double2* const ycur = ylds + par * (16 * 32);
            const double2 ynext = stage_load(kb_n, wave);
#pragma clang loop unroll(disable)
            for (int j4 = 0; j4 < 4; ++j4) {
                // reduce-scatter over the 4 lane rows, a pair of steps at a time: lanes 0-31 keep the first step of a pair,
                // lanes 32-63 the second (h[k]: pair k of the quarter); then even lane rows keep pair 0, odd ones pair 1
                double h[2][NG][2];
                const bool last = j4 == 3;
                // step s of the quarter: the loads of step s + AHEAD (past the block's 16 steps: the next block's), then its MFMAs
                auto step = [&](auto S) {
                    constexpr int s_ = decltype(S)::value;
                    const bool nx = last && s_ + AHEAD >= 4;
                    load(nx ? ent_n : ent_c, nx ? s_ + AHEAD - 4 : 4 * j4 + s_ + AHEAD, (s_ + AHEAD) % DEPTH);
                    compute(s_ % DEPTH, s_ & 1, ycur + (4 * j4 + s_) * 32);
                    __builtin_amdgcn_sched_barrier(0);
                };
                step(std::integral_constant<int, 0>{});
                step(std::integral_constant<int, 1>{});
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    h[0][g][0] = swap_sum32(tre[0][g], tre[1][g]);
                    h[0][g][1] = swap_sum32(tim[0][g], tim[1][g]);
                }
                step(std::integral_constant<int, 2>{});
                step(std::integral_constant<int, 3>{});
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    h[1][g][0] = swap_sum32(tre[0][g], tre[1][g]);
                    h[1][g][1] = swap_sum32(tim[0][g], tim[1][g]);
                }
                // lane row lq now holds step 2 (lq & 1) + (lq >> 1) of the quarter
                const int kkl = 4 * j4 + 2 * (lq & 1) + (lq >> 1);
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    const double sr = swap_sum16(h[0][g][0], h[1][g][0]);
                    const double si = swap_sum16(h[0][g][1], h[1][g][1]);
                    buf[(unsigned)((wave * 16 + kkl) * 32 + 16 * g + lb)] = make_double2(sr, si);
                }
            }
            // the next block's state rows, then one barrier per block: the other buffers were last read before the barrier of
            // the previous block
            double2* const ynb = ylds + (par ^ 1) * (16 * 32);
            ynb[(unsigned)(wave * 64 + lane)] = ynext;
            stage_rest(kb_n, ynb);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
            wave_sum(buf, kb_c);
            ent_c = ent_n;
            kb_c = kb_n;
        }
    }
    // (the lane number again, from the execution mask count: a lane value of the prologue that is needed down here is kept
    //  live across the loop, which uses every register, and is parked in scratch -- tests/test_codeobj_mirror.py refuses that)
    int lane_t;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane_t));
    store_tile<RT, NG>(a.epi, rg * CMB_ROWS + (lane_t >> 4), col0 + (lane_t & 15), ore, oim);
}

template <int NRE4, int NIM4>
__global__ __launch_bounds__(512, 2) void combine_mirror_kernel(const MirrorArgs m) {
    combine_mirror_body<NRE4, NIM4, 0>(m);
}

// profiling only (ctx option mirror_ablate = ABL; results wrong): the <0, 2> body with parts of it taken out
template <int ABL>
__global__ __launch_bounds__(512, 2) void mirror_probe_kernel(const MirrorArgs m) {
    combine_mirror_body<0, 2, ABL>(m);
}

// The U rows: the partial sums of the sets whose walk covers the row's U block, added in set order (part[0] + part[1] + ..;
// a set that does not cover the block never wrote there), then the epilogue of today's indexing.
template <int EMODE>
__global__ __launch_bounds__(256) void mirror_finish_kernel(const double2* part, const int* cover, int nsets, int half, int ld, Epilogue e) {
    const size_t n = (size_t)half * ld;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int u = (int)(i / ld), hb = half / 16;
    double2 c = make_double2(0.0, 0.0);
    bool any = false;
    for (int h = 0; h < nsets; ++h) {
        if (!cover[h * hb + u / 16]) continue;
        const double2 v = part[(size_t)h * n + i];
        c = any ? make_double2(c.x + v.x, c.y + v.y) : v;
        any = true;
    }
    apply_epilogue_t<EMODE>(e, half + u, (int)(i % ld), c);
}

// max |A_p[U, L] - s_p A_p[L, U]^T| and max |A_p| of both planes of every time-dependent segment, per chunk of rows:
// partial[(seg * nchunk + chunk) * 4 + {0: defect re, 1: defect im, 2: max re, 3: max im}]
MIDYN_GLOBAL __launch_bounds__(256) void mirror_defect_kernel(const double2* A, int n, int seg0, int nchunk, double* partial) {
    __shared__ double red[4][256];
    const int seg = seg0 + blockIdx.y, half = n / 2;
    const double2* As = A + (size_t)seg * n * n;
    double d[4] = {0.0, 0.0, 0.0, 0.0};
    for (int r = blockIdx.x; r < n; r += nchunk)
        for (int c = threadIdx.x; c < n; c += 256) {
            const double2 x = As[(size_t)r * n + c];
            d[2] = fmax(d[2], fabs(x.x));
            d[3] = fmax(d[3], fabs(x.y));
            if (r >= half && c < half) {
                const double2 y = As[(size_t)c * n + r];
                d[0] = fmax(d[0], fabs(x.x + y.x));
                d[1] = fmax(d[1], fabs(x.y - y.y));
            }
        }
    for (int k = 0; k < 4; ++k) red[k][threadIdx.x] = d[k];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int k = 0; k < 4; ++k) red[k][threadIdx.x] = fmax(red[k][threadIdx.x], red[k][threadIdx.x + w]);
        __syncthreads();
    }
    if (threadIdx.x < 4) partial[((size_t)blockIdx.y * nchunk + blockIdx.x) * 4 + threadIdx.x] = red[threadIdx.x][0];
}

// ---- instantiations (midyn_tu_combine_mirror.hip) ----------------------------------------------------------------------------
#ifdef MIDYN_TU_COMBINE_MIRROR
#define MIDYN_COMBINE_MIRROR_EXTERN
#else
#define MIDYN_COMBINE_MIRROR_EXTERN extern
#endif
#define MIDYN_X(R_, I_) MIDYN_COMBINE_MIRROR_EXTERN template __global__ void combine_mirror_kernel<R_, I_>(const MirrorArgs);
MIDYN_X(0, 1) MIDYN_X(0, 2) MIDYN_X(1, 0) MIDYN_X(2, 0) MIDYN_X(1, 1) MIDYN_X(2, 2)
#undef MIDYN_X
#define MIDYN_X(A_) MIDYN_COMBINE_MIRROR_EXTERN template __global__ void mirror_probe_kernel<A_>(const MirrorArgs);
MIDYN_X(1) MIDYN_X(2) MIDYN_X(3)
#undef MIDYN_X
#define MIDYN_X(E_) MIDYN_COMBINE_MIRROR_EXTERN template __global__ void mirror_finish_kernel<E_>(const double2*, const int*, int, int, int, Epilogue);
MIDYN_X(EPI_RHS) MIDYN_X(EPI_RK1) MIDYN_X(EPI_RK2) MIDYN_X(EPI_RK3) MIDYN_X(EPI_RK4)
#undef MIDYN_X

}  // namespace midyn
