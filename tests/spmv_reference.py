"""Extended-precision restatement of the sparse-operator route's C contract (include/midyn_spmv.h), for the tests that
drive ``midyn_spmv_eval_rhs`` / ``midyn_spmv_rk4_solve`` with plain arrays (tests/test_gpu_spmv_kernels.py) and for the
host-side tests of this module itself (tests/test_spmv_reference_host.py).  A helper module, not a test file; pure NumPy,
nothing of the package is imported.

  make_structure   padded row structures the contract allows: what ``pack_ell`` makes (style="pack") and what it never
                   makes (style="contract")
  rhs, rk4         the documented operation, one loop over slots and classic RK4, parametrised by dtype:
                   np.longdouble / np.clongdouble (80-bit) is THE reference, float64 / complex128 the calibration run
  tolerance        the absolute bound a device result is held to, from the calibration run's distance to the reference
  MUTANTS          in-bounds, wrong-value variants of the float64 restatement: the bound must reject every one
  RK4_CASES, EVAL_CASES, rk4_case, eval_case   the cases both test files use
"""
import numpy as np

if np.finfo(np.longdouble).eps > 2.0 ** -63:
    raise RuntimeError("spmv_reference: np.longdouble has no 64-bit mantissa on this platform (eps = %.3g): the reference "
                       "would be no more precise than the code under test" % float(np.finfo(np.longdouble).eps))

LD = (np.longdouble, np.clongdouble)
F64 = (np.float64, np.complex128)
EPS64 = float(np.finfo(np.float64).eps)

MUTANTS = ("coef_instance0", "stage3_weight", "phase_next_at_t", "no_conj_out", "stage4_coef_row1", "drop_last_slot",
           "out_slot_stride_m1", "y0_instance0", "phase_next_step_from_r2")


# ---------------------------------------------------------------------------------------------------------------------
# structures
# ---------------------------------------------------------------------------------------------------------------------
def row_lengths(struct):
    """Slots in use per row, by the rule of midyn_spmv_create: up to the last slot that is not (col = row, op = k, 0)."""
    n, k, w = struct["n"], struct["k"], struct["width"]
    unused = (struct["ops"] == k) & (struct["cols"] == np.arange(n)[:, None]) & (struct["vals"] == 0)
    return np.where(~unused, np.arange(1, w + 1)[None, :], 0).max(axis=1, initial=0).astype(np.int64)


def check_contract(struct):
    """NumPy restatement of what midyn_spmv_create requires and the header documents: shapes and types, index ranges,
    a row's slots grouped by operator index, unused slots last.  Raises AssertionError."""
    n, k, w = struct["n"], struct["k"], struct["width"]
    cols, ops, vals = struct["cols"], struct["ops"], struct["vals"]
    assert n > 0 and k >= 0 and w >= 0
    assert cols.shape == ops.shape == vals.shape == (n, w)
    assert cols.dtype == np.int32 and ops.dtype == np.int32 and vals.dtype == np.complex128
    assert all(a.flags.c_contiguous for a in (cols, ops, vals))
    assert np.all((cols >= 0) & (cols < n)), "column index outside [0, n)"
    assert np.all((ops >= 0) & (ops <= k)), "operator index outside [0, k]"
    assert np.all(np.isfinite(vals))
    length = row_lengths(struct)
    for r in range(n):
        used = ops[r, :length[r]]
        starts = np.flatnonzero(np.diff(used) != 0) + 1         # a group = a run of equal indices: every index has ONE run
        firsts = np.concatenate([used[:1], used[starts]])
        assert len(set(firsts.tolist())) == len(firsts), f"row {r}: the slots of an operator index are not adjacent"
        assert np.all(cols[r, length[r]:] == r) and np.all(ops[r, length[r]:] == k) and np.all(vals[r, length[r]:] == 0)
    fr = struct["frame_im"]
    assert fr is None or (fr.shape == (n,) and fr.dtype == np.float64)


def _values(rng, count):
    return rng.uniform(0.3, 1.0, count) * np.exp(1j * rng.uniform(0, 2 * np.pi, count))     # order 1, never 0, complex


def make_structure(n, k, W, seed, *, style, frame=True):
    """A padded row structure as a dict (n, k, width, cols, ops, vals: what ``SpmvStack`` takes; frame_im: n doubles in
    [-3, 3] or None), obeying include/midyn_spmv.h.

    style="pack": what ``pack_ell`` gives: groups ascending with the static part (index k) last, columns ascending inside a
    group, no duplicate (row, col, op), no stored zero, the last row with W slots where (k + 1) n >= W.
    style="contract": what the header allows and ``pack_ell`` never makes.  Where the sizes permit (stated per property):
    group order shuffled per row and the static group first in some row (k >= 2); columns unsorted (W >= 3, n >= 8);
    duplicate (row, col, op) slots (W >= 2); a stored zero with col != row (n >= 5, W >= 3); operator k - 1 without any
    slot (k >= 1); row n // 3 without any slot (n >= 2); the last row with all W slots; at least four distinct row lengths
    (n >= 5, W >= 3).  The properties are asserted here."""
    assert style in ("pack", "contract")
    rng = np.random.default_rng(seed)
    cols = np.repeat(np.arange(n, dtype=np.int32)[:, None], W, axis=1)
    ops = np.full((n, W), k, dtype=np.int32)
    vals = np.zeros((n, W), dtype=np.complex128)
    empty = n // 3 if n >= 2 else -1
    ramp = [1, 2, 3] + list(range(4, W))                          # the first rows: lengths 1, 2, 3, ... (then random)
    length = np.zeros(n, dtype=np.int64)
    given = 0
    for r in range(n):
        if r == empty:
            length[r] = 0
        elif r == n - 1:
            length[r] = W
        elif given < len(ramp):
            length[r] = min(ramp[given], W)
            given += 1
        else:
            length[r] = rng.integers(0, W + 1)
    if style == "pack":
        pairs = (k + 1) * n
        for r in range(n):
            take = min(int(length[r]), pairs)
            chosen = np.sort(rng.choice(pairs, size=take, replace=False))      # (op, col) pairs, by op then col
            ops[r, :take], cols[r, :take] = chosen // n, chosen % n
            vals[r, :take] = _values(rng, take)
            length[r] = take
    else:
        allowed = np.array([j for j in range(k + 1) if j != k - 1] if k >= 1 else [0])     # operator k - 1 owns no slot
        for r in range(n):
            ln = int(length[r])
            if ln == 0:
                continue
            drawn = rng.choice(allowed, size=ln)
            order = rng.permutation(allowed)
            if r == n - 1:                                        # the last row: static group first, with two slots
                drawn[:min(2, ln)] = k
                if ln >= 3:
                    drawn[2] = allowed[0]
                order = np.concatenate([[k], order[order != k]])
            row_ops = np.concatenate([np.full(int(np.sum(drawn == j)), j) for j in order]).astype(np.int32)
            ops[r, :ln] = row_ops
            cols[r, :ln] = rng.integers(0, n, ln)
            vals[r, :ln] = _values(rng, ln)
        if W >= 2:                                                # a duplicate (row, col, op): slots 0 and 1 of the last row
            cols[n - 1, 1] = cols[n - 1, 0]
        if n >= 5 and W >= 3:
            rz = int(np.flatnonzero((length >= 2) & (np.arange(n) != n - 1))[0])
            cols[rz, 0] = (rz + 1 + rng.integers(0, n - 1)) % n   # a stored zero off the diagonal, not in a last slot
            vals[rz, 0] = 0.0
    struct = dict(n=int(n), k=int(k), width=int(W), cols=np.ascontiguousarray(cols), ops=np.ascontiguousarray(ops),
                  vals=np.ascontiguousarray(vals), frame_im=rng.uniform(-3.0, 3.0, n) if frame else None, style=style)
    check_contract(struct)
    got = row_lengths(struct)
    assert np.array_equal(got, length), "a slot in use reads as unused (or the reverse)"
    if style == "pack":
        for r in range(n):
            key = ops[r, :got[r]].astype(np.int64) * n + cols[r, :got[r]]
            assert np.all(np.diff(key) > 0) and np.all(vals[r, :got[r]] != 0)
        assert got[n - 1] == min(W, (k + 1) * n)
    else:
        assert got[n - 1] == W
        if n >= 2:
            assert got[n // 3] == 0
        if k >= 1:
            assert not np.any(ops[np.arange(W)[None, :] < got[:, None]] == k - 1)
        if W >= 2:
            assert cols[n - 1, 0] == cols[n - 1, 1] and ops[n - 1, 0] == ops[n - 1, 1]
        if k >= 2 and W >= 3:
            assert ops[n - 1, 0] == k and np.any(ops[n - 1, :W] < k), "no row with the static group first"
        if k >= 2 and n >= 8 and W >= 3:
            assert any(np.any(np.diff(ops[r, :got[r]]) < 0) for r in range(n)), "no row with descending group order"
        if n >= 5 and W >= 3:
            assert len(set(got.tolist())) >= 4
            used = np.arange(W)[None, :] < got[:, None]
            assert np.any(used & (vals == 0) & (cols != np.arange(n)[:, None])), "no stored zero off the diagonal"
        if n >= 8 and W >= 3:
            assert any(ops[r, s] == ops[r, s + 1] and cols[r, s] > cols[r, s + 1] for r in range(n) for s in range(got[r] - 1)), \
                "no group with descending columns"
    return struct


# ---------------------------------------------------------------------------------------------------------------------
# the operation
# ---------------------------------------------------------------------------------------------------------------------
def _phase(struct, t, real_t, cplx_t):
    """e(t) = exp(i frame_im t) as a column, or None without a frame."""
    if struct["frame_im"] is None:
        return None
    arg = struct["frame_im"].astype(real_t) * real_t(t)
    return (np.cos(arg).astype(cplx_t) + cplx_t(1j) * np.sin(arg).astype(cplx_t))[:, None]


def _generator_times(struct, coef_cols, x, real_t, cplx_t, drop_last_slot=False):
    """(G_d' + sum_j c_j G_j) x for x of shape (n, C) and per-column coefficients coef_cols (k, C): ONE loop over the slots,
    every row at once.  The float64 run walks the slots last to first (the device walks them first to last)."""
    n, k, w = struct["n"], struct["k"], struct["width"]
    length = row_lengths(struct)
    if drop_last_slot and w > 0:
        length = np.where(length == length.max(), length - 1, length)
    weights = np.concatenate([np.asarray(coef_cols, dtype=real_t).reshape(k, x.shape[1]), np.ones((1, x.shape[1]), dtype=real_t)])
    vals = struct["vals"].astype(cplx_t)
    out = np.zeros(x.shape, dtype=cplx_t)
    slots = range(w) if real_t is np.longdouble else range(w - 1, -1, -1)
    for s in slots:
        live = (s < length)[:, None]
        term = weights[struct["ops"][:, s]] * (vals[:, s, None] * x[struct["cols"][:, s]])
        out = out + np.where(live, term, cplx_t(0))
    return out


def _rhs_between(struct, coef_cols, t_out, t_in, y, real_t, cplx_t, conj_out=True, drop_last_slot=False):
    """conj(e(t_out)) o [G (e(t_in) o y)]: the right-hand side when t_in == t_out."""
    e_in, e_out = _phase(struct, t_in, real_t, cplx_t), _phase(struct, t_out, real_t, cplx_t)
    g = _generator_times(struct, coef_cols, y if e_in is None else e_in * y, real_t, cplx_t, drop_last_slot)
    if e_out is None:
        return g
    return (np.conj(e_out) if conj_out else e_out) * g


def rhs(struct, coef, t, y, real_t, cplx_t):
    """out = conj(e(t)) o [(G_d' + sum_j c_j G_j)(e(t) o y)], e = exp(i frame_im t); y of shape (n,) or (n, m), coef (k,)."""
    y = np.asarray(y)
    y2 = y.reshape(struct["n"], -1).astype(cplx_t)
    k = struct["k"]
    coef_cols = np.repeat(np.asarray(coef if k else np.zeros(0), dtype=real_t).reshape(k, 1), y2.shape[1], axis=1)
    return _rhs_between(struct, coef_cols, t, t, y2, real_t, cplx_t).reshape(y.shape)


def rk4(struct, B, m, times, S, step_rows, step_h, step_save, P, y0, shared, real_t, cplx_t, mutant=None):
    """Classic RK4 over the step tables of midyn_spmv_rk4_solve; returns the block [B][P][n][m] (slot 0 = y0, a slot no step
    saves into is left 0).  Step s: stages at times[step_rows[s]] (never t + h / 2), coefficients S[b, step_rows[s]], step
    size step_h[s]; the new state goes to slot step_save[s] when that is >= 1.  ``mutant`` (float64 only) selects one of
    MUTANTS."""
    assert mutant is None or (mutant in MUTANTS and real_t is np.float64)
    n, k = struct["n"], struct["k"]
    C = B * m
    times = np.asarray(times, dtype=np.float64)
    step_rows = np.asarray(step_rows, dtype=np.int64).reshape(-1, 3)
    y0 = np.asarray(y0, dtype=np.complex128)
    assert y0.shape == ((n, m) if shared else (B, n, m))
    per_instance = np.broadcast_to(y0, (B, n, m)) if shared else y0
    if mutant == "y0_instance0":
        per_instance = np.broadcast_to(per_instance[0], (B, n, m))
    y = per_instance.transpose(1, 0, 2).reshape(n, C).astype(cplx_t)          # column c = b m + j
    out = np.zeros((B, P, n, m), dtype=cplx_t)
    out[:, 0] = np.broadcast_to(y0, (B, n, m)) if shared else y0
    flat = out.reshape(-1)

    def coef(row):
        if k == 0:
            return np.zeros((0, C), dtype=real_t)
        table = np.asarray(S, dtype=np.float64)[:, row, :]                    # (B, k)
        if mutant == "coef_instance0":
            table = np.broadcast_to(table[:1], table.shape)
        return np.repeat(table.T.astype(real_t), m, axis=1)

    def f(row_coef, t_out, t_in, x):
        return _rhs_between(struct, coef(row_coef), t_out, t_in, x, real_t, cplx_t, conj_out=mutant != "no_conj_out",
                            drop_last_slot=mutant == "drop_last_slot")

    for st in range(len(step_rows)):
        r0, r1, r2 = (int(r) for r in step_rows[st])
        t0, t1, t2 = times[r0], times[r1], times[r2]
        h = real_t(step_h[st])
        # the time whose phase each stage INPUT carries (the device stores stage inputs already multiplied by it)
        in0, in1, in2 = t0, t1, t2
        if mutant == "phase_next_at_t":
            in1 = in2 = t0
        if mutant == "phase_next_step_from_r2" and st > 0:
            in0 = times[int(step_rows[st - 1][2])]
        k1 = f(r0, t0, in0, y)
        k2 = f(r1, t1, in1, y + (h / 2) * k1)
        k3 = f(r1, t1, in1, y + (h / 2) * k2)
        k4 = f(r1 if mutant == "stage4_coef_row1" else r2, t2, in2, y + h * k3)
        w3 = real_t(1 if mutant == "stage3_weight" else 2)
        y = y + (h / 6) * (k1 + 2 * k2 + w3 * k3 + k4)
        save = int(step_save[st])
        if save >= 1:
            assert save < P
            if mutant == "out_slot_stride_m1":                    # the result index as if m were 1 (stays inside the block)
                rows_i, cols_i = np.meshgrid(np.arange(n), np.arange(C), indexing="ij")
                flat[(cols_i * P + save) * n + rows_i] = y
            else:
                out[:, save] = y.reshape(n, B, m).transpose(1, 0, 2)
    return out


def defined_slots(step_save, P):
    """The slots of the result block the schedule defines: 0 and every slot a step saves into."""
    keep = np.zeros(P, dtype=bool)
    keep[0] = True
    keep[[int(s) for s in step_save if int(s) >= 1]] = True
    return keep


def tolerance(ref_ld, run_f64):
    """max(8 max|run_f64 - ref_ld|, 32 eps64 max|ref_ld|): eight times the rounding a correct float64 evaluation of this case
    carries (measured against the reference, never against the device; the margin covers the device's other summation
    grouping, FMA contraction and h * (1.0 / 6) for h / 6), with a floor for cases whose float64 run happens to be exact."""
    ref_ld = np.asarray(ref_ld, dtype=np.clongdouble)
    spread = float(np.max(np.abs(np.asarray(run_f64).astype(np.clongdouble) - ref_ld))) if ref_ld.size else 0.0
    scale = float(np.max(np.abs(ref_ld))) if ref_ld.size else 0.0
    return max(8.0 * spread, 32.0 * EPS64 * scale)


def max_abs_diff(got, ref_ld):
    """max|got - ref| with the difference taken in extended precision."""
    ref_ld = np.asarray(ref_ld, dtype=np.clongdouble)
    return float(np.max(np.abs(np.asarray(got).astype(np.clongdouble) - ref_ld))) if ref_ld.size else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------
STEP_H = (0.02, -0.01, 0.0, 0.05, 0.03, -0.04, 0.01, 0.025)       # sign and size change from step to step; one step of length 0


def make_schedule(seed, nsteps, t_start, saves, spare_rows=2):
    """Step tables the contract allows and the scheduler never makes: every step has three table rows of its own, the rows
    lie in the table in shuffled order (with ``spare_rows`` rows no step uses), every second step starts 0.0625 after the
    end of the step before (so a step's first row is never the previous step's last row, in index and often in time).
    saves: {step number (1-based): slot}.  Returns times (R,), step_rows (nsteps, 3), step_h, step_save."""
    rng = np.random.default_rng(seed)
    R = 3 * nsteps + spare_rows
    place = rng.permutation(R)
    times = rng.uniform(t_start - 1.0, t_start + 1.0, R)          # (the spare rows keep these values)
    step_rows = np.zeros((nsteps, 3), dtype=np.int32)
    step_h = np.array([STEP_H[s % len(STEP_H)] for s in range(nsteps)], dtype=np.float64)
    step_save = np.full(nsteps, -1, dtype=np.int32)
    t = float(t_start)
    for s in range(nsteps):
        if s % 2 == 1:
            t += 0.0625
        step_rows[s] = place[3 * s:3 * s + 3]
        times[step_rows[s]] = (t, t + 0.5 * step_h[s], t + step_h[s])
        t = t + step_h[s]
        step_save[s] = saves.get(s + 1, -1)
    return times, step_rows, step_h, step_save


def _states(rng, shape):
    y = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    return y / np.sqrt(2.0 * shape[-2])                          # columns of norm about 1


def _rk4_case(tag, n, k, W, B, m, shared, *, seed, frame=True, t_start=0.3, nsteps=8, P=4, saves=None, style="contract"):
    struct = make_structure(n, k, W, seed, style=style, frame=frame)
    rng = np.random.default_rng(seed + 1)
    saves = {2: 1, 5: 2, 8: 3} if saves is None else saves
    times, step_rows, step_h, step_save = make_schedule(seed + 2, nsteps, t_start, saves)
    S = rng.uniform(-1.0, 1.0, (B, len(times), k))
    y0 = _states(rng, (n, m) if shared else (B, n, m))
    return dict(tag=tag, struct=struct, B=B, m=m, times=times, S=S, step_rows=step_rows, step_h=step_h, step_save=step_save,
                P=P, y0=y0, shared=shared)


def _rk4_cases():
    cases = {"full": lambda: _rk4_case("full", 67, 3, 7, 22, 3, False, seed=100, t_start=1000.0)}
    for i, (b, m) in enumerate(((15, 1), (16, 1), (17, 1), (5, 3), (4, 4))):
        cases[f"threshold-{b}x{m}"] = lambda b=b, m=m, i=i: _rk4_case("threshold", 27, 2, 5, b, m, True, seed=200 + 10 * i)
    for i, (b, m) in enumerate(((63, 1), (64, 1), (65, 1), (129, 1), (43, 3))):
        cases[f"block_edge-{b}x{m}"] = lambda b=b, m=m, i=i: _rk4_case("block_edge", 27, 2, 5, b, m, False, seed=300 + 10 * i)
    for i, n in enumerate((1, 3, 5, 63, 64, 65, 130)):
        cases[f"rows_edge-n{n}"] = lambda n=n, i=i: _rk4_case("rows_edge", n, 2, 4, 3, 2, True, seed=400 + 10 * i)
    for i, (k, fr) in enumerate(((0, False), (0, True), (2, False), (2, True))):
        cases[f"w0-k{k}-{'frame' if fr else 'noframe'}"] = lambda k=k, fr=fr, i=i: _rk4_case("w0", 9, k, 0, 2, 2, False,
                                                                                            seed=500 + 10 * i, frame=fr)
    cases["k0_static_only"] = lambda: _rk4_case("k0_static_only", 27, 0, 5, 3, 2, True, seed=600, frame=False)
    cases["no_frame"] = lambda: _rk4_case("no_frame", 27, 3, 6, 22, 3, False, seed=700, frame=False)
    cases["slots"] = lambda: _rk4_case("slots", 27, 2, 5, 3, 2, True, seed=800, P=6, saves={2: 4, 4: 1, 7: 4})
    cases["slots-nsteps0"] = lambda: _rk4_case("slots", 27, 2, 5, 3, 2, True, seed=810, P=6, nsteps=0, saves={})
    return cases


_RK4_BUILDERS = _rk4_cases()
RK4_CASES = tuple(_RK4_BUILDERS)
EVAL_TIMES = (0.0, 0.37, -2.5, 1000.0)
EVAL_CASES = tuple(f"eval-n{n}-m{m}" for n in (27, 65) for m in (1, 2, 15, 16, 17, 64, 65))
_CACHE = {}


def _frozen(value):
    if isinstance(value, np.ndarray):
        value.setflags(write=False)
    elif isinstance(value, dict):
        for v in value.values():
            _frozen(v)
    return value


def rk4_case(name):
    """The inputs of one case of RK4_CASES with its reference block, its calibration block, the tolerance and the mask of
    compared elements: computed once, shared by every test, read-only."""
    if name not in _CACHE:
        c = _RK4_BUILDERS[name]()
        args = (c["struct"], c["B"], c["m"], c["times"], c["S"], c["step_rows"], c["step_h"], c["step_save"], c["P"], c["y0"],
                c["shared"])
        c["ref"] = rk4(*args, *LD)
        c["f64"] = rk4(*args, *F64)
        c["slots"] = defined_slots(c["step_save"], c["P"])
        c["tol"] = tolerance(c["ref"][:, c["slots"]], c["f64"][:, c["slots"]])
        c["spread"] = max_abs_diff(c["f64"][:, c["slots"]], c["ref"][:, c["slots"]])
        _CACHE[name] = _frozen(c)
    return _CACHE[name]


def rk4_mutant(name, mutant):
    c = rk4_case(name)
    return rk4(c["struct"], c["B"], c["m"], c["times"], c["S"], c["step_rows"], c["step_h"], c["step_save"], c["P"], c["y0"],
               c["shared"], *F64, mutant=mutant)


def eval_case(name):
    """One case of EVAL_CASES: a structure, coefficients, a state of m columns, and per time of EVAL_TIMES the reference,
    the calibration run and the tolerance."""
    if name not in _CACHE:
        n, m = (int(p[1:]) for p in name.split("-")[1:])
        struct = make_structure(n, 3, 6, 900 + n, style="contract")
        rng = np.random.default_rng(1000 + 7 * n + m)
        c = dict(struct=struct, m=m, coef=rng.uniform(-1.0, 1.0, 3), y=_states(rng, (n, m))[:, 0] if m == 1 else _states(rng, (n, m)))
        c["ref"] = [rhs(struct, c["coef"], t, c["y"], *LD) for t in EVAL_TIMES]
        c["f64"] = [rhs(struct, c["coef"], t, c["y"], *F64) for t in EVAL_TIMES]
        c["tol"] = [tolerance(r, f) for r, f in zip(c["ref"], c["f64"])]
        c["spread"] = [max_abs_diff(f, r) for r, f in zip(c["ref"], c["f64"])]
        for v in c["ref"] + c["f64"]:
            v.setflags(write=False)
        _CACHE[name] = _frozen(c)
    return _CACHE[name]
