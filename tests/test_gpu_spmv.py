"""Sparse-operator models (array_library="scipy_sparse") on the device: the gather kernels behind ``evaluate_rhs`` and the
RK4 solvers, under both lane mappings (ctx option ``spmv_lanes``: 1 = rows, 2 = columns), against the golden vectors, the
CPU oracle (on the ``.toarray()`` copies of the operators), the dense-input route and a SciPy-sparse RK4 restated here."""
import numpy as np
import pytest
from scipy import sparse

from conftest import assert_close
from oracle import dynamics_oracle as orc

pytestmark = pytest.mark.gpu

EVAL_TOL = 1e-12
SOLVE_TOL = 1e-9
LANES = (1, 2)


@pytest.fixture(scope="module")
def qd():
    import qiskit_dynamics_amd as q

    q.default_context()  # raises loudly when libmidyn / the GPU is missing
    return q


def _sweep_signals(qd, cfg, b, k, t_final):
    from qiskit_dynamics_amd import workloads

    amps, phases = workloads.sweep_parameters(b, k)
    return [qd.Signal(lambda t, a=a: a * np.exp(-((t - t_final / 2) ** 2) / (2 * 1.0**2)), nu, ph)
            for a, nu, ph in zip(amps, cfg["carrier"], phases)]


# ------------------------------------------------------------------------------------------------
# golden: the 6-qubit chain in the diagonal frame
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", LANES)
def test_cfg2_small_golden_sparse(qd, golden, lanes):
    from qiskit_dynamics_amd import workloads

    g = golden("cfg2_small")
    cfg = workloads.schrodinger_config(n_qubits=6, n_drives=6, t_final=1.0, max_dt=0.01)
    hm = qd.HamiltonianModel(static_operator=sparse.csr_matrix(cfg["h_d"]), operators=[sparse.csr_matrix(o) for o in cfg["ops"]],
                             signals=_sweep_signals(qd, cfg, 0, 6, 1.0), rotating_frame=np.diag(cfg["h_d"]).real.copy(),
                             array_library="scipy_sparse")
    assert hm.array_library == "scipy_sparse" and hm.dim == 64 and hm.stack.k == 6 and hm.stack.n == 64
    ctx = qd.default_context()
    with ctx.options(spmv_lanes=lanes):
        for i, t in enumerate((0.0, 0.37, 1.0)):
            assert_close(hm.evaluate_rhs(t, g["diag_yv"]), g["diag_rhs"][i], EVAL_TOL)
        assert_close(hm(0.37, g["diag_yv"]), g["diag_rhs"][1], EVAL_TOL)
    gen = hm.evaluate(0.37)
    assert sparse.issparse(gen) and gen.format == "csr"
    assert_close(gen.toarray(), g["diag_eval_t037"], EVAL_TOL)
    # getters: sparse matrices, the Hamiltonian operators as given, the static part with the frame subtracted
    assert all(sparse.issparse(o) for o in hm.operators) and sparse.issparse(hm.static_operator)
    assert_close(np.stack([o.toarray() for o in hm.operators]), cfg["ops"], 0)
    assert_close(hm.static_operator.toarray(), cfg["h_d"] - np.diag(np.diag(cfg["h_d"])), 1e-15)
    hm.in_frame_basis = True      # the frame basis is the identity
    with ctx.options(spmv_lanes=lanes):
        assert_close(hm.evaluate_rhs(0.37, g["diag_yv"]), g["diag_rhs"][1], EVAL_TOL)
    # chosen without being named when an operator is sparse
    auto = qd.HamiltonianModel(operators=[sparse.csr_matrix(o) for o in cfg["ops"]], signals=_sweep_signals(qd, cfg, 0, 6, 1.0))
    assert auto.array_library == "scipy_sparse" and auto.rotating_frame.frame_diag is None


# ------------------------------------------------------------------------------------------------
# randomised models against the oracle
# ------------------------------------------------------------------------------------------------
def _random_hermitian(rng, n, density):
    a = sparse.random(n, n, density=density, random_state=rng, format="csr", dtype=float)
    b = sparse.random(n, n, density=density, random_state=rng, format="csr", dtype=float)
    h = a + 1j * b
    return (h + h.conj().T).tocsr()


def _clear_row_and_column(mat, r):
    keep = sparse.diags(np.where(np.arange(mat.shape[0]) == r, 0.0, 1.0))
    out = (keep @ mat @ keep).tocsr()
    out.eliminate_zeros()
    return out


def _random_model(n, seed):
    """(H_d, [H_0, H_1 = 0, H_2], frame diagonal): sparse Hermitian, complex, rows of unequal length, row `n // 3` empty in
    every operator, one operator without any entry."""
    rng = np.random.default_rng(seed)
    density = 3.0 / n
    empty = n // 3
    h_d = _clear_row_and_column(_random_hermitian(rng, n, density) + sparse.diags(rng.uniform(-2, 2, n)), empty)
    ops = [_clear_row_and_column(_random_hermitian(rng, n, density), empty), sparse.csr_matrix((n, n), dtype=complex),
           _clear_row_and_column(_random_hermitian(rng, n, 0.5 * density), empty)]
    frame = rng.uniform(-3.0, 3.0, n)
    return h_d, ops, frame


def _signals(qd, b):
    """Three signals of instance b (envelope, carrier frequency, phase): deterministic, different per instance."""
    return [qd.Signal(lambda t, a=0.4 + 0.05 * (b % 7) + 0.1 * j: a * np.cos(0.7 * t + 0.1 * j) + 0j, 0.3 + 0.11 * j + 0.01 * b,
                      0.2 * j - 0.03 * b) for j in range(3)]


def _coeff_fn(sigs):
    return lambda t: np.array([np.real(s(t)) for s in sigs])


def _y0s(n, count, seed):
    rng = np.random.default_rng(seed)
    ys = rng.standard_normal((count, n)) + 1j * rng.standard_normal((count, n))
    return [y / np.linalg.norm(y) for y in ys]


FORWARD = dict(t_span=[0.0, 0.4], t_eval=[0.1, 0.25, 0.4], max_dt=0.01)      # 40 steps + one of length 0 (t_eval ends at t_span[1])
BACKWARD = dict(t_span=[1.0, 0.0], t_eval=[0.8, 0.2], max_dt=0.025)          # 40 steps, h < 0
# (n = 300: the oracle forms a dense 300 x 300 generator per evaluation, so 30 steps and few instances compared)
FORWARD_30 = dict(t_span=[0.0, 0.3], t_eval=[0.1, 0.25], max_dt=0.01)
BACKWARD_30 = dict(t_span=[0.6, 0.0], t_eval=[0.4, 0.1], max_dt=0.02)

# (n, instances, y0 shared, frame, static operator, operators, time grid, instances compared with the oracle (None: all))
SWEEPS = {
    "n27_b1": (27, 1, True, True, True, True, FORWARD, None),
    "n27_b3_backward": (27, 3, False, True, True, True, BACKWARD, None),
    "n27_b64": (27, 64, True, True, True, True, FORWARD, None),
    "n27_b65": (27, 65, False, True, True, True, FORWARD, None),
    "n27_b130": (27, 130, True, True, True, True, FORWARD, None),
    "n27_b3_noframe": (27, 3, False, False, True, True, FORWARD, None),
    "n27_b3_nostatic": (27, 3, True, True, False, True, FORWARD, None),
    "n27_b3_noops": (27, 3, False, True, True, False, FORWARD, None),
    "n300_b3": (300, 3, False, True, True, True, FORWARD_30, None),
    "n300_b65": (300, 65, True, True, True, True, FORWARD_30, (0, 63, 64)),      # (the ends of the 64-column blocks)
    "n300_b2_noframe_backward": (300, 2, True, False, True, True, BACKWARD_30, None),
}
_REFERENCE = {}


def _sweep_case(qd, tag):
    n, batch, shared, with_frame, with_static, with_ops, grid, check = SWEEPS[tag]
    h_d, ops, frame = _random_model(n, 1000 + n)
    frame = frame if with_frame else None
    sig_lists = [_signals(qd, b) for b in range(batch)] if with_ops else None
    y0 = _y0s(n, 1, 7)[0] if shared else _y0s(n, batch, 8)
    check = range(batch) if check is None else check
    if tag not in _REFERENCE:       # computed once, shared by the two lane mappings, never modified
        a_d, a, d, basis = orc.hamiltonian_model_build(h_d.toarray() if with_static else None,
                                                       np.stack([o.toarray() for o in ops]) if with_ops else None, frame)
        ref = {}
        for b in check:
            _, ref[b] = orc.solve_generator_model(a_d, a, d, basis, _coeff_fn(sig_lists[b]) if with_ops else None,
                                                  grid["t_span"], y0 if shared else y0[b], "RK4", grid["max_dt"],
                                                  t_eval=grid["t_eval"])
            ref[b].setflags(write=False)
        _REFERENCE[tag] = ref
    return h_d if with_static else None, ops if with_ops else None, frame, sig_lists, y0, grid, check, _REFERENCE[tag]


def test_random_model_shape_properties():
    """The n = 27 model has what the sweeps are meant to exercise (no device needed for this part)."""
    from qiskit_dynamics_amd._lib import pack_ell

    h_d, ops, frame = _random_model(27, 1027)
    p = pack_ell(27, (-1j * h_d - sparse.diags(1j * frame)).tocsr(), [-1j * o for o in ops])
    lengths = np.sum((p["vals"] != 0) | (p["ops"] != 3) | (p["cols"] != np.arange(27)[:, None]), axis=1)
    assert p["width"] % 4 != 0 and len(set(lengths.tolist())) > 3 and lengths[27 // 3] == 1    # (the frame's diagonal entry)
    assert ops[1].nnz == 0 and np.iscomplexobj(p["vals"]) and np.any(p["vals"].imag != 0) and np.any(p["vals"].real != 0)


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("tag", list(SWEEPS))
def test_rk4_sweep_against_the_oracle(qd, tag, lanes):
    h_d, ops, frame, sig_lists, y0, grid, check, ref = _sweep_case(qd, tag)
    solver = qd.Solver(static_hamiltonian=h_d, hamiltonian_operators=ops, rotating_frame=frame, array_library="scipy_sparse")
    ctx = qd.default_context()
    ctx.reset_counters()
    with ctx.options(spmv_lanes=lanes, profile=1):
        if sig_lists is None:
            res = solver.solve(t_span=grid["t_span"], y0=y0, method="RK4", max_dt=grid["max_dt"], t_eval=grid["t_eval"])
        else:
            res = solver.solve(t_span=grid["t_span"], y0=y0, signals=sig_lists, method="RK4", max_dt=grid["max_dt"],
                               t_eval=grid["t_eval"])
    assert isinstance(res, list) and len(res) == (len(sig_lists) if sig_lists else len(y0))
    assert ctx.counters("rhs_spmv")["launches"] > 0
    for b in check:
        assert res[b].route == "spmv"
        assert_close(res[b].t, np.asarray(grid["t_eval"], dtype=float), 0)
        assert_close(res[b].y, ref[b], SOLVE_TOL)


@pytest.mark.parametrize("lanes", LANES)
def test_single_solve_with_two_columns_and_generator_model(qd, lanes):
    """solve_lmde on one model: y0 of shape (n, 2), no t_eval (slot 0 = y0), and a GeneratorModel that is not anti-Hermitian."""
    n = 27
    h_d, ops, frame = _random_model(n, 1027)
    sigs = _signals(qd, 2)
    y0 = np.stack(_y0s(n, 2, 9), axis=1)
    ctx = qd.default_context()
    model = qd.HamiltonianModel(static_operator=h_d, operators=ops, signals=sigs, rotating_frame=frame, array_library="scipy_sparse")
    a_d, a, d, basis = orc.hamiltonian_model_build(h_d.toarray(), np.stack([o.toarray() for o in ops]), frame)
    t_ref, y_ref = orc.solve_generator_model(a_d, a, d, basis, _coeff_fn(sigs), [0.0, 0.3], y0, "RK4", 0.01)
    with ctx.options(spmv_lanes=lanes):
        r = qd.solve_lmde(model, [0.0, 0.3], y0, method="hip_RK4", max_dt=0.01)
        for t in (0.0, 0.21):
            assert_close(model.evaluate_rhs(t, y0), orc.generator_rhs(a_d, a, _coeff_fn(sigs)(t), d, basis, t, y0), EVAL_TOL)
    assert r.route == "spmv" and r.y.shape == (2, n, 2)
    assert_close(r.t, t_ref, 0)
    assert_close(r.y, y_ref, SOLVE_TOL)
    rng = np.random.default_rng(5)
    g_d = (sparse.random(n, n, density=0.1, random_state=rng) + 1j * sparse.random(n, n, density=0.1, random_state=rng)).tocsr()
    g_1 = (sparse.random(n, n, density=0.05, random_state=rng) * (1 - 2j)).tocsr()
    gm = qd.GeneratorModel(static_operator=g_d, operators=[g_1], signals=sigs[:1], rotating_frame=sparse.diags(1j * frame).tocsr())
    assert gm.array_library == "scipy_sparse"
    a_d, a, d, basis = orc.generator_model_build(g_d.toarray(), g_1.toarray()[None], 1j * frame)
    _, y_ref = orc.solve_generator_model(a_d, a, d, basis, _coeff_fn(sigs[:1]), [0.0, 0.3], y0[:, 0], "RK4", 0.01)
    with ctx.options(spmv_lanes=lanes):
        r = qd.solve_lmde(gm, [0.0, 0.3], y0[:, 0], method="RK4", max_dt=0.01)
    assert_close(r.y, y_ref, SOLVE_TOL)
    assert_close(gm.evaluate(0.21).toarray(), orc.generator_evaluate(a_d, a, _coeff_fn(sigs[:1])(0.21), d, basis, 0.21), EVAL_TOL)


def _n27_oracle():
    h_d, ops, frame = _random_model(27, 1027)
    return (h_d, ops, frame) + tuple(orc.hamiltonian_model_build(h_d.toarray(), np.stack([o.toarray() for o in ops]), frame))


@pytest.mark.parametrize("lanes", LANES)
def test_matrix_y0_with_a_signal_list_per_instance(qd, lanes):
    """Instances x columns together: y0 of shape (27, 3) shared by 22 instances with their own signals (66 state columns,
    instance 21 across the 64-column block boundary).  Every instance against the oracle."""
    n, batch = 27, 22
    h_d, ops, frame, a_d, a, d, basis = _n27_oracle()
    sig_lists = [_signals(qd, b) for b in range(batch)]
    y0 = np.stack(_y0s(n, 3, 19), axis=1)
    grid = dict(t_span=[0.0, 0.2], t_eval=[0.05, 0.13, 0.2], max_dt=0.01)
    solver = qd.Solver(static_hamiltonian=h_d, hamiltonian_operators=ops, rotating_frame=frame, array_library="scipy_sparse")
    with qd.default_context().options(spmv_lanes=lanes):
        res = solver.solve(y0=y0, signals=sig_lists, method="RK4", **grid)
    assert isinstance(res, list) and len(res) == batch
    for b in range(batch):
        _, y_ref = orc.solve_generator_model(a_d, a, d, basis, _coeff_fn(sig_lists[b]), grid["t_span"], y0, "RK4", grid["max_dt"],
                                             t_eval=grid["t_eval"])
        assert res[b].route == "spmv" and res[b].y.shape == (len(grid["t_eval"]), n, 3)
        assert_close(res[b].t, np.asarray(grid["t_eval"]), 0)
        assert_close(res[b].y, y_ref, SOLVE_TOL)


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("y0_kind", ["distinct_vectors", "distinct_matrices", "one_shared"])
def test_one_signal_list_repeated_for_five_instances(qd, lanes, y0_kind):
    """The same signal-list OBJECT for every instance: distinct y0 are folded into the columns of one problem, one shared
    y0 is solved once and replicated.  Against the oracle and against five separate solves; t_eval starts at t_span[0]."""
    n, batch = 27, 5
    h_d, ops, frame, a_d, a, d, basis = _n27_oracle()
    sigs = _signals(qd, 3)
    if y0_kind == "distinct_vectors":
        y0 = _y0s(n, batch, 23)
    elif y0_kind == "distinct_matrices":
        y0 = [np.stack(_y0s(n, 2, 30 + b), axis=1) for b in range(batch)]
    else:
        y0 = _y0s(n, 1, 29)[0]
    grid = dict(t_span=[0.1, 0.3], t_eval=[0.1, 0.17, 0.3], max_dt=0.01)
    solver = qd.Solver(static_hamiltonian=h_d, hamiltonian_operators=ops, rotating_frame=frame, array_library="scipy_sparse")
    with qd.default_context().options(spmv_lanes=lanes):
        res = solver.solve(y0=y0, signals=[sigs] * batch, method="RK4", **grid)
        alone = [solver.solve(y0=y0[b] if isinstance(y0, list) else y0, signals=sigs, method="RK4", **grid) for b in range(batch)]
    assert isinstance(res, list) and len(res) == batch
    for b in range(batch):
        y0_b = y0[b] if isinstance(y0, list) else y0
        _, y_ref = orc.solve_generator_model(a_d, a, d, basis, _coeff_fn(sigs), grid["t_span"], y0_b, "RK4", grid["max_dt"],
                                             t_eval=grid["t_eval"])
        assert res[b].route == "spmv" and res[b].y.shape == (3,) + y0_b.shape
        assert_close(res[b].t, np.asarray(grid["t_eval"]), 0)
        assert_close(res[b].y[0], y0_b, 1e-15)                       # (t_eval[0] == t_span[0]: slot 0)
        assert_close(res[b].y, y_ref, SOLVE_TOL)
        assert_close(res[b].y, alone[b].y, 1e-13)
    if y0_kind == "one_shared":                                      # replicated results are copies, not one array
        assert res[0].y is not res[1].y and not np.shares_memory(res[0].y, res[1].y)


def test_many_steps_of_a_small_system_stay_on_the_sparse_route(qd):
    """300 steps at n = 27: a dense HamiltonianModel of this size goes parallel in time automatically (products of dense step
    propagators); a sparse one is stepped by the gather kernels."""
    n = 27
    h_d, ops, frame = _random_model(n, 1027)
    sigs = _signals(qd, 4)
    y0 = _y0s(n, 1, 13)[0]
    model = qd.HamiltonianModel(static_operator=h_d, operators=ops, signals=sigs, rotating_frame=frame, array_library="scipy_sparse")
    a_d, a, d, basis = orc.hamiltonian_model_build(h_d.toarray(), np.stack([o.toarray() for o in ops]), frame)
    _, y_ref = orc.solve_generator_model(a_d, a, d, basis, _coeff_fn(sigs), [0.0, 0.3], y0, "RK4", 1e-3)
    r = qd.solve_lmde(model, [0.0, 0.3], y0, method="RK4", max_dt=1e-3)
    assert r.route == "spmv" and r.nfev == 4 * 300
    assert_close(r.y, y_ref, SOLVE_TOL)


@pytest.mark.parametrize("lanes", LANES)
def test_coefficient_table_made_on_the_device(qd, lanes, monkeypatch):
    """A sweep of piecewise-constant signals whose table is evaluated on the device (a ``SignalTable``: the solve receives a
    DEVICE pointer) gives what the host-evaluated table gives, and what the oracle gives."""
    from qiskit_dynamics_amd import solvers

    n = 27
    h_d, ops, frame = _random_model(n, 1027)
    rng = np.random.default_rng(21)
    sig_lists = [[qd.DiscreteSignal(0.0531, rng.uniform(-1, 1, 8), 0.0, 0.3 + 0.1 * j, 0.2 * b) for j in range(3)] for b in range(5)]
    y0 = _y0s(n, 1, 17)[0]
    solver = qd.Solver(static_hamiltonian=h_d, hamiltonian_operators=ops, rotating_frame=frame, array_library="scipy_sparse")
    kwargs = dict(t_span=[0.0, 0.4], y0=y0, signals=sig_lists, method="RK4", max_dt=0.01)
    made = []
    real_table = solvers.SignalTable
    monkeypatch.setattr(solvers, "SignalTable", lambda *a, **k: made.append(real_table(*a, **k)) or made[-1])
    with qd.default_context().options(spmv_lanes=lanes):
        monkeypatch.setattr(solvers, "DEVICE_SIGNAL_TABLE_MIN", 1)
        on_device = solver.solve(**kwargs)
        assert len(made) == 1, "the coefficient table was not made on the device"
        monkeypatch.setattr(solvers, "DEVICE_SIGNAL_TABLE_MIN", 1 << 40)
        on_host = solver.solve(**kwargs)
        assert len(made) == 1
    a_d, a, d, basis = orc.hamiltonian_model_build(h_d.toarray(), np.stack([o.toarray() for o in ops]), frame)
    for b in (0, 4):
        assert_close(on_device[b].y, on_host[b].y, 1e-12)
        _, y_ref = orc.solve_generator_model(a_d, a, d, basis, _coeff_fn(sig_lists[b]), [0.0, 0.4], y0, "RK4", 0.01)
        assert_close(on_device[b].y, y_ref, SOLVE_TOL)


# ------------------------------------------------------------------------------------------------
# the dense-input route on the same model
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", LANES)
def test_sparse_and_dense_input_agree(qd, lanes):
    from qiskit_dynamics_amd import workloads

    cfg = workloads.schrodinger_config(n_qubits=6, n_drives=6, t_final=1.0, max_dt=0.01)
    scfg = workloads.schrodinger_config_sparse(n_qubits=6, n_drives=6, t_final=1.0, max_dt=0.01)
    frame = np.diag(cfg["h_d"]).real.copy()
    sig_lists = [_sweep_signals(qd, cfg, b, 6, 1.0) for b in range(4)]
    dense = qd.Solver(static_hamiltonian=cfg["h_d"], hamiltonian_operators=cfg["ops"], rotating_frame=frame)
    sp = qd.Solver(static_hamiltonian=scfg["h_d"], hamiltonian_operators=scfg["ops"], rotating_frame=frame)
    assert sp.model.array_library == "scipy_sparse" and dense.model.array_library == "hip"
    want = dense.solve(t_span=[0.0, 0.5], y0=cfg["y0"], signals=sig_lists, method="RK4", max_dt=0.01)
    with qd.default_context().options(spmv_lanes=lanes):
        got = sp.solve(t_span=[0.0, 0.5], y0=cfg["y0"], signals=sig_lists, method="RK4", max_dt=0.01)
    assert all(r.route == "spmv" for r in got) and not any(r.route == "spmv" for r in want)
    for a, b in zip(got, want):
        assert_close(a.y, b.y, SOLVE_TOL)


# ------------------------------------------------------------------------------------------------
# beyond the dense ceiling: 13 qubits
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", LANES)
def test_13_qubits_against_a_scipy_sparse_rk4(qd, lanes):
    from qiskit_dynamics_amd import workloads

    h_d, ops, nu = workloads.chain_hamiltonian_sparse(13, 4)
    n = 1 << 13
    frame = h_d.diagonal().real.copy()
    sig_lists = [[qd.Signal(0.3 + 0.2 * b + 0.1 * j, nu[j], 0.4 * j - 0.2 * b) for j in range(4)] for b in range(3)]
    y0 = np.zeros(n, dtype=complex)
    y0[[0, 5, n - 1]] = np.array([0.6, 0.64j, -0.48])
    solver = qd.Solver(static_hamiltonian=h_d, hamiltonian_operators=ops, rotating_frame=frame, array_library="scipy_sparse")
    assert solver.model.stack.n == n and solver.model.stack.width == 12 + 4       # per row: 12 XX couplings + 4 drives (the frame cancels the diagonal)
    with qd.default_context().options(spmv_lanes=lanes):
        res = solver.solve(t_span=[0.0, 0.1], y0=y0, signals=sig_lists, method="RK4", max_dt=0.01)
    g_d = (-1j * (h_d - sparse.diags(frame))).tocsr()
    g_ops = [(-1j * o).tocsr() for o in ops]
    for b, sigs in enumerate(sig_lists):
        coeff = _coeff_fn(sigs)

        def rhs(t, y, coeff=coeff):          # CSR generator per stage, in the frame: exp(-F t) o [C(t) (exp(F t) o y)]
            c = coeff(t)
            gen = g_d + sum(cj * gj for cj, gj in zip(c, g_ops))
            e = np.exp(1j * (-frame) * t)        # frame operator F = -i diag(frame): d = -i frame
            return e.conj() * (gen @ (e * y))

        y, t = y0, 0.0
        for _ in range(10):
            y = orc.rk4_step(rhs, t, y, 0.01)
            t = t + 0.01
        assert res[b].route == "spmv"
        assert_close(res[b].y[-1], y, SOLVE_TOL)
        assert abs(np.linalg.norm(res[b].y[-1]) - 1.0) <= SOLVE_TOL


# ------------------------------------------------------------------------------------------------
# scipy's adaptive methods with the sparse device RHS
# ------------------------------------------------------------------------------------------------
def test_dop853_against_the_oracle(qd):
    n = 27
    h_d, ops, frame = _random_model(n, 1027)
    sigs = _signals(qd, 1)
    y0 = _y0s(n, 1, 11)[0]
    model = qd.HamiltonianModel(static_operator=h_d, operators=ops, signals=sigs, rotating_frame=frame, array_library="scipy_sparse")
    a_d, a, d, basis = orc.hamiltonian_model_build(h_d.toarray(), np.stack([o.toarray() for o in ops]), frame)
    _, y_ref = orc.solve_generator_model(a_d, a, d, basis, _coeff_fn(sigs), [0.0, 1.0], y0, "RK4", 1e-3)
    r = qd.solve_lmde(model, [0.0, 1.0], y0, method="DOP853", atol=1e-10, rtol=1e-10)
    assert_close(r.y[-1], y_ref[-1], 5e-8)


# ------------------------------------------------------------------------------------------------
# error surface
# ------------------------------------------------------------------------------------------------
def test_error_surface(qd):
    n = 27
    h_d, ops, frame = _random_model(n, 1027)
    sigs = _signals(qd, 0)
    with pytest.raises(qd.DynamicsError, match="diagonal"):
        qd.HamiltonianModel(static_operator=h_d, operators=ops, rotating_frame=h_d, array_library="scipy_sparse")
    with pytest.raises(qd.DynamicsError, match="diagonal"):
        qd.HamiltonianModel(static_operator=h_d, operators=ops, rotating_frame=h_d.toarray(), array_library="scipy_sparse")
    with pytest.raises(qd.DynamicsError):
        qd.LindbladModel(static_hamiltonian=h_d, hamiltonian_operators=ops, static_dissipators=[ops[0]],
                         array_library="scipy_sparse")
    with pytest.raises(qd.DynamicsError):
        qd.Solver(static_hamiltonian=h_d, hamiltonian_operators=ops, static_dissipators=[ops[0]], array_library="scipy_sparse")
    with pytest.raises(qd.DynamicsError, match="Hermitian"):
        qd.HamiltonianModel(operators=[sparse.csr_matrix(np.triu(np.ones((n, n)), 1))], array_library="scipy_sparse")
    model = qd.HamiltonianModel(static_operator=h_d, operators=ops, signals=sigs, rotating_frame=frame, array_library="scipy_sparse")
    y0 = _y0s(n, 1, 3)[0]
    for method in ("scipy_expm", "hip_expm_parallel", "jax_RK4_parallel"):
        with pytest.raises(qd.DynamicsError, match="dense"):
            qd.solve_lmde(model, [0.0, 0.1], y0, method=method, max_dt=0.01)
    with pytest.raises(qd.DynamicsError):
        model.signals = sigs[:2]                                     # a signal list of the wrong length
    solver = qd.Solver(static_hamiltonian=h_d, hamiltonian_operators=ops, rotating_frame=frame, array_library="scipy_sparse")
    with pytest.raises(qd.DynamicsError):
        solver.solve(t_span=[0.0, 0.1], y0=y0, signals=sigs[:2], method="RK4", max_dt=0.01)
    with pytest.raises(qd.DynamicsError):
        solver.solve(t_span=[0.0, 0.1], y0=y0[:-1], signals=sigs, method="RK4", max_dt=0.01)   # y0 of the wrong dimension
    with pytest.raises(qd.DynamicsError):
        model.evaluate_rhs(0.1, y0[:-1])
    from qiskit_dynamics_amd import _lib

    packed = _lib.pack_ell(4, None, [sparse.identity(4, format="csr")])
    for field, value in (("cols", 4), ("cols", -1), ("ops", 2), ("ops", -1)):
        bad = dict(packed)
        bad[field] = packed[field].copy()
        bad[field][2, 0] = value                                     # the C side re-checks every slot
        with pytest.raises(qd.DynamicsError, match="outside"):
            _lib.SpmvStack(qd.default_context(), 4, 1, bad, None)
