"""The mirrored COMBINE + APPLY contraction (csrc/midyn_combine_mirror.h: combine_mirror_kernel<NRE4, NIM4> + mirror_finish_kernel)
against the unmirrored kernel (ctx option combine_mirror = 0), the MFMA GEMM route (combine = 0) and the CPU oracle.

  * the headline: the product Solver of BASELINE configs[2] (n = 1024, k = 8 imaginary planes, parity sectors), 4096 instances:
    mirrored by default, every launch counted as "rhs_combine" with the counters of the unmirrored kernel's shape;
  * every shipped variant at n = 256 (combine_mirror = 2): operators that couple the two row halves only, with symmetric
    imaginary planes ("X drives"), antisymmetric real planes ("Y drives") or both;
  * the stacks and shapes that keep today's kernel: a static operator in the frame, a U,L block beyond the symmetry bound,
    2048 instances, random planes.
  * block-sparse couplings (a diagonal L,U block at n = 1024, a few coupled U columns at n = 256): U blocks that a set of L row
    groups, or every set, never reaches, after another stack has left its sums in the partial-sum memory.

All of them need a real MI355X (`pytest -m gpu`).
"""
import numpy as np
import pytest

from conftest import assert_close

pytestmark = pytest.mark.gpu

SOLVE_TOL = 1e-9


@pytest.fixture(scope="module")
def qd():
    import qiskit_dynamics_amd as q

    q.default_context()
    return q


# ---- the headline --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def headline(qd):
    from oracle import dynamics_oracle as orc
    from qiskit_dynamics_amd import workloads

    cfg = workloads.schrodinger_config()
    solver = qd.Solver(static_hamiltonian=cfg["h_d"], hamiltonian_operators=cfg["ops"], rotating_frame=cfg["h_d"])
    model = orc.hamiltonian_model_build(cfg["h_d"], cfg["ops"], cfg["h_d"])
    return cfg, solver, model


def _signals(qd, cfg, b, k=8):
    from qiskit_dynamics_amd import workloads

    amps, phases = workloads.sweep_parameters(b, k)
    return [qd.Signal(lambda t, a=a: a * np.exp(-((t - cfg["t_final"] / 2) ** 2) / 2.0), nu, ph)
            for a, nu, ph in zip(amps, cfg["carrier"], phases)]


def _oracle_final(cfg, model, b, t_span, y0):
    from oracle import dynamics_oracle as orc
    from qiskit_dynamics_amd import workloads
    from threadpoolctl import threadpool_limits

    a_d, a, d, basis = model
    amps, phases = workloads.sweep_parameters(b, 8)

    def coeffs(t):
        return workloads.gaussian_coefficient_table(np.array([t]), amps, phases, cfg["carrier"], cfg["t_final"])[0]

    with threadpool_limits(limits=8):
        _, yref = orc.solve_generator_model(a_d, a, d, basis, coeffs, t_span, y0, "RK4", cfg["max_dt"])
    return yref[-1]


COUNTERS = ("rhs_combine", "rhs_gemm", "rhs_blocks_gemm", "mirror_finish", "combine_info", "combine_shape", "combine_wave",
            "combine_mirror")


def _run(qd, solver, sweeps, t_span, y0, max_dt, **options):
    ctx = qd.default_context()
    ctx.reset_counters()
    with ctx.options(profile=1, **options):
        res = solver.solve(t_span=t_span, y0=y0, signals=sweeps, method="RK4", max_dt=max_dt)
    return np.stack([r.y[-1] for r in res]), {c: ctx.counters(c) for c in COUNTERS}


def test_headline_4096_instances_mirrored_vs_unmirrored_and_oracle(qd, headline):
    cfg, solver, model = headline
    nb = 4096
    t_span = [2.4, 2.5]
    sweeps = [_signals(qd, cfg, b) for b in range(nb)]
    rng = np.random.default_rng(1024)
    y0 = rng.normal(size=1024) + 1j * rng.normal(size=1024)
    y0 /= np.linalg.norm(y0)
    mir, cm = _run(qd, solver, sweeps, t_span, y0, cfg["max_dt"])
    assert int(cm["combine_mirror"]["launches"]) == 1, cm["combine_mirror"]
    assert 0 <= cm["combine_mirror"]["ms"] <= 16, cm["combine_mirror"]          # the stack's defect, in units of eps
    assert cm["rhs_combine"]["launches"] == 80 and cm["mirror_finish"]["launches"] == 80, cm
    assert cm["rhs_gemm"]["launches"] == 0 and cm["rhs_blocks_gemm"]["launches"] == 0, cm
    assert (int(cm["combine_shape"]["launches"]), int(cm["combine_shape"]["ms"])) == (8, 1), cm["combine_shape"]
    assert int(cm["combine_wave"]["launches"]) == 32, cm["combine_wave"]
    ref, cr = _run(qd, solver, sweeps, t_span, y0, cfg["max_dt"], combine_mirror=0)
    assert int(cr["combine_mirror"]["launches"]) == 0 and cr["mirror_finish"]["launches"] == 0, cr
    assert cr["rhs_combine"]["launches"] == 80 and int(cr["combine_wave"]["launches"]) == 64, cr
    assert_close(mir, ref, 1e-13)
    assert np.max(np.abs(np.linalg.norm(mir, axis=1) - 1.0)) < 1e-10
    for b in (0, 2047, 4095):
        assert_close(mir[b], _oracle_final(cfg, model, b, t_span, y0), SOLVE_TOL)


def test_headline_full_length_mirrored_vs_oracle(qd, headline):
    cfg, solver, model = headline
    nb = 4096
    sweeps = [_signals(qd, cfg, b) for b in range(nb)]
    full, c = _run(qd, solver, sweeps, cfg["t_span"], cfg["y0"], cfg["max_dt"])
    assert int(c["combine_mirror"]["launches"]) == 1 and c["rhs_combine"]["launches"] == 4000, c
    assert np.max(np.abs(np.linalg.norm(full, axis=1) - 1.0)) < 1e-8
    assert_close(full[4095], _oracle_final(cfg, model, 4095, cfg["t_span"], cfg["y0"]), SOLVE_TOL)


def test_headline_2048_instances_keep_the_unmirrored_kernel(qd, headline):
    cfg, solver, _ = headline
    sweeps = [_signals(qd, cfg, b) for b in range(2048)]
    _, c = _run(qd, solver, sweeps, [2.4, 2.42], cfg["y0"], cfg["max_dt"])
    assert int(c["combine_mirror"]["launches"]) == 0 and c["mirror_finish"]["launches"] == 0, c
    assert c["rhs_combine"]["launches"] > 0 and int(c["combine_wave"]["launches"]) == 64, c


# ---- every variant at n = 256 ----------------------------------------------------------------------------------------------------

def _coupling_ops(rng, n, kinds):
    """Operators that map each half of the rows to the other only: 'x' imaginary plane, symmetric; 'y' real plane, antisymmetric."""
    h = n // 2
    ops = []
    for kind in kinds:
        b = rng.uniform(-1, 1, (h, h)) * 0.3
        a = np.zeros((n, n))
        a[:h, h:] = b
        a[h:, :h] = b.T if kind == "x" else -b.T
        ops.append(1j * a if kind == "x" else a + 0j)
    return np.array(ops)


def _solve(qd, stack, sched, table, y0, batch, **options):
    ctx = qd.default_context()
    ctx.reset_counters()
    with ctx.options(profile=1, combine_sweep=0, **options):
        ys = stack.rk4_solve(sched.times, table, sched.step_rows, sched.step_h, sched.step_save, sched.n_save, y0, batch, False)
    return ys, {c: ctx.counters(c) for c in COUNTERS}


VARIANTS = [("xxx", (0, 1)), ("xxxxxxx", (0, 2)), ("yy", (1, 0)), ("yyyyyy", (2, 0)), ("xxyy", (1, 1)), ("xyxyxyxyxyxyxyxy", (2, 2))]


@pytest.mark.parametrize("kinds,variant", VARIANTS, ids=["%d%d" % v for _, v in VARIANTS])
@pytest.mark.parametrize("framed", [False, True])
def test_mirror_variant_vs_unmirrored_gemm_and_oracle(qd, kinds, variant, framed):
    from oracle import dynamics_oracle as orc
    from qiskit_dynamics_amd.solvers import FixedStepSchedule, _rk4_points

    ctx = qd.default_context()
    rng = np.random.default_rng(7 + 10 * variant[0] + variant[1])
    n, batch = 256, 384
    ops = _coupling_ops(rng, n, kinds)
    fim = rng.normal(size=n) if framed else None
    stack = qd.Stack(ctx, ops, None, fim)
    sched = FixedStepSchedule([0.0, 0.03], None, 0.01, _rk4_points)
    table = rng.uniform(-1, 1, (batch, len(sched.times), len(kinds)))
    y0 = rng.uniform(-1, 1, (batch, n, 1)) + 1j * rng.uniform(-1, 1, (batch, n, 1))
    mir, cm = _solve(qd, stack, sched, table, y0, batch, combine=2, combine_mirror=2)
    assert int(cm["combine_mirror"]["launches"]) == 1 and cm["mirror_finish"]["launches"] == 12, cm
    assert cm["rhs_combine"]["launches"] == 12, cm
    assert int(cm["combine_info"]["ms"]) == 100 * variant[0] + 10 * variant[1], cm["combine_info"]
    assert (int(cm["combine_shape"]["launches"]), int(cm["combine_shape"]["ms"])) == (4, 1), cm["combine_shape"]   # four L row groups: four waves
    ref, cr = _solve(qd, stack, sched, table, y0, batch, combine=2, combine_mirror=0)
    assert int(cr["combine_mirror"]["launches"]) == 0 and cr["mirror_finish"]["launches"] == 0, cr
    assert_close(mir, ref, 1e-13)
    gemm, cg = _solve(qd, stack, sched, table, y0, batch, combine=0)
    assert cg["rhs_combine"]["launches"] == 0
    assert_close(mir, gemm, 1e-13)
    d = None if fim is None else 1j * fim
    for b in (0, 200, 383):
        def rhs(t, y, b=b):
            row = int(np.argmin(np.abs(np.asarray(sched.times) - t)))
            return orc.generator_rhs(None, ops, table[b, row], d, None, t, y)

        _, yref = orc.rk4_solve(rhs, [0.0, 0.03], y0[b, :, 0], 0.01)
        assert_close(mir[b, -1, :, 0], yref[-1], 1e-11)
    stack.close()


# ---- stacks that keep today's kernel ---------------------------------------------------------------------------------------------

def _perturbed(rng, ops):
    ops = ops.copy()
    ops[0, 200, 10] += 1e-9
    return ops, None


def _static(rng, ops):
    n = ops.shape[1]
    h = rng.uniform(-1, 1, (n, n)) * 0.3
    return ops, 1j * (h + h.T)


def _random(rng, ops):
    a = rng.uniform(-1, 1, ops.shape) * 0.3
    return 1j * a + 0j, None


@pytest.mark.parametrize("make", [_perturbed, _static, _random], ids=["perturbed", "static", "random"])
def test_ineligible_stacks_keep_the_unmirrored_kernel(qd, make):
    from qiskit_dynamics_amd.solvers import FixedStepSchedule, _rk4_points

    ctx = qd.default_context()
    rng = np.random.default_rng(3)
    n, batch = 256, 384
    ops, static = make(rng, _coupling_ops(rng, n, "xxxx"))
    stack = qd.Stack(ctx, ops, static, None)
    sched = FixedStepSchedule([0.0, 0.02], None, 0.01, _rk4_points)
    table = rng.uniform(-1, 1, (batch, len(sched.times), 4))
    y0 = rng.uniform(-1, 1, (batch, n, 1)) + 1j * rng.uniform(-1, 1, (batch, n, 1))
    got, c = _solve(qd, stack, sched, table, y0, batch, combine=2, combine_mirror=2)
    assert int(c["combine_mirror"]["launches"]) == 0 and c["mirror_finish"]["launches"] == 0, c
    if make is not _static:      # (a stack with a static operator may take another route at this shape: only "not mirrored" is asserted)
        assert c["rhs_combine"]["launches"] == 8, c
    if make is _perturbed:
        assert c["combine_mirror"]["ms"] > 16, c["combine_mirror"]
    ref, _ = _solve(qd, stack, sched, table, y0, batch, combine=2, combine_mirror=0)
    assert np.array_equal(got, ref)
    stack.close()


# ---- block-sparse couplings: U blocks that a set of L row groups (or every set) never reaches ----------------------------------

def _sparse_coupling_ops(rng, n, kinds, pattern):
    """'blocks': the L,U block of every operator is block-diagonal with two n / 4 blocks (at n = 1024 each of the two workgroup
    sets of L row groups reaches half of the U blocks); 'cols': only the first n / 4 U columns are coupled (the other U rows have
    no contraction at all)."""
    h = n // 2
    ops = []
    for kind in kinds:
        b = np.zeros((h, h))
        q = h // 2
        if pattern == "blocks":
            b[:q, :q] = rng.uniform(-1, 1, (q, q)) * 0.3
            b[q:, q:] = rng.uniform(-1, 1, (q, q)) * 0.3
        else:
            b[:, :q] = rng.uniform(-1, 1, (h, q)) * 0.3
        a = np.zeros((n, n))
        a[:h, h:] = b
        a[h:, :h] = b.T if kind == "x" else -b.T
        ops.append(1j * a if kind == "x" else a + 0j)
    return np.array(ops)


@pytest.mark.parametrize("n,pattern", [(1024, "blocks"), (256, "cols")])
def test_block_sparse_coupling_after_another_stack(qd, n, pattern):
    """The partial-sum buffer of the U rows is written only where a set's walk reaches; the finishing kernel must add only those
    sets.  A dense stack of the same shape runs first and is released, so that the buffer of the sparse one is likely to hold
    its stale sums."""
    from oracle import dynamics_oracle as orc
    from qiskit_dynamics_amd.solvers import FixedStepSchedule, _rk4_points

    ctx = qd.default_context()
    rng = np.random.default_rng(n + len(pattern))
    batch, kinds = 256, "xxy"
    sched = FixedStepSchedule([0.0, 0.03], None, 0.01, _rk4_points)
    table = rng.uniform(-1, 1, (batch, len(sched.times), len(kinds)))
    y0 = rng.uniform(-1, 1, (batch, n, 1)) + 1j * rng.uniform(-1, 1, (batch, n, 1))
    dense = qd.Stack(ctx, _coupling_ops(rng, n, kinds), None, None)
    _, cd = _solve(qd, dense, sched, table, y0, batch, combine=2, combine_mirror=2)
    assert int(cd["combine_mirror"]["launches"]) == 1, cd
    dense.close()
    ops = _sparse_coupling_ops(rng, n, kinds, pattern)
    fim = rng.normal(size=n)
    stack = qd.Stack(ctx, ops, None, fim)
    mir, cm = _solve(qd, stack, sched, table, y0, batch, combine=2, combine_mirror=2)
    assert int(cm["combine_mirror"]["launches"]) == 1 and cm["mirror_finish"]["launches"] == 12, cm
    assert cm["rhs_combine"]["launches"] == 12, cm
    assert cm["combine_info"]["launches"] == (n // 32) * (n // 16) // 4, cm["combine_info"]      # half of the sector lists
    ref, cr = _solve(qd, stack, sched, table, y0, batch, combine=2, combine_mirror=0)
    assert int(cr["combine_mirror"]["launches"]) == 0
    assert np.all(np.isfinite(mir))
    assert_close(mir, ref, 1e-13)
    for b in (0, 255):
        def rhs(t, y, b=b):
            row = int(np.argmin(np.abs(np.asarray(sched.times) - t)))
            return orc.generator_rhs(None, ops, table[b, row], 1j * fim, None, t, y)

        _, yref = orc.rk4_solve(rhs, [0.0, 0.03], y0[b, :, 0], 0.01)
        assert_close(mir[b, -1, :, 0], yref[-1], 1e-11)
    stack.close()
