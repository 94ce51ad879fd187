"""solve_lmde / scipy_expm_solver with a generator given as a Python callable G(t) (include/midyn_gentable.h): golden
vectors of the reference's scipy_expm_solver / RK4 propagators, every gen_chain_kernel instantiation against the CPU
oracle, the per-step fallback, chunk and push boundaries, errors, and the C-ABI from plain C.
All tests need a real MI355X: run with `pytest -m gpu`.
"""
import os
import subprocess

import numpy as np
import pytest
import scipy.linalg

from conftest import ROOT, assert_close

pytestmark = pytest.mark.gpu

SOLVE_TOL = 1e-9

# the (t_span, t_eval, max_dt) triples of the fixed_step.npz scipy_expm_solver / RK4 cases
GOLDEN_CASES = {
    "fw": ([0.0, 1.0], None, 0.1),
    "te": ([0.0, 1.0], [0.0, 0.33, 0.71, 1.0], 0.05),
    "bw": ([1.0, 0.0], [0.8, 0.2], 0.1),
}


@pytest.fixture(scope="module")
def qd():
    import qiskit_dynamics_amd as q

    q.default_context()  # raises loudly when libmidyn / the GPU is missing
    return q


@pytest.fixture(scope="module")
def ctx(qd):
    return qd.default_context()


@pytest.fixture(scope="module")
def fixed(golden):
    g = golden("fixed_step")
    g0, g1 = g["g0"], g["g1"]
    return g, (lambda t: g0 + np.cos(1.3 * t) * g1)


def crand(rng, *shape):
    return rng.uniform(-1, 1, shape) + 1j * rng.uniform(-1, 1, shape)


@pytest.mark.parametrize("tag", list(GOLDEN_CASES))
@pytest.mark.parametrize("mo", [1, 2, 3])
def test_golden_scipy_expm(qd, fixed, tag, mo):
    g, gen = fixed
    ts, te, mdt = GOLDEN_CASES[tag]
    n = g["y0"].shape[0]
    r = qd.solve_lmde(gen, ts, g["y0"], method="scipy_expm", t_eval=te, max_dt=mdt, magnus_order=mo)
    np.testing.assert_array_equal(r.t, g[f"expm{mo}_{tag}_t"])
    assert_close(r.y, g[f"expm{mo}_{tag}_y"], SOLVE_TOL)
    assert r.route == "generator_table" and r.device.startswith("hip:") and r.wall_s > 0
    from qiskit_dynamics_amd.solvers import _cached_schedule, _magnus_points
    assert r.nfev == len(_cached_schedule(ts, te, mdt, ("magnus", mo), _magnus_points(mo)).times)
    rm = qd.scipy_expm_solver(gen, ts, np.eye(n, dtype=complex), max_dt=mdt, t_eval=te, magnus_order=mo)
    np.testing.assert_array_equal(rm.t, g[f"expm{mo}_{tag}_t"])
    assert_close(rm.y, g[f"expm{mo}m_{tag}_y"], SOLVE_TOL)
    rh = qd.solve_lmde(gen, ts, g["y0"], method="hip_expm", t_eval=te, max_dt=mdt, magnus_order=mo)
    assert_close(rh.y, g[f"expm{mo}_{tag}_y"], SOLVE_TOL)
    for method in ("hip_expm_parallel", "jax_expm_parallel"):
        rp = qd.solve_lmde(gen, ts, g["y0"], method=method, t_eval=te, max_dt=mdt, magnus_order=mo)
        assert rp.route == "generator_table+parallel_in_time"
        np.testing.assert_array_equal(rp.t, g[f"expm{mo}_{tag}_t"])
        assert_close(rp.y, g[f"expm{mo}_{tag}_y"], SOLVE_TOL)
    rpm = qd.solve_lmde(gen, ts, np.eye(n, dtype=complex), method="hip_expm_parallel", t_eval=te, max_dt=mdt,
                        magnus_order=mo)
    assert_close(rpm.y, g[f"expm{mo}m_{tag}_y"], SOLVE_TOL)


@pytest.mark.parametrize("tag", list(GOLDEN_CASES))
def test_golden_rk4_parallel(qd, fixed, tag):
    g, gen = fixed
    ts, te, mdt = GOLDEN_CASES[tag]
    n = g["y0"].shape[0]
    for method in ("hip_RK4_parallel", "jax_RK4_parallel"):
        r = qd.solve_lmde(gen, ts, g["y0"], method=method, t_eval=te, max_dt=mdt)
        np.testing.assert_array_equal(r.t, g[f"rk4_{tag}_t"])
        assert_close(r.y, g[f"rk4_{tag}_y"], SOLVE_TOL)
    rm = qd.solve_lmde(gen, ts, np.eye(n, dtype=complex), method="hip_RK4_parallel", t_eval=te, max_dt=mdt)
    assert_close(rm.y, g[f"rk4m_{tag}_y"], SOLVE_TOL)


def _damped_generator(n, seed):
    """Random anti-Hermitian parts with time dependence + a small non-normal damping term (nothing relies on unitarity)."""
    rng = np.random.default_rng(seed)
    parts = []
    for _ in range(3):
        a = crand(rng, n, n) / np.sqrt(n)
        parts.append(a - a.conj().T)
    damp = 0.05 * crand(rng, n, n) / np.sqrt(n)
    a0, a1, a2 = parts

    def gen(t):
        return a0 + np.cos(2.1 * t) * a1 + (0.3 * t * t) * a2 - damp

    return gen


def _oracle(gen, ts, y0, mdt, mo, te=None):
    from oracle import dynamics_oracle as orc

    return orc.expm_solve(gen, ts, y0, mdt, t_eval=te, magnus_order=mo)


def _profiled(qd, ctx, fn):
    ctx.reset_counters()
    with ctx.options(profile=1):
        res = fn()
    return res, ctx.counters("gen_chain")["launches"], ctx.counters("gentable_info")["launches"]


@pytest.mark.parametrize("n,m", [(40, 1), (40, 16), (96, 1), (96, 16), (24, 24)])
def test_chain_variants_against_oracle(qd, ctx, n, m):
    """n_pad 64 / 128 x 1 / 16 columns: all four gen_chain_kernel instantiations, 300 Magnus-2 steps."""
    gen = _damped_generator(n, 100 + n + m)
    rng = np.random.default_rng(n * m)
    y0 = crand(rng, n) if m == 1 else crand(rng, n, m)
    ts, te, mdt = [0.0, 1.5], [0.4, 1.1], 0.005
    r, launches, chunks = _profiled(qd, ctx, lambda: qd.solve_lmde(gen, ts, y0, method="scipy_expm", t_eval=te,
                                                                    max_dt=mdt, magnus_order=2))
    assert launches == chunks >= 1, (launches, chunks)
    t_ref, y_ref = _oracle(gen, ts, y0, mdt, 2, te)
    np.testing.assert_array_equal(r.t, t_ref)
    assert_close(r.y, y_ref, SOLVE_TOL)


@pytest.mark.parametrize("n,m", [(200, 1), (40, 100)])
def test_per_step_fallback_against_oracle(qd, ctx, n, m):
    """n_pad 256, or more than 32 columns: one zgemm per step, no gen_chain launch."""
    gen = _damped_generator(n, 7 + n)
    rng = np.random.default_rng(n + m)
    y0 = crand(rng, n) if m == 1 else crand(rng, n, m)
    ts, mdt = [0.0, 1.5], 0.005
    r, launches, chunks = _profiled(qd, ctx, lambda: qd.solve_lmde(gen, ts, y0, method="scipy_expm", max_dt=mdt,
                                                                    magnus_order=2))
    assert launches == 0 and chunks >= 1
    _, y_ref = _oracle(gen, ts, y0, mdt, 2)
    assert_close(r.y, y_ref, SOLVE_TOL)


def test_chain_option_off_matches_default(qd, ctx):
    gen = _damped_generator(40, 3)
    y0 = crand(np.random.default_rng(3), 40, 16)
    kw = dict(method="scipy_expm", t_eval=[0.5, 1.0], max_dt=0.01, magnus_order=2)
    r_on, on, _ = _profiled(qd, ctx, lambda: qd.solve_lmde(gen, [0.0, 1.5], y0, **kw))
    with ctx.options(gentable_chain=0):
        r_off, off, _ = _profiled(qd, ctx, lambda: qd.solve_lmde(gen, [0.0, 1.5], y0, **kw))
    assert on >= 1 and off == 0
    assert_close(r_off.y, r_on.y, 1e-12)


@pytest.mark.parametrize("method", ["scipy_expm", "hip_expm_parallel", "hip_RK4_parallel"])
def test_small_chunks_match_one_chunk(qd, ctx, method):
    from qiskit_dynamics_amd.solvers import get_fixed_step_sizes

    gen = _damped_generator(24, 11)
    y0 = crand(np.random.default_rng(11), 24)
    kw = dict(method=method, t_eval=[0.3, 0.3, 0.8], max_dt=0.01, magnus_order=3)
    nsteps = int(np.sum(get_fixed_step_sizes([0.0, 1.0], kw["t_eval"], kw["max_dt"])[2]))
    one = qd.solve_lmde(gen, [0.0, 1.0], y0, **kw)
    assert ctx.counters("gentable_info")["launches"] == 1
    with ctx.options(gentable_chunk=7):
        small = qd.solve_lmde(gen, [0.0, 1.0], y0, **kw)
        assert ctx.counters("gentable_info")["launches"] == -(-nsteps // 7)
        assert ctx.counters("gentable_info")["ms"] == 7
    assert_close(small.y, one.y, 1e-12)


def test_push_granularity_gives_identical_results(qd, ctx):
    from qiskit_dynamics_amd import _lib
    from qiskit_dynamics_amd.solvers import FixedStepSchedule, _rk4_points

    gen = _damped_generator(12, 5)
    y0 = crand(np.random.default_rng(5), 12, 3)
    sched = FixedStepSchedule([0.0, 1.0], [0.25, 0.25, 0.6], 0.02, _rk4_points)
    rows = np.stack([gen(t) for t in sched.times])
    outs = []
    with ctx.options(gentable_chunk=5):
        for block in (1, len(rows)):
            tab = _lib.GenTable(ctx, 12, y0, len(rows), sched.step_rows, sched.step_h, sched.step_save, sched.n_save,
                                0, True)
            try:
                for r0 in range(0, len(rows), block):
                    tab.push(rows[r0:r0 + block])
                outs.append(tab.finish())
            finally:
                tab.close()
    np.testing.assert_array_equal(outs[0], outs[1])


def test_constant_generator_many_steps_bounded_staging(qd, ctx):
    rng = np.random.default_rng(17)
    a = crand(rng, 16, 16)
    A = 0.5 * (a - a.conj().T) - 0.01 * np.eye(16)
    y0 = crand(rng, 16)
    T = 4.0
    staging = {}
    with ctx.options(gentable_chunk=1000):
        for nsteps in (20000, 10000):
            r = qd.solve_lmde(lambda t: A, [0.0, T], y0, method="scipy_expm", max_dt=T / nsteps, magnus_order=1)
            assert r.nfev == nsteps
            staging[nsteps] = (ctx.counters("gentable_staging")["launches"], ctx.counters("gentable_staging")["ms"],
                               ctx.counters("gentable_info")["launches"])
            if nsteps == 20000:
                assert_close(r.y[-1], scipy.linalg.expm(T * A) @ y0, SOLVE_TOL)
    host20, dev20, chunks20 = staging[20000]
    assert chunks20 == 20 and staging[10000][2] == 10
    assert (host20, dev20) == staging[10000][:2]
    assert dev20 <= 2 * 1001 * 16 * 16 * 16 and host20 <= 3 * 1001 * 16 * 16 * 16


def _solve_ok(qd):
    r = qd.solve_lmde(lambda t: -1j * np.array([[0.0, 1.0], [1.0, 0.0]]), [0.0, 1.0], np.array([1.0, 0.0]),
                      method="scipy_expm", max_dt=0.1)
    assert_close(r.y[-1], np.array([np.cos(1.0), -1j * np.sin(1.0)]), SOLVE_TOL)


def test_errors_then_a_successful_solve(qd):
    g0 = -1j * np.diag([1.0, 2.0, 3.0])
    y0 = np.ones(3, dtype=complex)

    def wrong_shape(t):
        return g0 if t < 0.5 else np.zeros((2, 2))

    with pytest.raises(qd.DynamicsError, match=r"t=0\.5"):
        qd.solve_lmde(wrong_shape, [0.0, 1.0], y0, method="scipy_expm", max_dt=0.1)
    _solve_ok(qd)
    with pytest.raises(qd.DynamicsError, match="non-finite"):
        qd.solve_lmde(lambda t: g0 * (np.nan if t > 0.7 else 1.0), [0.0, 1.0], y0, method="hip_expm_parallel",
                      max_dt=0.1)
    _solve_ok(qd)
    with pytest.raises(qd.DynamicsError, match="magnus_order"):
        qd.solve_lmde(lambda t: g0, [0.0, 1.0], y0, method="scipy_expm", max_dt=0.1, magnus_order=4)
    _solve_ok(qd)
    with pytest.raises(qd.DynamicsError, match="max_dt"):
        qd.solve_lmde(lambda t: g0, [0.0, 1.0], y0, method="scipy_expm")
    _solve_ok(qd)
    with pytest.raises(qd.DynamicsError, match="atol"):
        qd.solve_lmde(lambda t: g0, [0.0, 1.0], y0, method="scipy_expm", max_dt=0.1, atol=1e-8)
    _solve_ok(qd)
    with pytest.raises(qd.DynamicsError, match="y0"):
        qd.solve_lmde(lambda t: g0, [0.0, 1.0], np.ones((3, 3, 2)), method="scipy_expm", max_dt=0.1)
    _solve_ok(qd)
    for method in ("RK4", "hip_RK4", "DOP853"):      # ODE methods stay refused for callables
        with pytest.raises(qd.DynamicsError, match="LMDE methods"):
            qd.solve_lmde(lambda t: g0, [0.0, 1.0], y0, method=method, max_dt=0.1)
        _solve_ok(qd)


def test_abi_errors_leave_the_context_usable(qd, ctx):
    from qiskit_dynamics_amd import _lib

    y0 = np.ones((2, 1), dtype=complex)
    rows = np.zeros((4, 3), dtype=np.int32)
    rows[:, :] = np.arange(4)[:, None]
    h, save = np.full(4, 0.25), np.array([-1, -1, -1, 1], dtype=np.int32)
    with pytest.raises(qd.DynamicsError, match="RK4"):
        _lib.GenTable(ctx, 2, y0, 4, rows, h, save, 2, 0, False)
    with pytest.raises(qd.DynamicsError, match="save slot"):
        _lib.GenTable(ctx, 2, y0, 4, rows, h, np.array([-1, -1, -1, 2], dtype=np.int32), 2, 1, False)
    G = np.zeros((4, 2, 2), dtype=complex)
    tab = _lib.GenTable(ctx, 2, y0, 4, rows, h, save, 2, 1, False)
    tab.push(G[:2])
    with pytest.raises(qd.DynamicsError, match="midyn_gentable_push: out-of-order"):
        ctx.check(ctx.lib.midyn_gentable_push(tab.handle, 3, 1, G.ctypes.data))
    with pytest.raises(qd.DynamicsError, match="only midyn_gentable_destroy"):
        tab.push(G[2:])
    tab.close()
    tab = _lib.GenTable(ctx, 2, y0, 4, rows, h, save, 2, 1, False)
    with pytest.raises(qd.DynamicsError, match="midyn_gentable_push: rows beyond"):
        tab.push(np.zeros((5, 2, 2), dtype=complex))
    tab.close()
    tab = _lib.GenTable(ctx, 2, y0, 4, rows, h, save, 2, 1, False)
    tab.push(G[:3])
    with pytest.raises(qd.DynamicsError, match="midyn_gentable_finish: only 3 of 4"):
        tab.finish()
    tab.close()
    _solve_ok(qd)


def test_c_abi_program(qd, tmp_path):
    from qiskit_dynamics_amd import _lib

    exe = tmp_path / "abi_gentable"
    src = os.path.join(ROOT, "tests", "abi_gentable.c")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-o", str(exe), src, "-ldl", "-lm"], check=True)
    p = subprocess.run([str(exe), _lib.HIP_RUNTIME, _lib.LIB_PATH], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "GENTABLE_OK" in p.stdout, p.stdout + p.stderr
