"""The mirrored combine route (csrc/midyn_combine_mirror.h) after the stage input moved to LDS and the fragment ring grew:

  * the headline stack (n = 1024, 8 imaginary planes) at 4096 instances, a few RK4 steps: the default route against
    combine_mirror = 0 within the 1e-13 of tests/test_gpu_combine_mirror.py, and two runs of the default route equal bit for
    bit (every sum has a fixed order: no atomics);
  * a fresh process that launches an n = 256 stack (4 waves per workgroup, 80 KB of LDS) BEFORE the n = 1024 one (8 waves,
    144 KB): the dynamic-LDS limit of the kernel is raised once per device and variant, to the most a launch can ask for, and
    not to the size of whichever launch comes first.

Both need a real MI355X (`pytest -m gpu`).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, assert_close

pytestmark = pytest.mark.gpu


def _headline(qd, nb):
    from qiskit_dynamics_amd import workloads

    cfg = workloads.schrodinger_config()
    solver = qd.Solver(static_hamiltonian=cfg["h_d"], hamiltonian_operators=cfg["ops"], rotating_frame=cfg["h_d"])
    sweeps = []
    for b in range(nb):
        amps, phases = workloads.sweep_parameters(b, 8)
        sweeps.append([qd.Signal(lambda t, a=a: a * np.exp(-((t - cfg["t_final"] / 2) ** 2) / 2.0), nu, ph)
                       for a, nu, ph in zip(amps, cfg["carrier"], phases)])
    rng = np.random.default_rng(1024)
    y0 = rng.normal(size=1024) + 1j * rng.normal(size=1024)
    return cfg, solver, sweeps, y0 / np.linalg.norm(y0)


def _run(qd, cfg, solver, sweeps, y0, steps, **options):
    ctx = qd.default_context()
    ctx.reset_counters()
    with ctx.options(profile=1, **options):
        res = solver.solve(t_span=[2.4, 2.4 + steps * cfg["max_dt"]], y0=y0, signals=sweeps, method="RK4", max_dt=cfg["max_dt"])
    return np.stack([r.y[-1] for r in res]), int(ctx.counters("combine_mirror")["launches"]), ctx.counters("mirror_finish")["launches"]


def test_headline_default_route_vs_unmirrored_and_bitwise_repeat():
    import qiskit_dynamics_amd as qd

    qd.default_context()
    cfg, solver, sweeps, y0 = _headline(qd, 4096)
    steps = 4
    mir, mirrored, finishes = _run(qd, cfg, solver, sweeps, y0, steps)
    assert mirrored == 1 and finishes == 4 * steps, (mirrored, finishes)
    ref, mirrored, finishes = _run(qd, cfg, solver, sweeps, y0, steps, combine_mirror=0)
    assert mirrored == 0 and finishes == 0, (mirrored, finishes)
    assert np.all(np.isfinite(mir))
    assert_close(mir, ref, 1e-13)
    again, mirrored, _ = _run(qd, cfg, solver, sweeps, y0, steps)
    assert mirrored == 1
    assert np.array_equal(mir, again)


_SMALL_THEN_LARGE = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import qiskit_dynamics_amd as qd
from qiskit_dynamics_amd.solvers import FixedStepSchedule, _rk4_points

ctx = qd.default_context()
rng = np.random.default_rng(11)
for n, batch, waves in ((256, 384, 4), (1024, 256, 8)):
    h = n // 2
    ops = []
    for _ in range(7):                      # seven imaginary planes: combine_mirror_kernel<0, 2>, the headline's variant
        b = rng.uniform(-1, 1, (h, h)) * 0.3
        a = np.zeros((n, n))
        a[:h, h:] = b
        a[h:, :h] = b.T
        ops.append(1j * a)
    stack = qd.Stack(ctx, np.array(ops), None, None)
    sched = FixedStepSchedule([0.0, 0.02], None, 0.01, _rk4_points)
    table = rng.uniform(-1, 1, (batch, len(sched.times), 7))
    y0 = rng.uniform(-1, 1, (batch, n, 1)) + 1j * rng.uniform(-1, 1, (batch, n, 1))
    out = {}
    for mirror in (2, 0):
        ctx.reset_counters()
        with ctx.options(profile=1, combine_sweep=0, combine=2, combine_mirror=mirror):
            out[mirror] = stack.rk4_solve(sched.times, table, sched.step_rows, sched.step_h, sched.step_save, sched.n_save, y0, batch, False)
        assert int(ctx.counters("combine_mirror")["launches"]) == (1 if mirror else 0), (n, mirror)
        if mirror:
            assert int(ctx.counters("combine_shape")["launches"]) == waves, (n, ctx.counters("combine_shape"))
            assert int(ctx.counters("combine_info")["ms"]) == 20, ctx.counters("combine_info")
    err = float(np.max(np.abs(out[2] - out[0])))
    assert np.all(np.isfinite(out[2])) and err <= 1e-13 * max(1.0, float(np.max(np.abs(out[0])))), (n, err)
    stack.close()
print("small-then-large ok")
"""


def test_small_stack_before_large_one_in_a_fresh_process(tmp_path):
    script = tmp_path / "small_then_large.py"
    script.write_text(_SMALL_THEN_LARGE)
    done = subprocess.run([sys.executable, "-s", str(script), ROOT], capture_output=True, text=True, timeout=600,
                          cwd=str(tmp_path), env=dict(os.environ))
    assert done.returncode == 0 and "small-then-large ok" in done.stdout, (done.returncode, done.stdout[-2000:], done.stderr[-4000:])
