#!/usr/bin/env python
"""RK4 sweeps on the sparse-operator route (array_library="scipy_sparse"): chain_hamiltonian_sparse in the diagonal frame.

For every (qubits, instances) pair: `--steps` RK4 steps through ``SpmvStack.rk4_solve`` with a prepared schedule and
coefficient table (no Python signal evaluation in the timed window), one warm-up call, `--repeats` timed calls between
HIP events on the context's stream (the call ends in a device synchronise and includes the table upload and the result
download; two save slots), and one further call with the `profile` option on, whose "rhs_spmv" counter is the time of the
stage kernels alone.  Reported: RHS evaluations per second (4 per step and instance) from the median call time, and the
bytes-per-stage model against the bandwidth the stage kernels achieved:

    bytes per stage = rows x columns x 16 B x (slots gathered + state reads and writes of the stage's epilogue)
                      + the operator structure read once per row and block of 64 columns (24 B per slot)

That model counts every gather; an element of the stage input is gathered by as many rows as its column has entries, and
all but the first of those reads can be served by L2 / the Infinity Cache.  The second figure ("compulsory") counts the
stage input once: what has to come from HBM when the state does not fit the caches.

`--dense-qubits Q` runs the same model at Q qubits through the dense-input route as well (operators as (k, n, n) arrays).
`--lanes-scan Q` times both lane mappings (ctx option spmv_lanes) at Q qubits over a range of column counts: the automatic
switch (SPMV_COLS_MIN in csrc/midyn_spmv.inc) is the smallest count from which the columns mapping is the faster one.

One JSON line per measurement on stdout; `--markdown FILE` also writes the tables.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import qiskit_dynamics_amd as qd  # noqa: E402
from qiskit_dynamics_amd import solvers, workloads  # noqa: E402

T_FINAL = 1.0


def build_sparse(n_qubits, n_drives):
    h_d, ops, nu = workloads.chain_hamiltonian_sparse(n_qubits, n_drives)
    t0 = time.perf_counter()
    model = qd.HamiltonianModel(static_operator=h_d, operators=ops, rotating_frame=h_d.diagonal().real.copy(),
                                array_library="scipy_sparse")
    return model, nu[:n_drives], time.perf_counter() - t0


def build_dense(n_qubits, n_drives):
    h_d, ops, nu = workloads.chain_hamiltonian(n_qubits, n_drives)
    t0 = time.perf_counter()
    model = qd.HamiltonianModel(static_operator=h_d, operators=ops, rotating_frame=np.diag(h_d).real.copy())
    return model, nu[:n_drives], time.perf_counter() - t0


def problem(model, carrier, instances, steps):
    sched = solvers._cached_schedule([0.0, T_FINAL], None, T_FINAL / steps, "rk4", solvers._rk4_points)
    k = len(carrier)
    amps = np.stack([workloads.sweep_parameters(b, k)[0] for b in range(instances)])
    phases = np.stack([workloads.sweep_parameters(b, k)[1] for b in range(instances)])
    table = np.ascontiguousarray(workloads.gaussian_coefficient_table(sched.times, amps, phases, carrier, T_FINAL))
    y0 = np.zeros((model.dim, 1), dtype=complex)
    y0[0, 0] = 1.0
    return sched, table, y0


def bytes_per_stage(stack, columns, lanes_cols):
    """The traffic model of one stage, (every gather counted, the stage input counted once): gathers + the epilogue's
    state traffic + the operator structure."""
    slots = stack.nnz / stack.n                      # slots gathered per row (unused slots are not visited)
    epilogue = 1 + 1 + 1.75 + 0.25                   # y read, x write, acc (write in stage 1, read + write in 2 and 3, read in 4), y write in stage 4
    element = stack.n * columns * 16.0
    blocks = -(-columns // 64) if lanes_cols else columns      # the rows mapping reads a row's structure once per column
    structure = stack.nnz * 24.0 * blocks
    return element * (slots + epilogue) + structure, element * (1 + epilogue) + structure


def measure(ctx, stack, sched, table, y0, instances, repeats):
    def call():
        return stack.rk4_solve(sched.times, table, sched.step_rows, sched.step_h, sched.step_save, sched.n_save, y0,
                               instances, True)

    out = call()                                      # warm-up: code objects, buffers of this shape in the pool
    norm = float(np.max(np.abs(np.linalg.norm(out[:, -1, :, 0], axis=1) - 1.0)))
    times = []
    for _ in range(repeats):
        ctx.timer_start()
        call()
        times.append(ctx.timer_stop())
    return times, norm


def stage_kernel_ms(ctx, stack, sched, table, y0, instances):
    ctx.reset_counters()
    with ctx.options(profile=1):
        stack.rk4_solve(sched.times, table, sched.step_rows, sched.step_h, sched.step_save, sched.n_save, y0, instances, True)
        c = ctx.counters("rhs_spmv")
    return c["ms"], int(c["launches"])


def run_sparse(ctx, model, carrier, n_qubits, instances, steps, repeats, lanes=0):
    stack = model.stack
    sched, table, y0 = problem(model, carrier, instances, steps)
    rec = dict(route="spmv", qubits=n_qubits, n=stack.n, width=stack.width, instances=instances, steps=steps, lanes=lanes)
    try:
        with ctx.options(spmv_lanes=lanes):
            times, norm = measure(ctx, stack, sched, table, y0, instances, repeats)
            kernel_ms, launches = stage_kernel_ms(ctx, stack, sched, table, y0, instances)
    except qd.DynamicsError as err:                    # the library's memory check: reported, not worked around
        if "device memory" not in str(err):
            raise
        rec.update(skipped=str(err))
        return rec
    cols_mapping = lanes == 2 or (lanes == 0 and instances >= 16)
    model_bytes, compulsory = (b * 4 * steps for b in bytes_per_stage(stack, instances, cols_mapping))
    med = float(np.median(times))
    rec.update(call_ms_median=med, call_ms_min=float(np.min(times)), call_ms_max=float(np.max(times)),
               rhs_evals_per_s=instances * 4 * steps / (med * 1e-3), stage_kernels_ms=kernel_ms, stage_launches=launches,
               model_gb_per_solve=model_bytes / 1e9, achieved_tb_per_s=model_bytes / (kernel_ms * 1e-3) / 1e12,
               compulsory_gb_per_solve=compulsory / 1e9, compulsory_tb_per_s=compulsory / (kernel_ms * 1e-3) / 1e12,
               norm_defect=norm)
    return rec


def run_dense(ctx, model, carrier, n_qubits, instances, steps, repeats):
    sched, table, y0 = problem(model, carrier, instances, steps)
    rec = dict(route="dense input", qubits=n_qubits, n=model.dim, instances=instances, steps=steps)
    try:
        times, norm = measure(ctx, model.stack, sched, table, y0, instances, repeats)
    except qd.DynamicsError as err:
        if "memory" not in str(err).lower():
            raise
        rec.update(skipped=str(err))
        return rec
    med = float(np.median(times))
    rec.update(call_ms_median=med, call_ms_min=float(np.min(times)), call_ms_max=float(np.max(times)),
               rhs_evals_per_s=instances * 4 * steps / (med * 1e-3), norm_defect=norm)
    return rec


def markdown(records):
    lines = ["| route | qubits | n | instances | lanes | call ms (median, min - max) | RHS evals/s | stage kernels ms | model GB (all gathers) | TB/s | compulsory GB | TB/s |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in records:
        if "skipped" in r:
            lines.append(f"| {r['route']} | {r['qubits']} | {r['n']} | {r['instances']} | {r.get('lanes', '')} | skipped: {r['skipped']} | | | | | | |")
            continue
        lines.append(f"| {r['route']} | {r['qubits']} | {r['n']} | {r['instances']} | {r.get('lanes', '')} | "
                     f"{r['call_ms_median']:.2f} ({r['call_ms_min']:.2f} - {r['call_ms_max']:.2f}) | {r['rhs_evals_per_s']:.3e} | "
                     + (f"{r['stage_kernels_ms']:.2f} | {r['model_gb_per_solve']:.2f} | {r['achieved_tb_per_s']:.2f} | "
                        f"{r['compulsory_gb_per_solve']:.2f} | {r['compulsory_tb_per_s']:.2f} |"
                        if "stage_kernels_ms" in r else " | | | | |"))
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--qubits", type=int, nargs="*", default=[12, 14, 16])
    ap.add_argument("--instances", type=int, nargs="*", default=[1, 64, 256, 1024])
    ap.add_argument("--drives", type=int, default=8)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dense-qubits", type=int, default=0)
    ap.add_argument("--lanes-scan", type=int, default=0, help="qubit count of the lane-mapping scan (0: none)")
    ap.add_argument("--scan-columns", type=int, nargs="*", default=[1, 2, 4, 8, 16, 32, 64, 128])
    ap.add_argument("--markdown", default="")
    args = ap.parse_args()
    ctx = qd.default_context()
    records = []

    def emit(rec):
        records.append(rec)
        print(json.dumps(rec), flush=True)

    for q in args.qubits:
        model, carrier, build_s = build_sparse(q, args.drives)
        print(json.dumps(dict(event="model", route="spmv", qubits=q, build_s=build_s, device_bytes=model.stack.device_bytes,
                              nnz=model.stack.nnz)), flush=True)
        for b in args.instances:
            emit(run_sparse(ctx, model, carrier, q, b, args.steps, args.repeats))
        if q == args.lanes_scan:
            for b in args.scan_columns:
                for lanes in (1, 2):
                    emit(run_sparse(ctx, model, carrier, q, b, args.steps, args.repeats, lanes=lanes))
        model.stack.close()
    if args.dense_qubits:
        model, carrier, build_s = build_dense(args.dense_qubits, args.drives)
        print(json.dumps(dict(event="model", route="dense input", qubits=args.dense_qubits, build_s=build_s)), flush=True)
        for b in args.instances:
            emit(run_dense(ctx, model, carrier, args.dense_qubits, b, args.steps, args.repeats))
    if args.markdown:
        with open(args.markdown, "w") as f:
            f.write(markdown(records))


if __name__ == "__main__":
    main()
