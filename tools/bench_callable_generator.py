"""solve_lmde with a generator given as a Python callable (include/midyn_gentable.h): where the time goes.

Per case (n, steps, Magnus order, state columns m), all in one process:
  wall_ms      end-to-end solve_lmde(..., method="scipy_expm") (sampling + streaming + device + result)
  sample_ms    the host sampling alone: the same callable at the same times, validated, no device
  device_ms    HIP-event time of the device pipeline alone: the same rows pushed from memory (ctx timer)
  chain_on_ms / chain_off_ms   end-to-end with ctx option gentable_chain 1 / 0, alternated
  oracle_ms    the CPU reference (oracle.expm_solve, scipy expm per step)
  max_dev      max |y - y_oracle|
and the target check wall <= 1.3 max(sample, device) + 2 ms.  Usage: python tools/bench_callable_generator.py [--reps 5]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [(16, 2000, 2, 1), (64, 2000, 2, 1), (128, 1000, 1, 1), (64, 500, 3, 64)]


def generator(n, seed=1):
    rng = np.random.default_rng(seed)
    parts = []
    for _ in range(2):
        a = (rng.uniform(-1, 1, (n, n)) + 1j * rng.uniform(-1, 1, (n, n))) / np.sqrt(n)
        parts.append(a - a.conj().T)
    a0, a1 = parts

    def gen(t):
        return a0 + np.cos(1.7 * t) * a1

    return gen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", type=str, default="", help="comma-separated case indices (default: all)")
    ap.add_argument("--no-oracle", action="store_true")
    args = ap.parse_args()
    import qiskit_dynamics_amd as qd
    from oracle import dynamics_oracle as orc
    from qiskit_dynamics_amd import _lib
    from qiskit_dynamics_amd.solvers import _cached_schedule, _magnus_points, validate_generator_sample

    ctx = qd.default_context()
    picks = [int(c) for c in args.cases.split(",")] if args.cases else range(len(CASES))
    rows_out = []
    for ci in picks:
        n, steps, mo, m = CASES[ci]
        gen = generator(n)
        rng = np.random.default_rng(n + m)
        y0 = rng.uniform(-1, 1, (n, m)) + 1j * rng.uniform(-1, 1, (n, m))
        y0 = y0[:, 0] if m == 1 else y0
        T = 1.0
        kw = dict(method="scipy_expm", max_dt=T / steps, magnus_order=mo)
        r = qd.solve_lmde(gen, [0.0, T], y0, **kw)          # warm-up (pool, schedule cache, code objects)
        sched = _cached_schedule([0.0, T], None, T / steps, ("magnus", mo), _magnus_points(mo))
        times = sched.times
        # host sampling alone
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            rows = np.empty((len(times), n, n), dtype=np.complex128)
            for j, t in enumerate(times):
                rows[j] = validate_generator_sample(gen(t), t, n)
            ts.append(time.perf_counter() - t0)
        sample_ms = 1e3 * min(ts)
        # device pipeline alone: the rows from memory, one push
        yd = np.ascontiguousarray(y0.reshape(n, -1))
        dev = []
        for _ in range(args.reps):
            ctx.synchronize()
            tab = _lib.GenTable(ctx, n, yd, len(times), sched.step_rows, sched.step_h, sched.step_save, sched.n_save, mo,
                                False)
            try:
                ctx.timer_start()
                tab.push(rows)
                dev.append(ctx.timer_stop())
                tab.finish()
            finally:
                tab.close()
        device_ms = min(dev)
        # end to end, chain on / off alternated
        walls = {1: [], 0: []}
        for _ in range(args.reps):
            for chain in (1, 0):
                with ctx.options(gentable_chain=chain):
                    t0 = time.perf_counter()
                    r = qd.solve_lmde(gen, [0.0, T], y0, **kw)
                    walls[chain].append(time.perf_counter() - t0)
        chunks = ctx.counters("gentable_info")
        wall_ms = 1e3 * min(walls[1])
        entry = dict(n=n, steps=steps, magnus_order=mo, m=m, rows=len(times), chunks=int(chunks["launches"]),
                     steps_per_chunk=int(chunks["ms"]), wall_ms=round(wall_ms, 3), sample_ms=round(sample_ms, 3),
                     device_ms=round(device_ms, 3), chain_on_ms=round(1e3 * min(walls[1]), 3),
                     chain_off_ms=round(1e3 * min(walls[0]), 3))
        entry["target_ms"] = round(1.3 * max(sample_ms, device_ms) + 2.0, 3)
        entry["target_met"] = bool(wall_ms <= entry["target_ms"])
        if not args.no_oracle:
            t0 = time.perf_counter()
            _, y_ref = orc.expm_solve(gen, [0.0, T], y0, T / steps, magnus_order=mo)
            entry["oracle_ms"] = round(1e3 * (time.perf_counter() - t0), 1)
            entry["max_dev"] = float(np.max(np.abs(r.y - y_ref)))
        rows_out.append(entry)
        print(json.dumps(entry), flush=True)
    hdr = ("n", "steps", "magnus_order", "m", "chunks", "wall_ms", "sample_ms", "device_ms", "target_ms", "target_met",
           "chain_on_ms", "chain_off_ms", "oracle_ms", "max_dev")
    print("| " + " | ".join(hdr) + " |")
    print("|" + "---|" * len(hdr))
    for e in rows_out:
        print("| " + " | ".join(str(e.get(k, "")) for k in hdr) + " |")


if __name__ == "__main__":
    main()
