"""Table of one tools/pmc_mirror.sh run: `python tools/pmc_mirror_report.py profile_out/<tag>` prints markdown.

Clock (bench.py `value` of the plain runs), rocprofv3 kernel-trace means of the mirrored pair and of the ablation kernels, the
counters of combine_mirror_kernel<0, 2>, and cycles per wave and kk step against the pipe model of DESIGN 4.15.
Counter units (gfx950): SQ_WAVE_CYCLES / SQ_WAIT_* / SQ_ACTIVE_INST_* are used as shares of SQ_WAVE_CYCLES only,
SQ_VALU_MFMA_BUSY_CYCLES counts cycles, FETCH_SIZE / WRITE_SIZE are reported in KB and read half of the bytes moved (x 2).
"""
import glob
import json
import os
import sqlite3
import sys

CLOCK_GHZ = 2.364          # sustained on fp64 MFMAs with random operands (profiles/r06_bench_detail.json)
WAVE_STEPS = 1024          # two waves per SIMD x 512 kk steps (n = 1024: 32 U blocks of 16)
MODEL = 885                # cycles per wave and kk step: 8 MFMA x 64 + 64 FMA x 5.13 + reduce-scatter 45


def dbs(root, d):
    return sorted(glob.glob(os.path.join(root, d, "*.db")) + glob.glob(os.path.join(root, d, "*", "*.db")))


def trace(root, d):
    out = {}
    for db in dbs(root, d):
        con = sqlite3.connect(db)
        for name, n, mean, lo, hi in con.execute("select name, count(*), avg(duration), min(duration), max(duration) from kernels group by name"):
            if "mirror" in name and "defect" not in name:
                out[name.replace("midyn::", "").replace("void ", "").split("(")[0]] = (n, mean / 1e3, lo / 1e3, hi / 1e3)
        con.close()
    return out


def counters(root, d):
    out = {}
    for db in dbs(root, d):
        con = sqlite3.connect(db)
        rows = con.execute("select dispatch_id, counter_name, sum(counter_value) from pmc_events "
                           "where name like '%combine_mirror_kernel%' group by dispatch_id, counter_name").fetchall()
        con.close()
        per = {}
        for _, cname, v in rows:
            per.setdefault(cname, []).append(v)
        for cname, xs in per.items():
            out[cname] = (len(xs), sum(xs) / len(xs))
    return out


def main():
    root = sys.argv[1]
    print(f"## {os.path.basename(os.path.normpath(root))}\n")
    if os.path.exists(os.path.join(root, "chain_status.txt")):
        print(open(os.path.join(root, "chain_status.txt")).read().strip() + "\n")
    print("| plain run | value (RHS evals/s) |\n|---|---|")
    for f in sorted(glob.glob(os.path.join(root, "bench_abl*.json"))):
        try:
            v = json.loads(open(f).read().strip().splitlines()[-1])["value"]
            print(f"| {os.path.basename(f)} | {v:.0f} |")
        except Exception as exc:  # noqa: BLE001
            print(f"| {os.path.basename(f)} | (no result: {exc}) |")
    print("\n| trace | kernel | launches | mean us | min | max | cycles per wave-step | of the model (885) |\n|---|---|---|---|---|---|---|---|")
    for d in ("stats", "stats_abl1", "stats_abl2", "stats_abl3"):
        for name, (n, mean, lo, hi) in sorted(trace(root, d).items()):
            cyc = mean * 1e3 * CLOCK_GHZ / WAVE_STEPS
            main_k = "finish" not in name
            print(f"| {d} | `{name}` | {n} | {mean:.1f} | {lo:.1f} | {hi:.1f} | " + (f"{cyc:.0f} | {MODEL / cyc:.2f} |" if main_k else "| |"))
    print("\n| counter of `combine_mirror_kernel<0, 2>` | dispatches | mean per dispatch |\n|---|---|---|")
    c = {}
    for d in ("pmc_wait", "pmc_valu", "pmc_tcc", "pmc_fetch", "pmc_write"):
        got = counters(root, d)
        if not got:
            print(f"| ({d}: no database) | | |")
        for cname, (n, v) in sorted(got.items()):
            c[cname] = v
            print(f"| {cname} | {n} | {v:.5g} |")
    print()
    if "SQ_WAVE_CYCLES" in c:
        w = c["SQ_WAVE_CYCLES"]
        print("Of SQ_WAVE_CYCLES: " + ", ".join(f"{k} {c[k] / w:.3f}" for k in ("SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY") if k in c)
              + f"; SQ_WAVE_CYCLES / (2048 waves x 512 steps) = {w / (2048 * 512):.0f} counter units per wave-step (compare the "
                "trace's cycles per wave-step for the unit on this ROCm; the three shares are unit-free).")
    if "SQ_VALU_MFMA_BUSY_CYCLES" in c:
        print(f"SQ_VALU_MFMA_BUSY_CYCLES per SIMD (1024 SIMDs): {c['SQ_VALU_MFMA_BUSY_CYCLES'] / 1024:.4g} cycles "
              f"(model: 1024 wave-steps x 512 = 524288).")
    if "TCC_HIT" in c and "TCC_MISS" in c:
        print(f"L2 hit rate {c['TCC_HIT'] / (c['TCC_HIT'] + c['TCC_MISS']):.3f}.")
    for k in ("FETCH_SIZE", "WRITE_SIZE"):
        if k in c:
            print(f"{k} x 1024 B x 2 = {c[k] * 2048 / 1e6:.1f} MB per launch.")


if __name__ == "__main__":
    main()
