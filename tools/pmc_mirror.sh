#!/bin/bash
# The mirrored combine kernel (combine_mirror_kernel<0, 2> + mirror_finish_kernel) on the bench headline: clock, kernel trace,
# the profiling-only ablations (ctx option mirror_ablate, mirror_probe_kernel<1..3>) and hardware counters.
#   usage (on the GPU, from the repository root): bash tools/pmc_mirror.sh [tag]      -> profile_out/<tag>/mirror_latency.md
#   (MIDYN_PROFILE_OUT names another directory than profile_out/ for the outputs)
# Every GPU process runs under its own time limit and the chain stops at the first one that fails: nothing is tried twice.
# Counter passes are processes of their own with no tracing domain; the trace is a process of its own too (tracing slows the
# host, so `value` comes from the plain runs only).
TAG=${1:-mirror}
R=$(pwd)
O=${MIDYN_PROFILE_OUT:-$R/profile_out}/$TAG
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
B="python $R/bench.py --gpus 1 --steps 40 --warmup 16"
P="python $R/bench.py --gpus 1 --steps 3 --warmup 1"
T="timeout -k 10 300"
pmc() {  # pmc <dir> <counters...>
    local d=$1; shift
    $T rocprofv3 --pmc "$@" -d $O/$d -o v -- $P > $O/$d.log 2>&1
}
$T $B > $O/bench_abl0.json 2> $O/bench_abl0.err &&
$T $B > $O/bench_abl0b.json 2> $O/bench_abl0b.err &&
$T rocprofv3 --kernel-trace --stats -d $O/stats -o v -- $B > $O/stats.log 2>&1 &&
$T rocprofv3 --kernel-trace --stats -d $O/stats_abl1 -o v -- $B --opt mirror_ablate=1 > $O/stats_abl1.log 2>&1 &&
$T rocprofv3 --kernel-trace --stats -d $O/stats_abl2 -o v -- $B --opt mirror_ablate=2 > $O/stats_abl2.log 2>&1 &&
$T rocprofv3 --kernel-trace --stats -d $O/stats_abl3 -o v -- $B --opt mirror_ablate=3 > $O/stats_abl3.log 2>&1 &&
pmc pmc_wait SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY &&
pmc pmc_valu SQ_VALU_MFMA_BUSY_CYCLES SQ_ACTIVE_INST_VALU SQ_INSTS_VALU SQ_INSTS_LDS SQ_WAIT_INST_LDS &&
pmc pmc_tcc TCC_HIT TCC_MISS &&
pmc pmc_fetch FETCH_SIZE &&
pmc pmc_write WRITE_SIZE
echo "pmc_mirror: chain ended with status $?" | tee $O/chain_status.txt
python $R/tools/pmc_mirror_report.py $O > $O/mirror_latency.md 2>&1
find $O -name "*.db" -delete; find $O -name "*.csv" -size +1M -delete
cat $O/mirror_latency.md
