# Counters of the quotient kernels at k = 17, ext_k = 19: counters-only rocprofv3 passes of
# tools/bench_quotient.py (no tracing alongside; one counter set per pass, each its own run),
# summarised per kernel by tools/pmc_quotient.py. Passes: a FETCH_SIZE, b WRITE_SIZE (KiB at the L2's
# memory side), c the SQ busy / wait / VALU set, d L2 hits and misses. FETCH_SIZE tallies a wide
# coalesced read at half its bytes on gfx950: the divide kernel of the same run reads h exactly once
# and calibrates it. Usage, from the repository root:
#   [PASSES="a b"] [OUT_ROOT=dir] bash tools/pmc_quotient.sh [tag]     (output under build/ by default)
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT_ROOT:-$R/build}/${1:-quotpmc}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
A="FETCH_SIZE"
B="WRITE_SIZE"
C="SQ_WAVES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_ACTIVE_INST_ANY"
D="TCC_HIT_sum TCC_MISS_sum"
for p in ${PASSES:-a b c d}; do
  eval CN=\$$(echo $p | tr a-d A-D)
  timeout -k 10 240 rocprofv3 --pmc $CN -d $OUT/pass_$p -o p --output-format csv -- python3 $R/tools/bench_quotient.py --reps 2 --mul-gps 1,1 --out $OUT/discard_$p.jsonl > $OUT/pass_$p.log 2>&1 || { echo quotient pmc pass $p failed; tail -5 $OUT/pass_$p.log; exit 3; }
done
cd $R
python3 tools/pmc_quotient.py $OUT > $OUT/quot_pmc.jsonl
cut -c1-600 $OUT/quot_pmc.jsonl
