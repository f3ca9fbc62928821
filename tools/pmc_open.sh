# "A column with 12 queries is fetched once": one counters-only rocprofv3 pass (FETCH_SIZE, KiB at
# the L2's memory side; no tracing alongside) over tools/bench_open.py's evaluation of 10 columns at
# the chip's 67 gate queries and its 8-input combine, at k = 17, summarised per kernel by
# tools/pmc_open.py. FETCH_SIZE tallies a wide coalesced read at half its bytes on gfx950 (see
# tools/pmc_quotient.sh): the combine kernel of the same run reads each of its 8 columns exactly
# once and calibrates the evaluation kernel's figure. Usage, from the repository root:
#   [OUT_ROOT=dir] bash tools/pmc_open.sh [tag]     (output under build/ by default)
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${OUT_ROOT:-$R/build}/${1:-openpmc}
mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
timeout -k 10 240 rocprofv3 --pmc FETCH_SIZE -d $OUT/pass_a -o p --output-format csv -- python3 $R/tools/bench_open.py --reps 2 --mul-gps 1,1 --cases eval_gate_queries,combine_8 --out $OUT/discard_a.jsonl > $OUT/pass_a.log 2>&1 || { echo open pmc pass failed; tail -5 $OUT/pass_a.log; exit 3; }
cd $R
python3 tools/pmc_open.py $OUT > $OUT/open_pmc.jsonl
cut -c1-600 $OUT/open_pmc.jsonl
