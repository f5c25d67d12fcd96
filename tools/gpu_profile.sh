# One GPU call: the full bench line, the rocprofv3 kernel-trace summary of a plain bench run, and the
# PMC passes (FETCH_SIZE, WRITE_SIZE, SQ) over the same launches (tools/pmc_workload.py).
# Every GPU step has its own time limit; steps are chained with && (stop at the first failure).
# Results go to $OUT (default profile_out/, not tracked).
set -o pipefail
OUT=${OUT:-profile_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 600 python3 -u bench.py --steps 20 --warmup 5 --full > "$OUT/bench.json" 2> "$OUT/bench.err" &&
echo "bench ok" &&
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o run -- python3 -u bench.py --steps 20 --warmup 5 > "$OUT/bench_prof.json" 2> "$OUT/bench_prof.err" &&
echo "kernel trace ok" &&
timeout -s KILL 150 rocprofv3 --pmc FETCH_SIZE --output-format csv -d "$OUT/pmc_fetch" -o run -- python3 tools/pmc_workload.py --order "$OUT/pmc_order.json" > "$OUT/pmc_fetch.log" 2>&1 &&
timeout -s KILL 150 rocprofv3 --pmc WRITE_SIZE --output-format csv -d "$OUT/pmc_write" -o run -- python3 tools/pmc_workload.py --order "$OUT/pmc_order.json" > "$OUT/pmc_write.log" 2>&1 &&
timeout -s KILL 150 rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE --output-format csv -d "$OUT/pmc_sq" -o run -- python3 tools/pmc_workload.py --order "$OUT/pmc_order.json" > "$OUT/pmc_sq.log" 2>&1 &&
echo "pmc ok"
