# bash tools/run_profiles.sh on a machine with an MI355X (bench lines of every mode, kernel trace, PMC traffic / SQ counters of the mx mode, all under
# $EV_OUT, default <repo>/out; then, with the same EV_OUT: python tools/profile_summary.py --tag r4_x)
cd "$(dirname "$0")/.."; export EV_OUT="$(mkdir -p "${EV_OUT:-out}" && cd "${EV_OUT:-out}" && pwd)"; OUT="$EV_OUT"
bash tools/gpu_check.sh bench prof pmc pmccal pmcsq 2>&1 | tail -n 8
timeout 600 python bench.py --full --mode ragged --steps 3 --warmup 1 --cpu-utts 0 --no-other-precision > "$OUT/bench_ragged.log" 2>&1; tail -n 1 "$OUT/bench_ragged.log" | cut -c1-300
timeout 600 python bench.py --full --mode vocoder --steps 3 --warmup 1 --cpu-utts 0 --no-other-precision > "$OUT/bench_vocoder.log" 2>&1; tail -n 1 "$OUT/bench_vocoder.log" | cut -c1-300
