#!/bin/bash
# Run on a machine with an MI355X:  bash tools/gpu_check.sh [stage...]    (logs and profiles go to $EV_OUT, default <repo>/out)
# Stages: ops parity gen smoke bench ubench prof pmc pmccal pmcsq dist2    (default: ops parity smoke bench)
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
OUT="${EV_OUT:-$ROOT/out}"
cd "$ROOT"
mkdir -p "$OUT" && OUT="$(cd "$OUT" && pwd)"
STAGES="${@:-ops parity smoke bench}"
rocminfo 2>/dev/null | grep -E "Marketing Name|gfx" | head -4 > "$OUT/device.log"
nproc >> "$OUT/device.log"
python -c "import bench; print(bench.csrc_hash())" > "$OUT/csrc_hash.txt"      # what every measurement of this call ran on (profile_summary.py stamps it)
for st in $STAGES; do
  case $st in
    ops)    timeout 900 python -m pytest tests/test_gpu_ops.py -m gpu -q --timeout 600 > "$OUT/ops.log" 2>&1; echo "ops rc=$?";;
    parity) timeout 1800 python -m pytest tests/test_gpu_parity.py -m gpu -q --timeout 900 > "$OUT/parity.log" 2>&1; echo "parity rc=$?";;
    smoke)  timeout 600 python __graft_entry__.py smoke > "$OUT/smoke.log" 2>&1; echo "smoke rc=$?";;
    bench)  timeout 900 python bench.py --full --steps 10 --warmup 3 --cpu-utts 4 --dump-launches "$OUT/launches.json" > "$OUT/bench.log" 2>&1; echo "bench rc=$?";;
    gen)    timeout 900 python -m pytest tests/test_gpu_generator.py tests/test_gpu_api.py tests/test_gpu_simbert.py tests/test_gpu_dist.py -m gpu -q --timeout 600 > "$OUT/gen.log" 2>&1; echo "gen rc=$?";;
    pmc)    cd /tmp && export TMPDIR=/tmp
            timeout 600 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d "$OUT/pmc_fetch" -o f -- python "$ROOT/bench.py" --full --steps 1 --warmup 1 --cpu-utts 0 --no-other-precision > "$OUT/pmc_fetch.log" 2>&1
            timeout 600 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d "$OUT/pmc_write" -o w -- python "$ROOT/bench.py" --full --steps 1 --warmup 1 --cpu-utts 0 --no-other-precision > "$OUT/pmc_write.log" 2>&1
            echo "pmc rc=$?"; cd "$ROOT";;
    pmcsq)  # MFMA-busy / wait / LDS-conflict counters (separate passes, --kernel-trace only; never combined with sys/hip/hsa traces)
            cd /tmp && export TMPDIR=/tmp
            rocprofv3 -L 2>/dev/null | grep -E "SQ_VALU_MFMA_BUSY_CYCLES|SQ_BUSY_CU_CYCLES|SQ_LDS_BANK_CONFLICT|SQ_LDS_IDX_ACTIVE|SQ_LDS_UNALIGNED_STALL|GRBM_GUI_ACTIVE|SQ_INSTS_VALU_MFMA|SQ_WAIT_INST_ANY|SQ_ACTIVE_INST_ANY" | head -40 > "$OUT/pmc_available.txt"
            BENCH="python $ROOT/bench.py --full --steps 1 --warmup 1 --cpu-utts 0 --no-other-precision"
            timeout 400 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CU_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY GRBM_GUI_ACTIVE --kernel-trace --output-format csv -d "$OUT/pmc_sq" -o s -- $BENCH > "$OUT/pmc_sq.log" 2>&1; echo "pmc_sq rc=$?"
            timeout 400 rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_LDS_UNALIGNED_STALL GRBM_GUI_ACTIVE --kernel-trace --output-format csv -d "$OUT/pmc_lds" -o l -- $BENCH > "$OUT/pmc_lds.log" 2>&1; echo "pmc_lds rc=$?"
            cd "$ROOT";;
    pmccal) # calibration of FETCH_SIZE / WRITE_SIZE on a copy of known size (MI355X_MICROARCH.md section HBM)
            cd /tmp && export TMPDIR=/tmp
            timeout 300 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d "$OUT/pmc_cal_fetch" -o c -- python "$ROOT/tools/pmc_calibrate.py" > "$OUT/pmc_cal_fetch.log" 2>&1
            timeout 300 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d "$OUT/pmc_cal_write" -o c -- python "$ROOT/tools/pmc_calibrate.py" > "$OUT/pmc_cal_write.log" 2>&1
            echo "pmccal rc=$?"; cd "$ROOT";;
    dist2)  timeout 900 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29533 bench.py --gpus 2 --steps 3 --warmup 1 --backend gloo --force-device 0 --batch 8 > "$OUT/dist2.log" 2>&1; echo "dist2 rc=$?"; tail -n 3 "$OUT/dist2.log" | cut -c1-600;;
    ubench) # stand-alone micro-benchmarks / hardware checks built in-tree (hipcc -o tools/build/<name> tools/<name>.hip): layout A/B of the plane sets,
            # the K32 -> K16 MFMA chain check; each prints its own verdict line
            for exe in tools/build/*; do [ -x "$exe" ] && timeout 300 "$exe" > "$OUT/ubench_$(basename $exe).txt" 2>&1; echo "ubench $(basename $exe) rc=$?"; tail -n 12 "$OUT/ubench_$(basename $exe).txt" | cut -c1-400; done;;
    prof)   cd /tmp && export TMPDIR=/tmp && timeout 900 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof" -o r1 -- python "$ROOT/bench.py" --full --steps 3 --warmup 1 --cpu-utts 0 --no-other-precision --voc-streams 1 > "$OUT/prof.log" 2>&1; echo "prof rc=$?"; cd "$ROOT";;
  esac
done
tail -n 30 "$OUT/ops.log" "$OUT/parity.log" "$OUT/gen.log" "$OUT/smoke.log" "$OUT/bench.log" 2>/dev/null | tail -n 120
