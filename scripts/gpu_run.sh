#!/bin/bash
# One parametrised GPU lease script (replaces the per-experiment scripts of earlier rounds):
#   gpurun --timeout N -- 'bash scripts/gpu_run.sh <tag> <stage> [<stage> ...]'
# Stages write under gpurun_out/<tag>/.  Everything DESIGN.md / profiles/ quote comes from `final`.
set -x
TAG=$1; shift
export TMPDIR=/tmp
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=$R/gpurun_out/$TAG
mkdir -p $O
for stage in "$@"; do
  case $stage in
    smoke)      timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1; echo "smoke rc=$?" >> $O/smoke.log ;;
    test_corr)  timeout 900 python -m pytest tests/test_corr_gpu.py -m gpu -q -rA 2>&1 | tail -80 > $O/pytest_corr.log ;;
    test_conv)  timeout 900 python -m pytest tests/test_conv_gpu.py -m gpu -q -rA 2>&1 | tail -80 > $O/pytest_conv.log ;;
    test_dcn)   timeout 900 python -m pytest tests/test_dcn_gpu.py -m gpu -q -rA 2>&1 | tail -80 > $O/pytest_dcn.log ;;
    test_rest)  timeout 1500 python -m pytest tests/test_restoration_gpu.py -m gpu -q -rA 2>&1 | tail -80 > $O/pytest_restoration.log ;;
    test_all)   timeout 2400 python -m pytest tests -m gpu -q -rA 2>&1 | tail -220 > $O/pytest_gpu.log ;;
    diag_corr)  timeout 600 python scripts/diag_corr_filter.py --lr320 > $O/diag_corr_filter.log 2>&1 ;;
    bench)      timeout 900 python bench.py --steps 20 --warmup 5 --full > $O/bench_default.log 2>&1; echo "rc=$?" >> $O/bench_default.log ;;
    bench_dist1) C2M_BENCH_FORCE_DIST=1 timeout 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29517 bench.py --gpus 1 --steps 5 --warmup 2 --no-cpu-baseline --no-alt > $O/bench_dist1.log 2>&1; echo "rc=$?" >> $O/bench_dist1.log ;;
    bench_quick) timeout 600 python bench.py --steps 8 --warmup 3 --no-cpu-baseline --no-alt > $O/bench_quick.log 2>&1; echo "rc=$?" >> $O/bench_quick.log ;;
    bench_corr) timeout 300 python bench.py --workload corr --steps 10 --warmup 3 --full > $O/bench_corr.log 2>&1 ;;
    bench_train) timeout 300 python bench.py --workload train --steps 20 --warmup 5 > $O/bench_train.log 2>&1
                C2M_TRAIN_KERNELS=0 timeout 300 python bench.py --workload train --steps 20 --warmup 5 > $O/bench_train_stock.log 2>&1
                timeout 300 python bench.py --workload train --batch 4 --steps 20 --warmup 5 > $O/bench_train_b4.log 2>&1
                C2M_TRAIN_KERNELS=0 timeout 300 python bench.py --workload train --batch 4 --steps 20 --warmup 5 > $O/bench_train_b4_stock.log 2>&1
                C2M_TRAIN_KERNELS=1 timeout 300 python bench.py --workload train --steps 20 --warmup 5 > $O/bench_train_kernels.log 2>&1
                C2M_BENCH_FORCE_DIST=1 timeout 300 python bench.py --workload train --steps 10 --warmup 3 > $O/bench_train_rccl_1rank.log 2>&1 ;;
    bench_cfg5) timeout 300 python bench.py --lr 320 --dtype bf16 --steps 5 --warmup 2 > $O/bench_cfg5_bf16.log 2>&1
                timeout 300 python bench.py --lr 320 --steps 5 --warmup 2 --full --no-cpu-baseline > $O/bench_cfg5_f32.log 2>&1 ;;
    bench_cfg5_bf16) timeout 300 python bench.py --lr 320 --dtype bf16 --steps 5 --warmup 2 --no-cpu-baseline > $O/bench_cfg5_bf16.log 2>&1
                C2M_BF16_IO=0 timeout 300 python bench.py --lr 320 --dtype bf16 --steps 5 --warmup 2 --no-cpu-baseline > $O/bench_cfg5_bf16_f32io.log 2>&1 ;;
    bench_conv16) (echo "== bf16 kernel, fp32 tensors, B=4"; timeout 200 python scripts/bench_conv.py --batch 4 --algo bf16 --only body
                   echo "== bf16 kernel, bf16 tensors, B=4"; timeout 200 python scripts/bench_conv.py --batch 4 --io16 --only body) > $O/bench_conv16.log 2>&1 ;;
    test_head)  timeout 900 python -m pytest tests/test_conv_gpu.py -m gpu -q -rA -k "head" 2>&1 | tail -60 > $O/pytest_head.log ;;
    bench_head) (timeout 200 python scripts/bench_conv.py --only "dcn head") > $O/bench_head.log 2>&1 ;;
    test_dcn16) timeout 900 python -m pytest tests/test_dcn_gpu.py -m gpu -q -x -k "f16x2" 2>&1 | tail -60 > $O/pytest_dcn16.log ;;
    bench_dcn16) timeout 600 python bench.py --steps 8 --warmup 3 --no-cpu-baseline --no-alt > $O/bench_dcn16_on.log 2>&1
                C2M_DCN_F16X2=0 timeout 600 python bench.py --steps 8 --warmup 3 --no-cpu-baseline --no-alt > $O/bench_dcn16_off.log 2>&1 ;;
    tpw_sweep)  for t in 0 1 2 3 4 5 6 7 9 13; do
                  echo "=== C2M_CONV_TPW=$t (0 = heuristic)" >> $O/tpw_sweep.txt
                  C2M_CONV_TPW=$t timeout 200 python scripts/bench_conv.py --only "${TPW_ONLY:-64->64 @320}" --iters 20 2>&1 | grep "^{'layer" >> $O/tpw_sweep.txt
                done ;;
    test_bf16)  timeout 900 python -m pytest tests/test_conv_gpu.py tests/test_restoration_gpu.py -m gpu -q -rA -k "bf16" 2>&1 | tail -80 > $O/pytest_bf16.log ;;
    bench_conv) timeout 300 python scripts/bench_conv.py > $O/bench_conv.log 2>&1 ;;
    bench_dcn)  timeout 600 python scripts/bench_dcn.py > $O/bench_dcn.log 2>&1 ;;
    prof)       cd /tmp
                timeout 600 rocprofv3 --kernel-trace --stats -f csv -d $O/prof_step -o step -- python $R/bench.py --steps 3 --warmup 2 --no-cpu-baseline --no-alt > $O/rocprof_step.log 2>&1
                cd $R ;;
    power)      (rocm-smi -M 2>&1 | grep -i "power\|GPU"; rocm-smi -P -c -t --json 2>&1 | cut -c1-900
                 BC="python $R/scripts/bench_conv.py --algo split16 --iters 6000"
                 bash scripts/power_probe.sh "$BC --only 'body 64->64 @640'" "f16 x 2 body 64->64 @640, N(0,1) data"
                 bash scripts/power_probe.sh "$BC --only 'body+res 64->64 @640'" "f16 x 2 body+res 64->64 @640, N(0,1) data"
                 bash scripts/power_probe.sh "$BC --only 'body 64->64 @640' --data zeros" "f16 x 2 body 64->64 @640, all-zero data") > $O/power_probe.log 2>&1 ;;
    power2)     (bash scripts/power_probe.sh "python $R/scripts/bench_conv.py --algo bf16 --io16 --iters 6000 --only 'body 64->64 @640'" "bf16 tensors, one product: body 64->64 @640"
                 bash scripts/power_probe.sh "python $R/bench.py --workload corr --steps 400 --warmup 3 --no-cpu-baseline" "correlation stage alone (bench.py --workload corr)" 12 8
                 bash scripts/power_probe.sh "python $R/scripts/bench_dcn_nhwc.py --iters 400" "DCNv2 forwards (three layers, fp32 and f16 x 2 in turn)" 16 6
                 bash scripts/power_probe.sh "python $R/bench.py --steps 120 --warmup 3 --no-cpu-baseline --no-alt" "the whole configs[2] step, back to back" 40 10) > $O/power_probe2.log 2>&1 ;;
    ab_lib)     (for lib in "" $R/build_exp/${AB_LIB:-fastall}/libc2m_hip.so "" $R/build_exp/${AB_LIB:-fastall}/libc2m_hip.so; do echo "=== C2M_LIB=$lib"; C2M_LIB=$lib timeout 300 python scripts/bench_conv.py --algo split16 --iters 20 2>&1 | grep "^{'layer"; done) > $O/ab_lib_layers.log 2>&1
                (for lib in "" $R/build_exp/${AB_LIB:-fastall}/libc2m_hip.so "" $R/build_exp/${AB_LIB:-fastall}/libc2m_hip.so; do echo "=== C2M_LIB=$lib"; C2M_LIB=$lib timeout 600 python bench.py --steps 10 --warmup 3 --no-cpu-baseline --no-alt 2>&1 | grep "^{" | cut -c1-700; done) > $O/ab_lib_step.log 2>&1 ;;
    prof_cfg5)  cd /tmp
                timeout 600 rocprofv3 --kernel-trace --stats -f csv -d $O/prof_cfg5 -o step -- python $R/bench.py --lr 320 --dtype bf16 --steps 3 --warmup 2 --no-cpu-baseline --no-alt > $O/rocprof_cfg5.log 2>&1
                cp $(find $O/prof_cfg5 -name '*kernel_stats.csv' | head -1) $O/cfg5_kernel_stats.csv; rm -rf $O/prof_cfg5
                cd $R ;;
    pmc)        cd /tmp
                timeout 600 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_INSTS_VALU SQ_INSTS_SALU GRBM_GUI_ACTIVE --kernel-trace -f csv -d $O/pmc_mfma -o step -- python $R/bench.py --steps 2 --warmup 2 --no-cpu-baseline --no-alt > $O/pmc_mfma.log 2>&1
                timeout 600 rocprofv3 --pmc FETCH_SIZE --kernel-trace -f csv -d $O/pmc_fetch -o step -- python $R/bench.py --steps 2 --warmup 2 --no-cpu-baseline --no-alt > $O/pmc_fetch.log 2>&1
                timeout 600 rocprofv3 --pmc WRITE_SIZE --kernel-trace -f csv -d $O/pmc_write -o step -- python $R/bench.py --steps 2 --warmup 2 --no-cpu-baseline --no-alt > $O/pmc_write.log 2>&1
                cd $R ;;
    pmc_corr)   cd /tmp
                timeout 300 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_WAVE_CYCLES SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_INSTS_VALU SQ_INSTS_LDS SQ_ACTIVE_INST_LDS --kernel-trace -f csv -d $O/pmc_corr1 -o c -- python $R/bench.py --workload corr --steps 2 --warmup 1 --no-cpu-baseline > $O/pmc_corr1.log 2>&1
                timeout 300 rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_VMEM SQ_WAIT_INST_LDS SQ_LDS_DATA_FIFO_FULL SQ_LDS_CMD_FIFO_FULL SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU --kernel-trace -f csv -d $O/pmc_corr2 -o c -- python $R/bench.py --workload corr --steps 2 --warmup 1 --no-cpu-baseline > $O/pmc_corr2.log 2>&1
                timeout 300 rocprofv3 --pmc FETCH_SIZE WRITE_SIZE --kernel-trace -f csv -d $O/pmc_corr3 -o c -- python $R/bench.py --workload corr --steps 2 --warmup 1 --no-cpu-baseline > $O/pmc_corr3.log 2>&1
                cd $R
                (python scripts/pmc_kernel.py $O/pmc_corr1 corr; python scripts/pmc_kernel.py $O/pmc_corr2 corr; python scripts/pmc_kernel.py $O/pmc_corr3 corr) > $O/pmc_corr_summary.txt 2>&1
                rm -rf $O/pmc_corr1 $O/pmc_corr2 $O/pmc_corr3 ;;
    pmc_cfg5)   cd /tmp
                timeout 400 rocprofv3 --pmc FETCH_SIZE --kernel-trace -f csv -d $O/pmc5_fetch -o s -- python $R/bench.py --lr 320 --dtype bf16 --steps 2 --warmup 1 --no-cpu-baseline > $O/pmc5_fetch.log 2>&1
                timeout 400 rocprofv3 --pmc WRITE_SIZE --kernel-trace -f csv -d $O/pmc5_write -o s -- python $R/bench.py --lr 320 --dtype bf16 --steps 2 --warmup 1 --no-cpu-baseline > $O/pmc5_write.log 2>&1
                cd $R
                (python scripts/pmc_kernel.py $O/pmc5_fetch c2m; python scripts/pmc_kernel.py $O/pmc5_write c2m) > $O/pmc_cfg5_summary.txt 2>&1
                rm -rf $O/pmc5_fetch $O/pmc5_write ;;
    prof_train) cd /tmp
                timeout 600 rocprofv3 --kernel-trace --stats -f csv -d $O/prof_train -o t -- python $R/bench.py --workload train --batch 4 --steps 10 --warmup 3 > $O/rocprof_train.log 2>&1
                cd $R
                python - "$O" <<'PY'
import csv, sys, glob
O = sys.argv[1]
f = glob.glob(O + "/prof_train/**/t_kernel_stats.csv", recursive=True)
rows = list(csv.DictReader(open(f[0]))) if f else []
tot = sum(float(r["TotalDurationNs"]) for r in rows)
with open(O + "/train_b4_kernel_stats.txt", "w") as out:
    out.write("total kernel ms over 13 steps: %.1f, kernels: %d kinds, launches %d\n" % (tot / 1e6, len(rows), sum(int(r["Calls"]) for r in rows)))
    for r in rows[:45]:
        out.write("%-100s calls %6s total_ms %9.3f avg_us %9.2f pct %s\n" % (r["Name"][:100], r["Calls"], float(r["TotalDurationNs"]) / 1e6, float(r["AverageNs"]) / 1e3, r["Percentage"]))
PY
                rm -rf $O/prof_train ;;
    pmc_train)  cd /tmp
                for c in FETCH_SIZE WRITE_SIZE; do   # (one counter per pass: both together exceed what the hardware collects)
                  timeout 400 rocprofv3 --pmc $c --kernel-trace -f csv -d $O/pmct_$c -o s -- python $R/bench.py --workload train --global-batch 4 --steps 3 --warmup 2 > $O/pmct_$c.log 2>&1
                done
                cd $R
                (python scripts/pmc_kernel.py $O/pmct_FETCH_SIZE ""; python scripts/pmc_kernel.py $O/pmct_WRITE_SIZE "") > $O/pmc_train_summary.txt 2>&1
                rm -rf $O/pmct_FETCH_SIZE $O/pmct_WRITE_SIZE ;;
    avail)      cd /tmp; (rocprofv3 --list-avail 2>&1 | grep -o "\b\(TCP\|TA\|TD\|TCC\|SQ\|SQC\|GRBM\|CPC\|SPI\)_[A-Za-z0-9_]*" | sort -u | tr "\n" " ") > $O/pmc_avail.txt 2>&1; cd $R ;;
    pmc_dcn)    cd /tmp
                i=0
                for set in "SQ_INSTS_VALU SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_WAVE_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_INSTS_VMEM SQ_ACTIVE_INST_VALU" \
                           "SQ_INST_CYCLES_VMEM SQ_ACTIVE_INST_VMEM SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_VALU_MFMA_BUSY_CYCLES SQ_ACTIVE_INST_ANY SQ_INSTS_LDS SQ_ACTIVE_INST_LDS" \
                           "${PMC_SET3:-TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_sum TCP_PENDING_STALL_CYCLES_sum TA_TA_BUSY_sum}" \
                           "${PMC_SET4:-TCP_TOTAL_ACCESSES_sum TCP_TA_TCP_STATE_READ_sum TCP_TCP_TA_DATA_STALL_CYCLES_sum TA_BUSY_avr}" \
                           "${PMC_SET5:-TA_ADDR_STALLED_BY_TC_CYCLES_sum TA_DATA_STALLED_BY_TC_CYCLES_sum TA_BUFFER_WAVEFRONTS_sum TD_TD_BUSY_sum}" \
                           "${PMC_SET6:-TCP_TCC_WRITE_REQ_sum TCC_EA0_WRREQ_sum TCC_EA0_WRREQ_STALL_sum TCC_HIT_sum TCC_MISS_sum}"; do
                  i=$((i+1))
                  timeout 300 rocprofv3 --pmc $set --kernel-trace -f csv -d $O/pmcd_$i -o c -- python $R/scripts/bench_dcn_nhwc.py --iters 2 > $O/pmcd_$i.log 2>&1
                  echo "=== dcn forward, pass $i: $set" >> $O/pmc_dcn_c3.txt
                  python $R/scripts/pmc_kernel.py $O/pmcd_$i dcn_fwd >> $O/pmc_dcn_c3.txt 2>&1
                  tail -3 $O/pmcd_$i.log | cut -c1-300 >> $O/pmc_dcn_c3.txt
                  timeout 300 rocprofv3 --pmc $set --kernel-trace -f csv -d $O/pmcc_$i -o c -- python $R/scripts/abl_c3.py 16 640 twin > $O/pmcc_$i.log 2>&1
                  echo "=== first layer (twin), pass $i: $set" >> $O/pmc_dcn_c3.txt
                  python $R/scripts/pmc_kernel.py $O/pmcc_$i conv3x3_c3 >> $O/pmc_dcn_c3.txt 2>&1
                  tail -2 $O/pmcc_$i.log | cut -c1-300 >> $O/pmc_dcn_c3.txt
                  rm -rf $O/pmcd_$i $O/pmcc_$i
                done
                cd $R ;;
    ab_corrf)   (timeout 120 python scripts/abl_corr_filter.py 2>&1 | grep "^{"; timeout 300 python bench.py --workload corr --steps 10 --warmup 3 --no-cpu-baseline 2>&1 | grep "^{" | python -c "import sys,json; p=json.loads(sys.stdin.read()); print({'configs1_pairs_per_s': round(p['value'],1), 'ms_per_step': round(p['ms_per_step'],3), 'kernels_ms': p['c2m_kernel_ms_per_step']})") > $O/corr_filter_time.log 2>&1 ;;
    pmc_conv_ta) cd /tmp
                i=0
                for set in "TA_TA_BUSY_sum TCP_PENDING_STALL_CYCLES_sum TCP_TCP_TA_DATA_STALL_CYCLES_sum TCP_TOTAL_CACHE_ACCESSES_sum GRBM_GUI_ACTIVE" \
                           "TCP_TCC_READ_REQ_sum TCP_TCC_WRITE_REQ_sum TCC_HIT_sum TCC_MISS_sum TCC_EA0_WRREQ_STALL_sum GRBM_GUI_ACTIVE" \
                           "SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_ACTIVE_INST_VMEM SQ_INST_CYCLES_VMEM SQ_WAIT_INST_ANY SQ_WAIT_ANY SQ_WAVE_CYCLES GRBM_GUI_ACTIVE" \
                           "TD_TD_BUSY_sum TCP_TA_TCP_STATE_READ_sum TCP_READ_TAGCONFLICT_STALL_CYCLES_sum TCP_WRITE_TAGCONFLICT_STALL_CYCLES_sum GRBM_GUI_ACTIVE"; do
                  i=$((i+1))
                  timeout 300 rocprofv3 --pmc $set --kernel-trace -f csv -d $O/pmcta_$i -o c -- python $R/scripts/bench_conv.py --algo split16 --only "64->64 @640" --iters 4 > $O/pmcta_$i.log 2>&1
                  echo "=== pass $i: $set" >> $O/pmc_conv_ta.txt
                  grep "^{'layer" $O/pmcta_$i.log >> $O/pmc_conv_ta.txt
                  python $R/scripts/pmc_kernel.py $O/pmcta_$i "conv3x3_split_kernel" >> $O/pmc_conv_ta.txt 2>&1
                  rm -rf $O/pmcta_$i
                done
                cd $R ;;
    *)          echo "unknown stage $stage" ;;
  esac
done
cd $R
find gpurun_out/$TAG -name "*.db" -delete
find gpurun_out/$TAG -name "*kernel_trace.csv" -size +8M -delete
