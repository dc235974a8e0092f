# Round-2 evidence run on the GPU box: full GPU test suite, smoke, the default bench line, the train_kd line, rocprofv3
# kernel stats of both workloads, PMC passes (HBM traffic; MFMA / LDS utilisation).  Results under gpurun_out/$TAG.
set -x
TAG=${1:-r02f}
R=$GRAFT_REPO_ROOT
cd $R
export TMPDIR=/tmp
O=$R/gpurun_out/$TAG
mkdir -p $O
timeout 1500 python -m pytest tests -m gpu -q > $O/pytest_gpu.log 2>&1; tail -3 $O/pytest_gpu.log
cp gpurun_out/margins.json $O/margins.json 2>/dev/null
python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1; tail -1 $O/smoke.log
python bench.py --full 2>$O/bench.err | tail -1 > $O/bench_default.json
python bench.py --workload train_kd 2>$O/bench_kd.err | tail -1 > $O/bench_train_kd.json
CONVDR_BENCH_FORCE_DIST=1 python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29533 bench.py --gpus 1 --steps 4 --warmup 1 --no-cpu-baseline --no-extras 2>$O/bench_tr.err | tail -1 > $O/bench_torchrun1_forced_dist.json
cd /tmp
rocprofv3 --kernel-trace --stats -d $O/prof -o bench -- python3 $R/bench.py --steps 3 --warmup 1 --no-cpu-baseline --no-extras > $O/prof_bench.log 2>&1
rocprofv3 --kernel-trace --stats -d $O/prof_kd -o kd -- python3 $R/bench.py --workload train_kd --steps 5 --warmup 2 > $O/prof_kd.log 2>&1
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/pmc_fetch -- python3 $R/bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-extras > $O/pmc_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/pmc_write -- python3 $R/bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-extras > $O/pmc_write.log 2>&1
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_INSTS_VALU_MFMA_MOPS_BF16 SQ_BUSY_CYCLES --output-format csv -d $O/pmc_mfma -- python3 $R/bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-extras > $O/pmc_mfma.log 2>&1
rocprofv3 --pmc SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT SQ_ACTIVE_INST_LDS GRBM_GUI_ACTIVE --output-format csv -d $O/pmc_lds -- python3 $R/bench.py --steps 1 --warmup 1 --no-cpu-baseline --no-extras > $O/pmc_lds.log 2>&1
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_INSTS_VALU_MFMA_MOPS_BF16 SQ_BUSY_CYCLES --output-format csv -d $O/pmc_mfma_kd -- python3 $R/bench.py --workload train_kd --steps 2 --warmup 1 > $O/pmc_mfma_kd.log 2>&1
cd $R
python tools/rocpd_summary.py $(find $O/prof -name "*.db" | head -1) > $O/bench_default.kernel_stats.txt
python tools/rocpd_summary.py $(find $O/prof_kd -name "*.db" | head -1) > $O/train_kd.kernel_stats.txt
python tools/train_timeline.py $(find $O/prof_kd -name "*.db" | head -1) > $O/train_kd.timeline.txt
python tools/pmc_summary.py $O/pmc_fetch $O/pmc_write > $O/pmc_hbm_traffic.json
python tools/pmc_summary.py $O/pmc_mfma $O/pmc_lds > $O/pmc_mfma_lds.json
python tools/pmc_summary.py $O/pmc_mfma_kd > $O/pmc_mfma_train_kd.json
find $O -name "*.db" -delete; find $O -name "*counter_collection.csv" -delete; find $O -name "*.csv" -size +1M -delete
du -sh $O
