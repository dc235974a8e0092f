set -x
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
O=$PWD/${1:?usage: refresh_profiles.sh OUTDIR (relative to the repository root)}
mkdir -p $O
timeout 1500 python -m pytest tests -m gpu -x -q > $O/pytest_gpu.log 2>&1; tail -3 $O/pytest_gpu.log
python bench.py --full 2>$O/bench.err | tail -1 > $O/bench_default.json
python bench.py --workload train_kd 2>$O/bench_kd.err | tail -1 > $O/bench_train_kd.json
python -m torch.distributed.run --nnodes=1 --nproc-per-node 1 --master-addr 127.0.0.1 --master-port 29533 bench.py --gpus 1 --steps 4 --warmup 1 --full --no-cpu-baseline 2>$O/bench_tr.err | tail -1 > $O/bench_torchrun1.json
R=$GRAFT_REPO_ROOT
cd /tmp
rocprofv3 --kernel-trace --stats -d $O/prof -o r01f -- python3 $R/bench.py --steps 3 --warmup 1 --no-cpu-baseline > $O/prof_bench.log 2>&1
rocprofv3 --kernel-trace --stats -d $O/prof_kd -o r01f_kd -- python3 $R/bench.py --workload train_kd --steps 5 --warmup 2 --no-cpu-baseline > $O/prof_kd.log 2>&1
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $O/pmc_fetch -- python3 $R/bench.py --steps 1 --warmup 1 --no-cpu-baseline > $O/pmc_fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $O/pmc_write -- python3 $R/bench.py --steps 1 --warmup 1 --no-cpu-baseline > $O/pmc_write.log 2>&1
cd $R
find $O -name "*.db" | head; du -sh $O
python tools/rocpd_summary.py $(find $O/prof -name "*.db" | head -1) > $O/bench_default.kernel_stats.txt
python tools/rocpd_summary.py $(find $O/prof_kd -name "*.db" | head -1) > $O/train_kd.kernel_stats.txt
python tools/pmc_summary.py $O/pmc_fetch $O/pmc_write > $O/pmc_hbm_traffic.json
# keep the merge under the size cap: drop raw traces
find $O -name "*.db" -delete; find $O -name "*counter_collection.csv" -delete
du -sh $O
