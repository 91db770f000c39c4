set -x
cd $GRAFT_REPO_ROOT
export TMPDIR=/tmp
O=${1:?usage: bash tests/tools/run_profile.sh OUTDIR}
mkdir -p $O
[ -n "$SKIP_TESTS" ] || timeout 900 python -m pytest tests -x -q -m gpu 2>&1 | tail -3
timeout 300 python bench.py --full > $O/bench.json 2> $O/bench.err; tail -1 $O/bench.json
timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/stats -o st -- python3 bench.py --full --no_cpu_baseline > $O/bench_rocprof.json 2>$O/rocprof.err
find $O/stats -name "*kernel_stats.csv" | head
timeout 300 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $O/pmc_fetch -o f -- python3 bench.py --full --no_cpu_baseline --steps 3 --warmup 1 > /dev/null 2>$O/pmc1.err
timeout 300 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $O/pmc_write -o w -- python3 bench.py --full --no_cpu_baseline --steps 3 --warmup 1 > /dev/null 2>$O/pmc2.err
timeout 300 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_WAVE_CYCLES --kernel-trace --output-format csv -d $O/pmc_mfma -o m -- python3 bench.py --full --no_cpu_baseline --steps 3 --warmup 1 > /dev/null 2>$O/pmc3.err
for d in fetch write mfma; do python tests/tools/pmc_summary.py $O/pmc_$d $O/pmc_$d.csv; head -8 $O/pmc_$d.csv; done
# keep the merge-back small
find $O -name "*counter_collection.csv" -delete; find $O -name "*kernel_trace.csv" -delete; find $O -name "*.db" -delete
du -sh $O
