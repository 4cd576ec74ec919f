set -x
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
OUT=${1:?usage: profile_round.sh OUTDIR}; mkdir -p $OUT
timeout 600 python bench.py --full --steps 10 --warmup 2 > $OUT/bench.json 2> $OUT/bench.err
timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/stats -o st -- python3 bench.py --steps 5 --warmup 1 --no-cpu-baseline --no-accuracy > $OUT/bench_prof.json 2> $OUT/bench_prof.err
cp $(find $OUT/stats -name "*kernel_stats.csv" | head -1) $OUT/kernel_stats.csv
timeout 600 rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/fetch -o f -- python3 scripts/quick_bench.py 10 50e6 > /dev/null 2>&1
timeout 600 rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/write -o w -- python3 scripts/quick_bench.py 10 50e6 > /dev/null 2>&1
python3 scripts/make_traffic.py $OUT/fetch $OUT/write $OUT/traffic.json
timeout 600 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VMEM_RD --kernel-trace --output-format csv -d $OUT/pmc -o pmc -- python3 scripts/quick_bench.py 10 50e6 > /dev/null 2>&1
python3 scripts/pmc_summary.py $(find $OUT/pmc -name "*counter_collection.csv" | head -1) > $OUT/pmc.txt
rm -rf $OUT/stats $OUT/fetch $OUT/write $OUT/pmc
cat $OUT/bench.json
head -12 $OUT/kernel_stats.csv
