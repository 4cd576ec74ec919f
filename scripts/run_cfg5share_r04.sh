OUT=${1:?usage: run_cfg5share_r04.sh OUTDIR}; mkdir -p $OUT
for P in 14 16 20; do
  timeout 1500 python bench.py --full --config cfg5share --log2m $P --steps 3 --warmup 1 --no-cpu-baseline > $OUT/bench_cfg5share_p$P.json 2> $OUT/bench_cfg5share_p$P.err
  tail -c 600 $OUT/bench_cfg5share_p$P.json
  bash scripts/profile_r04.sh r04_cfg5 cfg5share_p$P 13 3e9 4 64 $P 24
done
