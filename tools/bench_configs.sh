#!/bin/bash
# One bench line per BASELINE.json config that fits one GPU, into profiles/r<N>_configs/ (run on the GPU box), then the
# reference's own published shapes (hidden 500 and 400, LSTM_HIP_PAD_HIDDEN = --flags 256).
#   bash tools/bench_configs.sh r4              (everything)
#   bash tools/bench_configs.sh r4 refshapes    (the reference's shapes only)
R=${1:-r3}
OUT=gpurun_out/${R}_configs
mkdir -p $OUT
if [ "${2:-}" != refshapes ]; then
python bench.py --full --config 0 --steps 400 --warmup 40 > $OUT/cfg0_alice29_h128_s25_b1.json 2> $OUT/cfg0.err; echo "cfg0 rc=$?"
python bench.py --full --config 1 --steps 200 --warmup 20 > $OUT/cfg1_enwik5_h256_s50_b32.json 2> $OUT/cfg1.err; echo "cfg1 rc=$?"
python bench.py --full --config 2 --steps 200 --warmup 20 > $OUT/cfg2_enwik6_h512_s100_b64.json 2> $OUT/cfg2.err; echo "cfg2 rc=$?"
python bench.py --config 2 --steps 20 --warmup 5 > $OUT/cfg2_driver_flags.json 2> $OUT/cfg2d.err; echo "cfg2 (driver flags) rc=$?"
python bench.py --full --config 2 --batch 128 --steps 50 --warmup 5 --no-cpu-baseline > $OUT/cfg2_enwik6_h512_s100_b128_two_launches.json 2> $OUT/cfg2w.err; echo "cfg2 b128 rc=$?"
python bench.py --full --config 4 --steps 100 --warmup 10 > $OUT/cfg4_enwik7_h1024_s100_b16_bf16.json 2> $OUT/cfg4.err; echo "cfg4 rc=$?"
python bench.py --full --config 4 --fp32 --steps 100 --warmup 10 --no-cpu-baseline > $OUT/cfg4_enwik7_h1024_s100_b16_fp32.json 2> $OUT/cfg4f.err; echo "cfg4 fp32 rc=$?"
python bench.py --full --config 4 --batch 64 --steps 50 --warmup 5 --no-cpu-baseline > $OUT/cfg4_enwik7_h1024_s100_b64_bf16.json 2> $OUT/cfg4c.err; echo "cfg4 b64 rc=$?"
python bench.py --full --config 4 --batch 128 --steps 20 --warmup 3 --cpu-budget 10 > $OUT/cfg4_enwik7_h1024_s100_b128_bf16.json 2> $OUT/cfg4b.err; echo "cfg4 b128 rc=$?"
fi
# the reference's shapes (OV/lstm_eigen_class_CUDA/models/): padded, at their padded width Np without the flag, and hidden 400
# unpadded (a multiple of 16 but not of 64: the per-step engine); 448 is the other candidate width for 400.
# Each line has a time limit, and the first failure ends the script.
ref() {
    local name=$1; shift
    timeout -k 10 600 python bench.py "$@" > $OUT/ref_$name.json 2> $OUT/ref_$name.err
    local rc=$?; echo "$name rc=$rc"
    [ $rc -eq 0 ] || exit $rc
}
ref h500_s7_b1024_pad         --hidden 500 --seq 7 --batch 1024 --flags 256 --steps 50 --warmup 5
ref h512_s7_b1024_native      --hidden 512 --seq 7 --batch 1024 --steps 50 --warmup 5
ref h400_s100_b1024_pad       --hidden 400 --seq 100 --batch 1024 --flags 256 --steps 20 --warmup 3
ref h512_s100_b1024_native    --hidden 512 --seq 100 --batch 1024 --steps 20 --warmup 3
ref h448_s100_b1024_native    --hidden 448 --seq 100 --batch 1024 --steps 20 --warmup 3
ref h400_s100_b1024_unpadded  --hidden 400 --seq 100 --batch 1024 --steps 20 --warmup 3
ref h400_s100_b64_pad         --hidden 400 --seq 100 --batch 64 --flags 256 --steps 100 --warmup 10
ref h448_s100_b64_native      --hidden 448 --seq 100 --batch 64 --steps 100 --warmup 10
ref h400_s100_b64_unpadded    --hidden 400 --seq 100 --batch 64 --steps 100 --warmup 10
for f in $OUT/*.json; do echo "== $f"; cut -c1-400 $f; done
