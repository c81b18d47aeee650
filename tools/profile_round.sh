#!/bin/bash
# Everything a round's profiles/ refresh needs, in one GPU-box call (bash tools/profile_round.sh r05 <commit>):
# bench kernel stats + HBM / SQ counters (profile_bench.sh), the three training steps' kernel stats and HBM traffic, the stand-alone
# element-wise kernels, the shape cliffs, and one un-profiled `bench.py --full` line.  This script's logs and results land in $OUT
# (default profile_out/); copy what is judged to profiles/.
TAG=${1:-r05}; COMMIT=${2:-unknown}
R=${GRAFT_REPO_ROOT:-$PWD}
cd $R
OUT=${OUT:-$R/profile_out}; mkdir -p $OUT
bash tools/profile_bench.sh $TAG $COMMIT > $OUT/profile_bench_$TAG.log 2>&1
bash tools/profile_training.sh $TAG > $OUT/profile_training_$TAG.log 2>&1
bash tools/profile_training_cfg3.sh $TAG > $OUT/profile_training_cfg3_$TAG.log 2>&1
bash tools/profile_training_cfg4.sh $TAG > $OUT/profile_training_cfg4_$TAG.log 2>&1
bash tools/pmc_training.sh > $OUT/pmc_training_$TAG.log 2>&1
bash tools/pmc_training_cfg3.sh > $OUT/pmc_training_cfg3_$TAG.log 2>&1
bash tools/pmc_training_cfg4.sh > $OUT/pmc_training_cfg4_$TAG.log 2>&1
cd $R
python3 tools/bench_elementwise.py > $OUT/${TAG}_elementwise.jsonl 2> $OUT/${TAG}_elementwise.err
python3 tools/bench_cliffs.py > $OUT/${TAG}_cliffs.jsonl 2> $OUT/${TAG}_cliffs.err
python3 bench.py --full --steps 200 > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
python3 -c "import sys; sys.path.insert(0, '.'); from stribor_amd import _hip; print(_hip.build_id())" > $OUT/${TAG}_build_id.txt
ls $OUT | head -50
