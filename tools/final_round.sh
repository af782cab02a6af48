#!/bin/bash
# usage (GPU box): bash tools/final_round.sh [tag] [out_dir]  -- the round's closing evidence on the current tree -> <out_dir>/<tag>_*
# (out_dir defaults to evidence/; copy into profiles/)
tag=${1:-r06_final7}
out=${2:-evidence}
mkdir -p $out
python -m pytest tests -m gpu -x -q --durations=8 > $out/${tag}_pytest_gpu.txt 2>&1; echo "pytest exit $?" >> $out/${tag}_pytest_gpu.txt
python bench.py --full --steps 20 --warmup 5 > $out/${tag}_bench.json 2> $out/${tag}_bench.err
if [ -z "$FINAL_SHORT" ]; then
  bash tools/profile_round.sh ${tag/final/v} > /dev/null 2>&1
  bash tools/small_trace.sh dsec640x480 10000 > $out/r06_lowlat_trace_dsec.txt 2>&1
  bash tools/small_trace.sh upenn346x260 1000 > $out/r06_lowlat_trace_upenn.txt 2>&1
  bash tools/ab_env_small.sh 3 "ESVO_LOWLAT=0" "ESVO_LOWLAT=1" > $out/r06_lowlat_ab.txt 2>&1
  bash tools/ab_band_share.sh > $out/r06_lowlat_band.txt 2>&1
  python tools/closed_loop_ms.py > $out/r06_lowlat_closed_loop.txt 2>&1
  python bench.py --full --steps 20 --warmup 5 --extras --no-cpu-baseline > $out/${tag}_extras_bench.json 2> $out/${tag}_extras_bench.err
fi
tail -3 $out/${tag}_pytest_gpu.txt
