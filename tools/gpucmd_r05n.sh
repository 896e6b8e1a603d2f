#!/bin/bash
# Round 5, call N: partial.hip built without the IR load/store vectorizer (fewer SGPR
# spill reloads) against the same sources with it (varlibs/libmapfx_lsv.so):
# MARL_PARTIAL and runner bench lines interleaved, then the partial / runner GPU tests.
set -o pipefail
O=gpurun_out/r05n
mkdir -p $O
for rep in 1 2 3; do
  for v in new lsv; do
    if [ $v = new ]; then L=""; else L=$PWD/varlibs/libmapfx_lsv.so; fi
    MAPFX_LIB=$L timeout -k 10 200 python3 bench.py --full --env marl_partial --cpu-seconds 0 > $O/p_${v}_$rep.json 2> $O/p_${v}_$rep.err || { tail $O/p_${v}_$rep.err; exit 1; }
    MAPFX_LIB=$L timeout -k 10 200 python3 bench.py --full --env runner --cpu-seconds 0 > $O/r_${v}_$rep.json 2> $O/r_${v}_$rep.err || { tail $O/r_${v}_$rep.err; exit 1; }
    python3 -c "import json; p=json.load(open('$O/p_${v}_$rep.json')); r=json.load(open('$O/r_${v}_$rep.json')); print('$v $rep partial', p['ms_per_step'], p['roofline']['frac'], 'runner', r['ms_per_step'])"
  done
done
timeout -k 10 600 python3 -u -m pytest tests/test_gpu_partial.py tests/test_gpu_partial_full_range.py tests/test_gpu_runner.py -x -q --timeout 300 --timeout-method thread > $O/tests.txt 2>&1 || { tail -30 $O/tests.txt; exit 1; }
tail -2 $O/tests.txt
