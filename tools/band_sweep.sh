#!/bin/bash
# SPIMDECON_BAND sweep on one GPU: the RL tests at band 2, then one bench line per band in
# OUT/b<band>.json.  usage: tools/band_sweep.sh OUT
set -o pipefail
OUT=${1:?usage: tools/band_sweep.sh OUT}
mkdir -p $OUT
export TMPDIR=/tmp
SPIMDECON_BAND=2 timeout -k 10 300 python -u -m pytest tests/test_gpu_rl.py -x -q --timeout 120 --timeout-method thread > $OUT/tests.log 2>&1 || exit 1
for b in 0 1 2 3 4 6 17; do
  SPIMDECON_BAND=$b timeout -k 10 200 python3 bench.py --full --steps 5 --no-cpu-baseline > $OUT/b$b.log 2>&1 || exit 1
  tail -1 $OUT/b$b.log > $OUT/b$b.json
done
