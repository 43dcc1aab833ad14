#!/bin/bash
# tools/headline_ab.sh PARENT_DIR [ROUNDS]: the headline leg of bench.py at this tree and at a BUILT tree of the parent commit
# (PARENT_DIR: bench.py + samplenet_amd/ with its library), alternated on ONE box in one call -> the record of profiles/*/headline_ab.txt.
# Every run sits under its own time limit; the script stops at the first run that does not end cleanly.
cd "$(dirname "$0")/.."
HERE=$(pwd); PARENT=$(cd "$1" && pwd); ROUNDS=${2:-3}
echo "# python bench.py --gpus 1 --no-cpu-baseline --no-extra-legs --no-module-surface (the headline leg alone: synthetic input, the sampler's"
echo "# step as one graph) at this commit and at its parent, on ONE MI355X box in one call, alternated this / parent, $ROUNDS runs each."
for i in $(seq 1 $ROUNDS); do
  for v in this parent; do
    if [ $v == this ]; then d=$HERE; else d=$PARENT; fi
    line=$(cd $d && timeout -k 10 300 python bench.py --gpus 1 --no-cpu-baseline --no-extra-legs --no-module-surface 2>/dev/null | tail -1)
    rc=$?
    if [ $rc -ne 0 ]; then echo "$v round $i: bench.py ended with $rc"; exit $rc; fi
    echo "$line" | python -c "import json,sys; d=json.load(sys.stdin); print('%-6s round $i  %8.0f clouds/s   %.4f ms/step' % ('$v', d['value'], d['ms_per_step']))" || exit 1
  done
done
