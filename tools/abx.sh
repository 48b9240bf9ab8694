#!/bin/bash
# A/B/C... of library builds and environment switches inside ONE gpurun call (box-to-box variance is larger than most kernel changes).
#   tools/abx.sh "<label>=<lib.so>[,VAR=VAL...] ..." [bench.py arguments]      "cur" as the library = the in-tree build
# Two alternating rounds (ROUNDS=3 for three); prints label, images/s and ms per step of every run.  DUMP=<dir>: every run also writes its
# logits to <dir>/<label>_r<round>/logits.npy (bench.py --dump-outputs) and the md5 sums are printed at the end: equal builds, equal bytes.
# Every run has a time limit of its own and a failed run ends the script.
set -e
set -o pipefail
cd "$(dirname "$0")/.."
LIB=diff-vit_amd/csrc/libp2vit_hip.so
cp $LIB /tmp/p2v_cur.so
trap 'cp /tmp/p2v_cur.so $LIB' EXIT
SPECS=$1; shift
for r in $(seq 1 ${ROUNDS:-2}); do
  for spec in $SPECS; do
    label=${spec%%=*}; rest=${spec#*=}
    lib=${rest%%,*}; envs=""
    if [ "$rest" != "$lib" ]; then envs=$(echo "${rest#*,}" | tr ',' ' '); fi
    if [ "$lib" = cur ]; then lib=/tmp/p2v_cur.so; fi
    cp $lib $LIB
    dump=""
    if [ -n "$DUMP" ]; then dump="--dump-outputs $DUMP/${label}_r$r"; fi
    env $envs timeout -k 10 ${RUN_LIMIT:-300} python bench.py --no-cpu-baseline --repeats 3 $dump "$@" 2>/dev/null | python -c "import json,sys; d=json.loads(sys.stdin.readlines()[-1]); print('$label', d['value'], d['ms_per_step'])"
  done
done
if [ -n "$DUMP" ]; then md5sum $DUMP/*/logits.npy; fi
