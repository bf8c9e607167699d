#!/bin/bash
# whole-step kernel trace of the bench (run on the GPU box) beside its --full record; the summaries are copied to profiles/ afterwards
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
O=${1:?usage: scripts/prof_step.sh OUT_DIR (relative to the repository root)}
mkdir -p $R/$O
cd $R
python bench.py --full > $O/bench.json 2> $O/bench.err
tail -1 $O/bench.json
rocprofv3 --kernel-trace --stats -d $O/step -o step --output-format csv -- python bench.py --full --quick > $O/step.log 2>&1
tail -1 $O/step.log | cut -c1-300
ls $O/step
