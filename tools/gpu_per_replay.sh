#!/bin/bash
# per-replay kernel census of the headline step (tools/per_replay_counts.py): two kernel-trace runs, 10 and 30 timed steps
set -e
: "${OUT:?set OUT to the folder, relative to the repository root, that receives the outputs}"
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
mkdir -p "$R/$OUT"
for n in 10 30; do
  rm -rf /tmp/prc_$n
  rocprofv3 --kernel-trace --stats -d /tmp/prc_$n -o t --output-format csv -- python3 $R/bench.py --steps $n --warmup 5 --full --no-kernel-timing --no-cpu-baseline > $R/$OUT/prc_$n.json 2> $R/$OUT/prc_$n.err
  cp $(find /tmp/prc_$n -name "*kernel_stats.csv" | head -1) $R/$OUT/prc_${n}_kernel_stats.csv
done
python3 $R/tools/per_replay_counts.py $R/$OUT/prc_10_kernel_stats.csv $R/$OUT/prc_30_kernel_stats.csv 40 > $R/$OUT/r4_per_replay.txt
head -50 $R/$OUT/r4_per_replay.txt
