#!/bin/bash
# ONE box: the profile passes (kernel trace with the traced process's own line, PMC passes -> HBM traffic, stamped with the kernel
# sources), then the full bench line (which reports that traffic), the apply counters, and every fraction recomputed from those
# files -> DIR/*_TAG.*   (scripts/final_refresh.sh TAG DIR, DIR = where scripts/profile_bench.sh writes its summaries; copy to profiles/)
T=$1
D=${2:?usage: scripts/final_refresh.sh TAG DIR (the directory scripts/profile_bench.sh writes to)}
bash scripts/profile_bench.sh $T > $D/prof_$T.log 2>&1
cp $D/prof_${T}_traffic.json profiles/traffic_latest.json
python bench.py --full > $D/bench_$T.json 2> $D/bench_$T.err
bash scripts/profile_apply_pmc.sh $T > /dev/null 2>&1
python scripts/recompute_fractions.py $D/bench_$T.json $D/prof_$T.json > $D/onebox_$T.txt 2>&1
cat $D/onebox_$T.txt
