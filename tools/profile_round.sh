#!/bin/bash
# tools/profile_round.sh TAG — on an MI355X: bench line + rocprofv3 kernel trace + HBM-traffic PMC passes, all under $OUT/TAG_* (OUT defaults to profile_out)
TAG=${1:-rXX}
cd /tmp && export TMPDIR=/tmp
cd $GRAFT_REPO_ROOT
export OUT=${OUT:-profile_out}
mkdir -p $OUT
python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
rocprofv3 --kernel-trace -d $OUT/${TAG}_kt -o kt -- python bench.py --steps 20 --warmup 3 --no-secondary --no-cpu-baseline > $OUT/${TAG}_kt.log 2>&1
python tools/rocpd_summary.py $(find $OUT/${TAG}_kt -name "*.db" | head -1) > $OUT/${TAG}_kernel_stats.txt
LVX_SERIAL=1 rocprofv3 --kernel-trace -d $OUT/${TAG}_kts -o kt -- python bench.py --steps 20 --warmup 3 --no-secondary --no-cpu-baseline > $OUT/${TAG}_kts.log 2>&1
python tools/rocpd_summary.py $(find $OUT/${TAG}_kts -name "*.db" | head -1) > $OUT/${TAG}_kernel_stats_serial.txt
for c in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --pmc $c --output-format csv -d $OUT/${TAG}_pmc_$c -o pmc -- python bench.py --steps 5 --warmup 1 --no-secondary --no-cpu-baseline > $OUT/${TAG}_pmc_$c.log 2>&1
done
python tools/pmc_summary.py $OUT/${TAG}_pmc_FETCH_SIZE $OUT/${TAG}_pmc_WRITE_SIZE > $OUT/${TAG}_pmc_hbm.txt
tail -1 $OUT/${TAG}_bench.json | cut -c1-600
