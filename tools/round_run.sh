# tools/round_run.sh TAG — on the GPU box: the whole evidence set of a state: GPU tests, bench line, kernel traces (concurrent + serial), HBM traffic counters,
# SQ counters, timeline, LM-iteration trace; everything under $OUT/TAG_* (OUT defaults to profile_out)
TAG=${1:-rXX}
cd /tmp && export TMPDIR=/tmp; cd $GRAFT_REPO_ROOT
export OUT=${OUT:-profile_out}
mkdir -p $OUT
timeout 2400 python -m pytest tests -m gpu -x -q > $OUT/${TAG}_gpu_tests.log 2>&1; grep -n "passed\|failed" $OUT/${TAG}_gpu_tests.log | tail -2
bash tools/profile_round.sh $TAG
bash tools/pmc_sq.sh; cp $OUT/pmc_sq_summary.txt $OUT/${TAG}_pmc_sq.txt
python tools/make_traffic_json.py $OUT/${TAG}_pmc_FETCH_SIZE $OUT/${TAG}_pmc_WRITE_SIZE "profiles/${TAG}_pmc_hbm_traffic.txt" $OUT/pmc_sq2 "profiles/${TAG}_pmc_sq.txt" > $OUT/${TAG}_latest_traffic.json
python tools/rocpd_timeline.py $(find $OUT/${TAG}_kt -name "*.db" | head -1) 12 > $OUT/${TAG}_timeline.txt
rm -rf $OUT/${TAG}_lm
timeout 300 rocprofv3 --kernel-trace -d $OUT/${TAG}_lm -o kt -- python tools/lm_iter_probe.py 8 > $OUT/${TAG}_lm.log 2>&1
python tools/rocpd_summary.py $(find $OUT/${TAG}_lm -name "*.db" | head -1) > $OUT/${TAG}_kernel_stats_lm_iteration.txt
grep "^lm \|solve_step" $OUT/${TAG}_lm.log | cut -c1-120
rm -rf $OUT/${TAG}_lm $OUT/${TAG}_kt $OUT/${TAG}_kts $OUT/${TAG}_pmc_FETCH_SIZE $OUT/${TAG}_pmc_WRITE_SIZE $OUT/pmc_sq1 $OUT/pmc_sq2
