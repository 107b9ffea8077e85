# one training-step profile: per-layer standalone table, then the kernel trace of bench.py -> timeline + per-kernel totals
# usage: tools/r03_step_profile.sh TAG OUTDIR   (the bench line needs --full: the recorded JSON carries `roofline` and `phases`)
cd /tmp && export TMPDIR=/tmp
R=$GRAFT_REPO_ROOT
TAG=${1:-r03_mid}
O=${2:?usage: tools/r03_step_profile.sh TAG OUTDIR}
mkdir -p $O
python3 $R/tools/conv_bench.py --shapes all --kinds fwd,dgrad,wgrad --iters 10 --pre --stats --add > $O/${TAG}_conv_layers.txt 2>&1
rm -rf $O/prof_step
rocprofv3 --kernel-trace -d $O/prof_step -o x -- python3 $R/bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-extras > $O/${TAG}_bench_under_rocprof.json 2> $O/${TAG}_bench_under_rocprof.err
DB=$(find $O/prof_step -name "*.db" | head -1)
python3 $R/tools/rocpd_timeline.py $DB 2 multi_tensor_apply > $O/${TAG}_step_timeline.txt 2>&1
python3 $R/tools/rocpd_stats.py $DB $O/${TAG}_bench_kernel_stats.csv > /dev/null 2>&1
rm -rf $O/prof_step
