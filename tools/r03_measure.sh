# Round-3 measurement set (run on the GPU box: gpurun -- 'bash tools/r03_measure.sh'); everything
# lands in gpurun_out/r03/ and is copied from there into profiles/.
R=$GRAFT_REPO_ROOT
O=$R/gpurun_out/r03
mkdir -p $O
cd $R
for cfg in cfg2 cfg3 cfg1 cfg4; do
  python bench.py --full --preset $cfg --steps 20 > $O/bench_$cfg.json 2> $O/bench_$cfg.err
done
python bench.py --full --preset longtail --steps 4 --no-pmc --api-reads 0 > $O/bench_longtail.json 2> $O/bench_longtail.err
python bench.py --full --gpus 2 --steps 6 > $O/bench_cfg5_rehearsal_2ranks_on_1gpu.json 2> $O/bench_n2.err
# kernel stats of the cfg2 run (rocprofv3 --kernel-trace --stats), same command as the bench line
cd /tmp && export TMPDIR=/tmp
rm -rf /tmp/r03_stats
rocprofv3 --kernel-trace --stats -d /tmp/r03_stats -- python $R/bench.py --steps 3 --warmup 1 --no-pmc --no-cpu-baseline --e2e none --api-reads 0 > $O/bench_line_under_rocprof.json 2>/dev/null
python $R/tools/rocpd_summary.py $(find /tmp/r03_stats -name "*.db" | head -1) > $O/kernel_stats_10k_reads.txt
rm -rf /tmp/r03_stats4
rocprofv3 --kernel-trace --stats -d /tmp/r03_stats4 -- python $R/bench.py --preset cfg4 --steps 3 --warmup 1 --no-pmc --no-cpu-baseline --e2e none --api-reads 0 > /dev/null 2>&1
python $R/tools/rocpd_summary.py $(find /tmp/r03_stats4 -name "*.db" | head -1) > $O/kernel_stats_cfg4_rna.txt
# SQ counters of the DP kernels per preset
for cfg in cfg2 cfg3 cfg1; do
  rm -rf /tmp/r03_sq
  rocprofv3 --kernel-trace --pmc SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES SQ_INSTS_SALU GRBM_GUI_ACTIVE -d /tmp/r03_sq -- python $R/bench.py --preset $cfg --steps 1 --warmup 0 --no-pmc --no-cpu-baseline --e2e none --api-reads 0 > /dev/null 2>&1
  python $R/tools/pmc_sq.py $(find /tmp/r03_sq -name "*.db" | head -1) 10000 $([ $cfg = cfg1 ] && echo 2000 || echo 10000) > $O/pmc_sq_counters_$cfg.txt 2>&1
done
cd $R
[ -x alt_builds/occupancy ] || hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -o alt_builds/occupancy tools/occupancy.hip
alt_builds/occupancy > $O/occupancy.txt 2>&1
ls -la $O
