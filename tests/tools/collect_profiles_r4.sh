#!/bin/bash
# Round-4 evidence run on the MI355X box: rocprofv3 kernel statistics and PMC passes for bench.py and the stage benches.
# usage (from the repo root on the box): bash tests/tools/collect_profiles_r4.sh   -> gpurun_out/profiles_r4/
# (every step prints a line when it is done: the box's watchdog kills a command that is silent for seven minutes)
set -u
R=$PWD
O=$R/gpurun_out/profiles_r4
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
prof() { # name, program args...
  local name=$1; shift
  rm -rf /tmp/rp_$name
  rocprofv3 --kernel-trace --stats -d /tmp/rp_$name -o $name --output-format csv -- python3 "$@" > $O/$name.stdout 2> $O/$name.stderr
  find /tmp/rp_$name -name "*kernel_stats.csv" -exec cp {} $O/${name}_kernel_stats.csv \;
  echo "done $name"
}
pmc() { # name, kernel filter, counters..., then "--", program args
  local name=$1 kern=$2; shift 2
  local ctrs=()
  while [ "$1" != "--" ]; do ctrs+=("$1"); shift; done; shift
  rm -rf /tmp/rp_$name
  rocprofv3 --pmc "${ctrs[@]}" -d /tmp/rp_$name -o pmc --output-format csv -- python3 "$@" > /dev/null 2>&1
  python3 $R/tests/tools/pmc_summary.py /tmp/rp_$name --kernel $kern >> $O/$name.txt
  echo "done $name"
}
prof bench $R/bench.py --full --extra-file $O/bench_full.json
grep '^{' $O/bench.stdout | tail -1 > $O/bench.json
for c in FETCH_SIZE WRITE_SIZE; do
  rm -rf /tmp/rp_pmc_$c
  rocprofv3 --pmc $c -d /tmp/rp_pmc_$c -o pmc --output-format csv -- python3 $R/bench.py --steps 5 --warmup 1 --no-cpu --no-extra > /dev/null 2>&1
  python3 $R/tests/tools/pmc_summary.py /tmp/rp_pmc_$c --kernel k_jpeg420 > $O/pmc_$c.txt
  echo "done pmc $c"
done
prof jpeg_geoms $R/tests/tools/bench_jpeg_geoms.py
prof vp8_residual $R/tests/tools/bench_vp8_residual.py
prof intra_c5 $R/tests/tools/bench_intra_c5.py 6
pmc intra_c5_pmc k_hevc_intra_groups SQ_WAVES SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_BRANCH SQ_INSTS_VMEM_RD SQ_WAVE_CYCLES SQ_BUSY_CYCLES -- $R/tests/tools/bench_intra_c5.py 6
export MODE=frames FFHIP_VP8_FRAMES=fused FRAMES=256
prof vp8_frames256 $R/tests/tools/prof_vp8_batch.py
pmc vp8_frames256_pmc k_vp8_frames SQ_WAVES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_INSTS_VALU -- $R/tests/tools/prof_vp8_batch.py
pmc vp8_frames256_pmc k_vp8_frames SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_BRANCH SQ_ACTIVE_INST_SCA SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR -- $R/tests/tools/prof_vp8_batch.py
unset MODE FFHIP_VP8_FRAMES FRAMES
PICTURES=8 NO_CPU=1 prof hevc_grid8 $R/tests/tools/bench_hevc_grid.py
cd $R
NO_CPU=1 python3 tests/tools/bench_hevc_grid.py > $O/hevc_grid.json 2> /dev/null
echo "done hevc grid"
SIZES=16,64,256,1024 python3 tests/tools/bench_vp8_frames.py > $O/vp8_frames.jsonl 2> /dev/null
echo "done vp8 frames"
ls -la $O
# the planner's kernels as a timeline, the grouped kernel's wave-time accounting and the single picture's critical path (diagnostics build)
cd $R
bash tests/tools/prof_hevc_timeline.sh > /dev/null 2>&1; cp gpurun_out/hevc_timeline/grid_8.txt $O/hevc_timeline_grid8.txt; cp gpurun_out/hevc_timeline/grid_1.txt $O/hevc_timeline_grid1.txt; cp gpurun_out/hevc_timeline/one_8k.txt $O/hevc_timeline_8k.txt
echo "done timelines"
if [ -f ffpic_amd/libffpic_hip_trace.so ]; then
  python3 tests/tools/diag_intra_trace.py c5 > $O/intra_trace_c5.txt 2>&1; echo "done trace c5"
  PICTURES=1 python3 tests/tools/diag_intra_trace_grid.py > $O/intra_trace_grid1.txt 2>&1; echo "done trace grid 1"
  PICTURES=8 python3 tests/tools/diag_intra_trace_grid.py > $O/intra_trace_grid8.txt 2>&1; echo "done trace grid 8"
fi
ls -la $O | tail -12
