#!/bin/bash
# Round-4 evidence, run on the GPU box through gpurun on the round's FINAL build.  Everything lands in gpurun_out/r04_final/ and every file carries the sha256 of the
# libpgo.so that produced it (first line / "libpgo_sha256" key); scripts/pmc_r04_summary.py then writes the files committed under profiles/.
#   part "gate": the driver's own test command, the same under PGO_DEBUG_POISON=1, the once-red test 20x in separate processes
#   part "prof": rocprofv3 kernel stats + PMC passes + bench line + per-config rows + session replay + multi-rank checks
export TMPDIR=/tmp
OUT=gpurun_out/r04_final
PM=gpurun_out/r04_final/pmc
mkdir -p gpurun_out/r04_final/pmc
python -c "from solve_keyframe_pose_graph_amd import _build; _build.build_libpgo(); _build.build_host(); _build.build_graphgen()"   # (the snapshot's file times can make the shipped library look stale: whatever the loader would rebuild is rebuilt NOW, before the sha is taken)
SHA=$(sha256sum solve_keyframe_pose_graph_amd/libpgo.so | cut -d' ' -f1)
echo $SHA > $OUT/libpgo_sha256.txt
stamp() { sed -i "1i # libpgo.so sha256 $SHA" "$1"; }
PARTS=${1:-gate,prof}
if [[ $PARTS == *gate* ]]; then
  {
    echo "## python -m pytest tests/ -x -q -m gpu      (the driver's command)"
    timeout 1500 python -m pytest tests/ -x -q -m gpu -p no:cacheprovider 2>&1 | grep -v "^RCCL\|^HIP\|^ROCm\|^Hostname\|^Librccl" | tail -6
    echo "## PGO_DEBUG_POISON=1 python -m pytest tests/ -q -m gpu      (every new device allocation NaN-filled)"
    PGO_DEBUG_POISON=1 timeout 1500 python -m pytest tests/ -q -m gpu -p no:cacheprovider 2>&1 | grep -v "^RCCL\|^HIP\|^ROCm\|^Hostname\|^Librccl" | tail -6
    echo "## 20 separate processes of: python -m pytest tests/test_gpu_coarse.py -q -m gpu -k small_configs      (the test that was red in GPUTEST_r03)"
    for i in $(seq 1 20); do timeout 300 python -m pytest tests/test_gpu_coarse.py -q -m gpu -p no:cacheprovider -k small_configs 2>&1 | grep "passed\|failed" | sed 's/ in .*//'; done | sort | uniq -c
    echo "## python -m pytest tests -m gpu --collect-only -q | head -12      (oracle anchors of C1..C5 first)"
    python -m pytest tests -m gpu --collect-only -q -p no:cacheprovider 2>/dev/null | head -12
  } > $OUT/r04_gate.txt 2>&1
  stamp $OUT/r04_gate.txt
fi
[[ $PARTS == *prof* ]] || exit 0
trace() {   # trace <name> <stats file> <command...>: rocprofv3 --kernel-trace --stats of a command, summarised, the raw database dropped
  local name=$1 stats=$2; shift 2
  rocprofv3 --kernel-trace --stats -d gpurun_out/r04_final/trace_$name -o t -- "$@" > $OUT/trace_$name.log 2>&1
  python scripts/rocpd_summary.py stats $(find gpurun_out/r04_final/trace_$name -name "*.db" | head -1) > $OUT/$stats; stamp $OUT/$stats
  rm -rf gpurun_out/r04_final/trace_$name
}
pmc() {     # pmc <name> <counters...> -- <command...>: one --pmc pass; leaves the database for pmc_sum, which removes it
  local name=$1; shift; local ctr=(); while [ "$1" != "--" ]; do ctr+=("$1"); shift; done; shift
  rocprofv3 --kernel-trace --pmc "${ctr[@]}" -d gpurun_out/r04_final/pmc/db_$name -o pmc -- "$@" > $PM/$name.log 2>&1
}
pmc_sum() { python scripts/rocpd_summary.py pmc $(find gpurun_out/r04_final/pmc/db_$1 -name "*.db" | head -1) $2 $3 > $PM/$4; }
pmc_drop() { rm -rf gpurun_out/r04_final/pmc/db_$1; }
trace mg r04_mg_kernel_stats.txt python scripts/gpu_mg_profile.py
trace k1big r04_k1_400k_kernel_stats.txt python scripts/k1_only.py 400000
trace session r04_session_kernel_stats.txt python scripts/research/session_one_solve.py 3000
for c in FETCH_SIZE WRITE_SIZE; do
  pmc k1_$c $c -- python scripts/k1_only.py; pmc_sum k1_$c $c k1_edges_kernel k1_$c.json; pmc_drop k1_$c
  pmc pcg_$c $c -- python scripts/gpu_pcg_kernel_times.py C3; pmc_sum pcg_$c $c mf_spmv pcg_spmv_$c.json; pmc_sum pcg_$c $c cg_update pcg_update_$c.json; pmc_drop pcg_$c
  pmc mg_$c $c -- python scripts/gpu_mg_iteration_only.py; pmc_sum mg_$c $c pgo mg_all_$c.json; pmc_drop mg_$c
done
pmc pcg_l2 TCC_HIT_sum TCC_MISS_sum -- python scripts/gpu_pcg_kernel_times.py C3
for c in TCC_HIT_sum TCC_MISS_sum; do pmc_sum pcg_l2 $c mf_spmv pcg_spmv_$c.json; pmc_sum pcg_l2 $c cg_update pcg_update_$c.json; done; pmc_drop pcg_l2
pmc pcg_sq SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU -- python scripts/gpu_pcg_kernel_times.py C3
for c in SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_BUSY_CYCLES SQ_ACTIVE_INST_VALU; do pmc_sum pcg_sq $c mf_spmv pcg_spmv_$c.json; pmc_sum pcg_sq $c cg_update pcg_update_$c.json; done; pmc_drop pcg_sq
# the PMC passes condensed NOW (on this box) so that the bench below reports the static traffic figures of exactly this build, then the bench line (driver's command)
cp profiles/r04_cpu_c3_full.json $OUT/ 2>/dev/null
python scripts/pmc_r04_summary.py $OUT > $OUT/pmc_summary.log 2>&1
cp profiles/k1_pmc_latest.json profiles/k1_pmc_r04.json profiles/pcg_pmc_latest.json profiles/mg_pmc_latest.json profiles/r04_pcg_pmc.txt $OUT/ 2>/dev/null
python bench.py --full --steps 20 --warmup 5 > $OUT/r04_bench.json 2> $OUT/bench.err
rocprofv3 --kernel-trace --stats -d $OUT/trace_bench -o t -- python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --no-k1-out-of-cache > $OUT/r04_bench_under_rocprof.json 2> $OUT/bench_rocprof.err
python scripts/rocpd_summary.py stats $(find gpurun_out/r04_final/trace_bench -name "*.db" | head -1) > $OUT/r04_bench_kernel_stats.txt; stamp $OUT/r04_bench_kernel_stats.txt
rm -rf gpurun_out/r04_final/trace_bench
python scripts/dev/mf_timeline.py C3 > $OUT/r04_mf_timeline.txt 2>&1; stamp $OUT/r04_mf_timeline.txt
python scripts/dev/verbose_solve.py C3 2 2>&1 | grep "build_graph\|hierarchy (host)" > $OUT/r04_build_phases.txt; stamp $OUT/r04_build_phases.txt
python scripts/gpu_all_configs.py > $OUT/r04_all_configs.txt 2>&1; stamp $OUT/r04_all_configs.txt
python scripts/gpu_mg_graph_types.py 20 > $OUT/r04_mg_graph_types.txt 2>&1; stamp $OUT/r04_mg_graph_types.txt
python scripts/gpu_session_replay.py 3000 600 100 2 > $OUT/r04_session_replay_2deg.jsonl 2> $OUT/replay.err
python scripts/research/session_step_times.py 400,1000,3000 2>&1 | grep -v "^\[pgo\]" > $OUT/r04_session_step_times.txt; stamp $OUT/r04_session_step_times.txt
python scripts/gpu_multi_overhead.py > $OUT/multi_overhead.log 2>&1
python scripts/gpu_multi_overhead.py mg > $OUT/multi_overhead_mg.log 2>&1
python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29517 bench.py --full --gpus 2 --steps 10 --warmup 2 --collective gloo > $OUT/r04_bench_gloo2.json 2> $OUT/bench_gloo2.err
python bench.py --full --config C5 --steps 5 --warmup 1 --no-cpu-baseline > $OUT/r04_bench_c5_strong_1gpu.json 2> $OUT/bench_c5.err
cp gpurun_out/multi_overhead.json $OUT/r04_multi_overhead.json 2>/dev/null; cp gpurun_out/multi_overhead_mg.json $OUT/r04_multi_overhead_mg.json 2>/dev/null
python scripts/pmc_r04_summary.py $OUT > $OUT/pmc_summary.log 2>&1
ls -la $OUT $PM
