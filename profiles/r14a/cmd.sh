# r14a: the GPU visit of the mesh-service consolidation (every GPU step under its own time limit, the steps chained).
# PARENT: libpmmg_hip.so built from the parent commit's sources with the flags of parmmg_amd/build.py.
set -o pipefail
NEW=$PWD/parmmg_amd/libpmmg_hip.so
# 1. refusal texts and checksums, one fresh process per build; the listings are compared from line 2 on
PMMG_HIP_SO=$PARENT timeout -k 10 120 python3 -u profiles/r14a/services_ab.py > services_parent.txt && \
PMMG_HIP_SO=$NEW timeout -k 10 120 python3 -u profiles/r14a/services_ab.py > services_new.txt && \
# 2. the transfer calls
timeout -k 10 300 python3 -u tools/identity_ab.py $PARENT $NEW identity_vs_parent.txt && \
# 3. the suites of the new build
timeout -k 10 900 python3 -u -m pytest tests -m gpu -x -q --durations=10 && \
timeout -k 10 120 python3 -c "import __graft_entry__ as g; g.smoke()"
# 4. speed: parent and new alternately, three rounds, one process per run
for r in 1 2 3; do for b in parent new; do
  if [ $b = parent ]; then export PMMG_HIP_SO=$PARENT; else export PMMG_HIP_SO=$NEW; fi
  timeout -k 10 400 python3 -u tools/metis_graph_time.py --config cfg2 --out speed_cfg2/graph_$b$r.json && \
  timeout -k 10 400 python3 -u tools/mesh_stats_time.py --config cfg2 --out speed_cfg2/stats_$b$r.json && \
  timeout -k 10 400 python3 -u tools/contiguity_time.py --config cfg2 --out speed_cfg2/contig_$b$r.json && \
  timeout -k 10 300 python3 -u tools/snap_only.py cfg2 5 > speed_cfg2/snap_$b$r.log && \
  timeout -k 10 300 python3 -u bench.py --gpus 1 --steps 20 --warmup 3 --no-cpu-baseline > speed_cfg2/bench_$b$r.log || break 2
done; done
# 5. metis_graph_time and mesh_stats_time again at cfg2, five rounds (speed_cfg2_again/); the four tools at cfg4,
#    three rounds, as in 4 with --config cfg4 and without bench.py (speed_cfg4/)
