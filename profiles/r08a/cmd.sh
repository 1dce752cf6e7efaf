# r08a: the GPU visits of the mesh reports (pmmg_hip_qual_histo / pmmg_hip_edge_lengths); each line one
# visit, every GPU step under its own time limit
set -o pipefail
export TMPDIR=/tmp
# 1. the new tests, then the timing tool on cfg4's adapted mesh in three numberings (both hash modes each)
timeout -k 10 300 python3 -u -m pytest tests/test_mesh_stats.py -m gpu -x -q && \
python3 tools/gpu_job.py --tag r08a \
  "py tools/mesh_stats_time.py --config cfg4 --rounds 5 --out bench_out/r08a/mesh_stats.json" \
  "py tools/mesh_stats_time.py --config cfg4 --rounds 3 --numbering mmg --out bench_out/r08a/mesh_stats_mmg.json" \
  "py tools/mesh_stats_time.py --config cfg4 --rounds 3 --numbering shuffled --out bench_out/r08a/mesh_stats_shuffled.json"
# 2. the whole GPU suite, smoke(), one benchmark run
timeout -k 10 900 python3 -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread && \
timeout -k 10 120 python3 -c "import __graft_entry__ as g; g.smoke()" && \
timeout -k 10 280 python3 -u bench.py --gpus 1 --steps 20 --warmup 3
