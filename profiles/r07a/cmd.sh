# r07a: the GPU visits of the point-map change (each line one visit, every GPU step under its own time limit)
set -o pipefail
export TMPDIR=/tmp
# 1. the new tests, then the A/B tool on cfg2 as a check of the tool
timeout -k 10 420 python3 -u -m pytest tests/test_gpu_point_map.py -m gpu -x -q --timeout 120 --timeout-method thread && \
timeout -k 10 240 python3 -u tools/point_map_ab.py --configs cfg2 --rounds 3 --out bench_out/r07a/point_map_cfg2.json
# 2. the whole GPU suite, then smoke()
timeout -k 10 900 python3 -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread && \
timeout -k 10 120 python3 -c "import __graft_entry__ as g; g.smoke()"
# 3. the A/B on cfg3 and cfg4
python3 tools/gpu_job.py --tag r07a "py tools/point_map_ab.py --out bench_out/r07a/point_map.json"
# 4. / 5. bench.py of this tree and of the parent commit's tree (exported and built beside it), alternating
for i in 1 2 3 4 5 6 7 8 9; do
  timeout -k 10 280 python3 -u bench.py --gpus 1 --steps 20 --warmup 3 --no-cpu-baseline && \
  (cd _ab/parent && timeout -k 10 280 python3 -u bench.py --gpus 1 --steps 20 --warmup 3 --no-cpu-baseline) || break
done
# resource usage (no GPU): both builds with the flags of parmmg_amd/build.py plus -Rpass-analysis=kernel-resource-usage
