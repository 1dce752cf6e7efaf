# r13a: the GPU visits of the contiguity change (each block one visit, every GPU step under its own time limit)
set -o pipefail
# 1. the new tests
timeout -k 10 420 python3 -m pytest tests/test_gpu_contig.py -m gpu -x -q -s --durations=15
# 2. the new tests again, the whole GPU suite, smoke(), the C-ABI program of ctest
timeout -k 10 300 python3 -m pytest tests/test_gpu_contig.py -m gpu -x -q && \
timeout -k 10 900 python3 -u -m pytest tests -m gpu -x -q --durations=10 && \
timeout -k 10 120 python3 -c "import __graft_entry__ as g; g.smoke()" && \
timeout -k 10 120 tests/c/test_c_abi tests/golden
# 3. the timing tool on cfg2, then cfg4, then bench.py of the parent commit's tree (exported and built beside this
#    one as _ab/parent) and of this tree, alternating
timeout -k 10 150 python3 -u tools/contiguity_time.py --config cfg2 --out bench_out/r13a/contiguity_cfg2.json && \
timeout -k 10 400 python3 -u tools/contiguity_time.py --config cfg4 --out bench_out/r13a/contiguity_cfg4.json
for i in 1 2 3 4; do
  (cd _ab/parent && timeout -k 10 200 python3 -u bench.py --gpus 1 --steps 20 --warmup 3 --no-cpu-baseline) && \
  timeout -k 10 200 python3 -u bench.py --gpus 1 --steps 20 --warmup 3 --no-cpu-baseline || break
done
# resource usage (no GPU): the flags of parmmg_amd/build.py plus -Rpass-analysis=kernel-resource-usage
SRC=pmmg_contig.hip bash tools/resource_usage.sh k_contig
