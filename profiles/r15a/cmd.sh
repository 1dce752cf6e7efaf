# r15a: the GPU visit of the exhaustive searches' consolidation (every GPU step under its own time limit, the steps
# chained).  PARENT: libpmmg_hip.so built from the parent commit's sources with the flags of parmmg_amd/build.py.
set -o pipefail
NEW=$PWD/parmmg_amd/libpmmg_hip.so
# 1. the new test, the transfer calls of both builds, the suites of the new build
timeout -k 10 240 python3 -u -m pytest tests/test_gpu_fallback_edges.py -m gpu -x -q -s --durations=15 && \
timeout -k 10 430 python3 -u tools/identity_ab.py $PARENT $NEW identity_vs_parent.txt && \
timeout -k 10 600 python3 -u -m pytest tests -m gpu -x -q --durations=10 && \
timeout -k 10 120 python3 -c "import __graft_entry__ as g; g.smoke()"
# 2. speed: parent and new alternately, three rounds, one process per run; each run's result line -> speed/<tool>_<build><round>.json
for r in 1 2 3; do for b in parent new; do
  if [ $b = parent ]; then export PMMG_HIP_SO=$PARENT; else export PMMG_HIP_SO=$NEW; fi
  timeout -k 10 300 python3 -u bench.py --gpus 1 --steps 20 --warmup 3 --full --no-cpu-baseline --no-host-mode --no-quality \
    --no-snapshot --no-surface-solo --no-graded > speed/bench_$b$r.log && \
  timeout -k 10 120 python3 -u tools/groups_only.py --no-parity > speed/groups_$b$r.log && \
  timeout -k 10 120 python3 -u tools/fallback_time.py --rounds 20 > speed/fallback_$b$r.log && \
  timeout -k 10 200 python3 -u tools/sweep.py --config cfg4 --steps 10 --child perm=shuffle > speed/shuffled_$b$r.log || break 2
done; done
python3 profiles/r15a/speed_cmp.py speed 3 > speed_vs_parent.txt
# without a GPU: bash tools/resource_usage.sh (both trees), the device assembly of the six .hip files (both trees,
# the flags in device_assembly_cmp.txt), python -m pytest -m "not gpu"
