#!/bin/bash
# usage (GPU box, repo root): tools/r03_run.sh <tag> [pytest|bench|prof|kern ...]   - one gpurun call, everything under gpurun_out/<tag>/
tag=${1:-r03}; shift
what=${*:-pytest bench}
cd "${GRAFT_REPO_ROOT:-.}"; export TMPDIR=/tmp
out=gpurun_out/$tag; mkdir -p $out
for w in $what; do
  case $w in
    pytest) timeout -k 10 1500 python -m pytest tests -m gpu -q --maxfail=25 --timeout 600 --durations=15 -p no:cacheprovider > $out/pytest_gpu.log 2>&1; tail -40 $out/pytest_gpu.log ;;
    opb) timeout -k 10 900 python tools/op_bench.py > $out/op_bench.json 2> $out/op_bench.err; tail -30 $out/op_bench.json ;;
    pypar) timeout -k 10 900 python -m pytest tests/test_gpu_parity.py tests/test_gpu_random_parity.py -m gpu -q --maxfail=10 --timeout 600 --durations=8 -p no:cacheprovider > $out/pytest_par.log 2>&1; tail -25 $out/pytest_par.log ;;
    pykm) timeout -k 10 900 python -m pytest tests/test_gpu_kmeans.py -m gpu -q --timeout 600 -p no:cacheprovider > $out/pytest_km.log 2>&1; tail -15 $out/pytest_km.log ;;
    pyacc) timeout -k 10 600 python -m pytest tests/test_gpu_kmeans.py -m gpu -q -k "accumulate or counting or objective or golden or bounds" --timeout 600 -p no:cacheprovider > $out/pytest_acc.log 2>&1; tail -3 $out/pytest_acc.log ;;
    pydur) timeout -k 10 900 python -m pytest tests/test_gpu_dist.py tests/test_gpu_parity.py -m gpu -q -k "rccl or ranking or rank_all or 2d_split" --durations=12 --timeout 600 -p no:cacheprovider > $out/pytest_dur.log 2>&1; tail -25 $out/pytest_dur.log ;;
    bench) timeout -k 10 900 python bench.py --full > $out/bench.json 2> $out/bench.err; tail -c 1500 $out/bench.json; echo; tail -5 $out/bench.err ;;
    benchq) timeout -k 10 600 python bench.py --full --dedup-rows 0 --kmeans-rows 0 --no-cpu-baseline > $out/bench_quick.json 2> $out/bench_quick.err; tail -c 1500 $out/bench_quick.json; echo; tail -5 $out/bench_quick.err ;;
    prof) SKIP_BENCH=1 timeout -k 10 1500 tools/profile_bench.sh $tag/prof > $out/prof.log 2>&1; tail -30 $out/prof.log ;;
    kern) timeout -k 10 1500 tools/profile_kernels.sh $tag/kern > $out/kern.log 2>&1; tail -30 $out/kern.log ;;
    kmprof) timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $out/kmprof -o km -- python tools/kmeans_iter_workload.py > $out/kmprof.log 2>&1; tail -5 $out/kmprof.log ;;
    kmprofb) timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $out/kmprofb -o km -- python tools/kmeans_iter_workload.py 10000000 blobs > $out/kmprofb.log 2>&1; tail -5 $out/kmprofb.log ;;
    sweep) make -C lotus_amd/csrc tuning -j8 > $out/tuning_build.log 2>&1; timeout -k 10 600 python tools/small_batch_sweep.py > $out/small_batch_sweep.log 2>&1; cat $out/small_batch_sweep.log ;;
    sbtrace) timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $out/sbtrace -o sb -- python tools/small_batch_sweep.py trace > $out/sbtrace.log 2>&1; tail -3 $out/sbtrace.log ;;
    kmdebug) timeout -k 10 600 python tools/kmeans_bounds_debug.py > $out/kmdebug.log 2>&1; tail -60 $out/kmdebug.log ;;
    kmtime) timeout -k 10 600 python tools/kmeans_iter_workload.py 10000000 both blobs > $out/kmtime.log 2>&1; tail -20 $out/kmtime.log ;;
    kmtrace) timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $out/kmtrace -o km -- python tools/kmeans_iter_workload.py 10000000 bounds blobs > $out/kmtrace.log 2>&1; grep iterations $out/kmtrace.log ;;
    smoke) timeout -k 10 300 python -c 'import __graft_entry__ as g; g.smoke()' > $out/smoke.log 2>&1; tail -3 $out/smoke.log ;;
    *) echo "unknown step $w" ;;
  esac
done
find $out -name "*.db" -delete 2>/dev/null
echo done
