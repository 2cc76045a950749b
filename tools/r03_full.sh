#!/bin/bash
# Round-3 GPU call: PMC passes (mj_k_sp instruction counts, mj_k_encode HBM bytes at the bench's own 65,536 tables) -> their
# summaries under profiles/ of the box's copy, THEN the whole -m gpu suite, the default bench line (which reads those summaries),
# rocprofv3 kernel stats of the v4 / v3 bench, the issue-rate microbenchmark, the 2-rank gloo smoke run of bench.py --gpus 2 and __graft_entry__.smoke().
# Output: gpurun_out/$1/ (profiles/ sub-directory = the files to commit).
TAG=${1:-r03}; OUT=/root/repo/gpurun_out/$TAG; mkdir -p $OUT/profiles; cd /root/repo
/root/repo/tools/bin/ubench_valu > $OUT/profiles/r03_ubench_valu.jsonl 2> $OUT/ubench.err; echo "ubench rc=$?"
cd /tmp && export TMPDIR=/tmp
timeout 300 rocprofv3 --pmc WRITE_SIZE --kernel-include-regex 'mj_k_encode' --output-format csv -d $OUT/pmc_write -- python /root/repo/bench.py --steps 6 --warmup 3 --no-cpu-baseline --no-matrix --version 4 > $OUT/pmc_write.log 2>&1
timeout 300 rocprofv3 --pmc FETCH_SIZE --kernel-include-regex 'mj_k_encode' --output-format csv -d $OUT/pmc_fetch -- python /root/repo/bench.py --steps 6 --warmup 3 --no-cpu-baseline --no-matrix --version 4 > $OUT/pmc_fetch.log 2>&1
cd /root/repo; tools/pmc_sp.sh ${TAG}_pmc_sp 65536 > $OUT/pmc_sp.log 2>&1; tail -2 $OUT/pmc_sp.log
python tools/summarize_sp_pmc.py gpurun_out/${TAG}_pmc_sp r03 > $OUT/summarize_sp.log 2>&1; tail -3 $OUT/summarize_sp.log
cd /tmp
timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/v4_stats -- python /root/repo/bench.py --steps 20 --warmup 6 --no-cpu-baseline --no-matrix --version 4 > $OUT/v4_stats.log 2>&1
timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/v3_stats -- python /root/repo/bench.py --steps 60 --warmup 20 --no-cpu-baseline --no-matrix --version 3 > $OUT/v3_stats.log 2>&1
cd /root/repo; python tools/summarize_profiles.py $OUT r03 65536 > $OUT/summarize.log 2>&1; tail -2 $OUT/summarize.log
cp profiles/r03_* profiles/pmc_encode.json $OUT/profiles/ 2>/dev/null
timeout 600 python bench.py --full > $OUT/bench.json 2> $OUT/bench.err; echo "bench rc=$?"; cut -c1-400 $OUT/bench.json
cp $OUT/bench.json $OUT/profiles/r03_bench_v4.json
timeout 300 python bench.py --gpus 2 --dist-backend gloo --tables 8192 --steps 10 --warmup 3 --preroll 256 --no-cpu-baseline --no-matrix 2> $OUT/gloo.err | grep '^{' > $OUT/profiles/r03_bench_gloo_2ranks_1gpu.json; echo "gloo 2-rank rc=$?"; cut -c1-300 $OUT/profiles/r03_bench_gloo_2ranks_1gpu.json
timeout 300 python -c 'import __graft_entry__ as g; g.smoke(); print("smoke ok")' > $OUT/smoke.log 2>&1; echo "smoke rc=$?"; tail -1 $OUT/smoke.log
timeout 1500 python -m pytest tests -m gpu -q --durations=10 > $OUT/gputest.log 2>&1; echo "gputest rc=$?"; tail -4 $OUT/gputest.log
rm -rf $OUT/pmc_write $OUT/pmc_fetch $OUT/v4_stats $OUT/v3_stats; du -sh $OUT
