# round 3, GPU box: the whole -m gpu suite, the bench lines (1 and 8 utterances per GPU), rocprofv3 kernel traces and PMC passes
set -x
R=$GRAFT_REPO_ROOT; O=$R/gpurun_out/r3f; mkdir -p $O
cd $R
python -m pytest tests -q -m gpu --durations=12 > $O/pytest.log 2>&1; echo "pytest rc=$?" >> $O/pytest.log; tail -25 $O/pytest.log
python bench.py --full > $O/bench.json 2> $O/bench.err; echo "bench rc=$?"
python bench.py --full --utts 8 --no-extras --no-cpu-baseline > $O/bench8.json 2> $O/bench8.err; echo "bench8 rc=$?"
cd /tmp; export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $O/kt1 -- python $R/bench.py --full --steps 200 --warmup 20 --no-extras --no-cpu-baseline > /dev/null 2>&1
rocprofv3 --kernel-trace --stats --output-format csv -d $O/kt8 -- python $R/bench.py --full --steps 200 --warmup 20 --utts 8 --no-extras --no-cpu-baseline > /dev/null 2>&1
for c in FETCH_SIZE WRITE_SIZE; do
  rocprofv3 --kernel-trace --pmc $c --output-format csv -d $O/pmc1_$c -- python $R/bench.py --full --steps 40 --warmup 5 --no-extras --no-cpu-baseline > /dev/null 2>&1
done
rocprofv3 --kernel-trace --stats --output-format csv -d $O/ktc -- python $R/tools/codec_bench.py 32 30 > $O/codec32.txt 2>&1
cd $R
python tools/prof_summary.py $(ls $O/kt1/*/*kernel_trace.csv | head -1) $O/r03_decode_kernel_trace_summary.md > /dev/null
python tools/prof_summary.py $(ls $O/kt8/*/*kernel_trace.csv | head -1) $O/r03_decode16rows_kernel_trace_summary.md > /dev/null
python tools/prof_summary.py $(ls $O/ktc/*/*kernel_trace.csv | head -1) $O/r03_codec_b32_kernel_trace_summary.md > /dev/null
for c in FETCH_SIZE WRITE_SIZE; do python tools/pmc_summary.py $(ls $O/pmc1_$c/*/*counter_collection.csv | head -1) $O/r03_pmc1_$c.md > /dev/null; done
cp $(ls $O/kt1/*/*kernel_stats.csv | head -1) $O/r03_rocprofv3_kernel_stats.csv; cp $(ls $O/kt8/*/*kernel_stats.csv | head -1) $O/r03_rocprofv3_kernel_stats_16rows.csv
rm -rf $O/kt1 $O/kt8 $O/ktc $O/pmc1_*
ls -la $O
