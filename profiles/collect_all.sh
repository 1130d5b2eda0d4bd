#!/bin/bash
# Everything under profiles/ that is measured on the GPU box, in one call from the repo root:
#   profiles/collect_all.sh TAG OUTDIR   (round tag; OUTDIR/<tag>_* are then copied into profiles/)
TAG=${1:-r03}
OUT=${2:?usage: profiles/collect_all.sh TAG OUTDIR}
R=${GRAFT_REPO_ROOT:-$(pwd)}
cd $R
mkdir -p $OUT
S=profiles/tune/steps.sh
$S "timeout -k 10 500 bash profiles/collect.sh $TAG > $OUT/${TAG}_collect.log 2>&1; tail -2 $OUT/${TAG}_collect.log | cut -c1-400" \
   "timeout -k 10 400 bash profiles/collect_sq.sh > $OUT/${TAG}_collect_sq.log 2>&1; tail -3 $OUT/${TAG}_collect_sq.log" \
   "NFST_TUNING=1 NFST_LIB=nfst_amd/lib/variants/libnfst_hip_prof.so timeout -k 10 200 python profiles/tune/stamps.py 256 4 > $OUT/${TAG}_stage_stamps.txt 2>&1; NFST_TUNING=1 NFST_LIB=nfst_amd/lib/variants/libnfst_hip_prof.so timeout -k 10 200 python profiles/tune/stamps.py 256 1 >> $OUT/${TAG}_stage_stamps.txt 2>&1; grep -c . $OUT/${TAG}_stage_stamps.txt" \
   "timeout -k 10 300 python profiles/bench_ingest.py 64 > $OUT/${TAG}_ingest.json 2> $OUT/${TAG}_ingest.err; tail -c 300 $OUT/${TAG}_ingest.json" \
   "timeout -k 10 400 python profiles/bench_secondary.py > $OUT/${TAG}_secondary_kernels.json 2> $OUT/${TAG}_secondary.err; tail -c 300 $OUT/${TAG}_secondary_kernels.json" \
   "timeout -k 10 400 bash profiles/collect_secondary.sh > $OUT/${TAG}_collect_secondary.log 2>&1; tail -3 $OUT/${TAG}_collect_secondary.log" \
   "timeout -k 10 300 python profiles/tune/deep_times.py > $OUT/${TAG}_deep_lattices.txt 2>&1; cat $OUT/${TAG}_deep_lattices.txt | grep -v amdgpu" \
   "timeout -k 10 300 python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err; tail -c 200 $OUT/${TAG}_bench.json"
