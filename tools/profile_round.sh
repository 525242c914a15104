#!/bin/bash
# One GPU session: the full bench line (--full), rocprofv3 kernel trace of the bench, PMC passes (one counter group each) over the
# roofline kernels.  Outputs under <out> (copy what is judged into profiles/).   bash tools/profile_round.sh <tag> [<out>]
set -u
TAG=${1:-r02}
export OUT=${2:-profile_out}
mkdir -p $OUT
export TMPDIR=/tmp
python bench.py --full > $OUT/${TAG}_bench.log 2>&1
tail -1 $OUT/${TAG}_bench.log > $OUT/${TAG}_bench_line.json
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_${TAG} -o bench -- python bench.py --steps 20 --warmup 2 --no-cpu-baseline --no-clip --no-multi-edit > $OUT/${TAG}_prof_bench.log 2>&1
python tools/summarize_profile.py $OUT/prof_${TAG} --steps 22 > $OUT/${TAG}_bench_kernel_summary.md 2>&1
for grp in "FETCH_SIZE" "WRITE_SIZE" "SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU SQ_INSTS_MFMA SQ_VALU_MFMA_BUSY_CYCLES" "SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_SALU SQ_INSTS_VMEM SQ_WAIT_INST_LDS SQ_INSTS_VALU_TRANS SQ_WAVES" "GRBM_GUI_ACTIVE GRBM_COUNT"; do
  name=$(echo $grp | cut -d' ' -f1)
  rocprofv3 --kernel-trace --pmc $grp --output-format csv -d $OUT/pmc_${TAG}_${name} -o t -- python tools/pmc_targets.py > $OUT/pmc_${TAG}_${name}.log 2>&1
done
python tools/pmc_traffic.py $OUT/${TAG}_traffic.json $OUT/pmc_${TAG}_FETCH_SIZE $OUT/pmc_${TAG}_WRITE_SIZE > /dev/null 2>&1
python tools/pmc_summary.py $OUT/pmc_${TAG}_* > $OUT/${TAG}_pmc_raw.txt 2>&1
# kernel durations inside the PMC passes' traces (for the clock: GRBM_GUI_ACTIVE / duration)
python - <<'PY' > $OUT/${TAG}_pmc_durations.txt 2>&1
import csv, glob, collections, os
out = os.environ["OUT"]
for d in sorted(glob.glob(f"{out}/pmc_*_GRBM_GUI_ACTIVE")) + sorted(glob.glob(f"{out}/pmc_*_FETCH_SIZE")):
    acc = collections.defaultdict(list)
    for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            acc[r["Kernel_Name"].split("(")[0][-70:]].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print(d)
    for k, v in acc.items():
        print(f"  {k:<72s} n={len(v)} mean {sum(v)/len(v):9.1f} us  min {min(v):9.1f}")
PY
rm -rf $OUT/prof_${TAG}/*/*.db 2>/dev/null
tail -c 3000 $OUT/${TAG}_bench_line.json
echo
head -30 $OUT/${TAG}_bench_kernel_summary.md
cat $OUT/${TAG}_pmc_durations.txt
# keep the output small: the summaries and the stats CSVs stay, the raw per-dispatch traces go
mkdir -p $OUT/${TAG}_keep
cp $OUT/prof_${TAG}/*/*kernel_stats.csv $OUT/${TAG}_bench_kernel_stats.csv 2>/dev/null
du -sh $OUT/* 2>/dev/null | sort -h | tail -8
find $OUT -type f -size +6M -delete
rmdir $OUT/${TAG}_keep 2>/dev/null
