#!/bin/bash
# tools/merge_bench.sh [LOG] -- `jellyfish-amd merge` at scale on one GPU: the device path against the host heap
# (JFGPU_MERGE_HOST=1, which is the code before the device path) on the same sorted runs, alternating, a warm-up and three
# timed runs each, outputs compared byte for byte; then one run per window size.  The runs are those of
# count -m 21 -C -s $SIZE --disk --no-merge over $N_READS random reads of 150 bases (tools/gen_random_reads.py) with at
# least $MIN_RECORDS records; everything lives under $TMPDIR (local scratch) and is removed at the end.  Every step has its
# own time limit and the script stops at the first one that fails.  profiles/merge_bench.txt is its output.
set -o pipefail
cd "$(dirname "$0")/.."
LOG=${1:-$PWD/merge_bench.txt}
mkdir -p "$(dirname "$LOG")"
D=${TMPDIR:-/tmp}/jf_merge_bench_$$
mkdir -p $D || exit 1
trap 'rm -rf $D' EXIT
CLI=${CLI:-$PWD/bin/jellyfish-amd}
export SOURCE_DATE_EPOCH=1700000000 JFGPU_MERGE_TRACE=1
{
echo "# $(date -u) ; scratch $D ; $(df -h $D | tail -1)"
timeout -k 10 200 python tools/gen_random_reads.py $D/reads.fa ${N_READS:-2400000} 150 7 || exit 1
ls -l $D/reads.fa
t0=$(date +%s.%N)
timeout -k 10 400 $CLI count -m 21 -C -s ${SIZE:-128M} --disk --no-merge -o $D/run $D/reads.fa || exit 1
echo "count --disk --no-merge: $(awk "BEGIN{print $(date +%s.%N) - $t0}") s"
ls -l $D/
RUNS=""
for f in $D/run[0-9]*; do
  n=$($CLI stats $f | awk '/Distinct/ {print $2}')
  echo "$f distinct=$n"
  [ "$n" -ge ${MIN_RECORDS:-50000000} ] && RUNS="$RUNS $f"
done
echo "merging:$RUNS"
[ $(echo $RUNS | wc -w) -ge 2 ] || { echo "fewer than two runs of 50 M records"; exit 1; }
one() {   # name, env...
  name=$1; shift
  t0=$(date +%s.%N)
  mkdir -p $D/$name
  (cd $D/$name && env "$@" timeout -k 10 300 $CLI merge -o out.jf $RUNS 2> $D/err) || { cat $D/err; return 1; }
  t1=$(date +%s.%N)
  echo "$name wall_s=$(awk "BEGIN{print $t1 - $t0}") $(grep '^merge: ' $D/err)"
}
one dev_warm X=1 || exit 1
one host_warm JFGPU_MERGE_HOST=1 || exit 1
cmp $D/dev_warm/out.jf $D/host_warm/out.jf && echo "outputs identical: $(stat -c %s $D/dev_warm/out.jf) bytes" || { echo "OUTPUTS DIFFER"; exit 1; }
for i in 1 2 3; do
  one dev X=1 || exit 1
  one host JFGPU_MERGE_HOST=1 || exit 1
done
cmp $D/dev/out.jf $D/host/out.jf && echo "outputs identical" || { echo "OUTPUTS DIFFER"; exit 1; }
for w in ${WINDOWS:-1000000 4000000 16000000 33554432}; do
  one dev_w$w JFGPU_MERGE_WINDOW=$w || exit 1
  cmp $D/dev_w$w/out.jf $D/host/out.jf || { echo "OUTPUTS DIFFER at window $w"; exit 1; }
  rm -rf $D/dev_w$w
done
} 2>&1 | tee $LOG
