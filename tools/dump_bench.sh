#!/bin/bash
# tools/dump_bench.sh [LOG] -- `jellyfish-amd dump` and `count --text` at scale on one GPU: the device formatter against the
# host loops (JFGPU_DUMP_HOST=1, which is the code before the device path) on the same database, alternating, a warm-up
# and three timed runs each, outputs compared byte for byte; then one run per window size, one pair in the FASTA layout,
# `count --text` both ways (the Writing phase of --timing) and a sweep of database sizes 2^10 .. 2^24 (the big database's
# file cut after that many records) for JFGPU_DUMP_DEVICE_MIN.  The database is count -m 21 -C -s $SIZE over $N_READS random
# reads of 150 bases (tools/gen_random_reads.py): about 130 records a read.  Everything lives under $TMPDIR (local scratch)
# and is removed at the end.  Every step has its own time limit and the script stops at the first one that fails.
# profiles/dump_bench.txt is its output.
set -o pipefail
cd "$(dirname "$0")/.."
LOG=${1:-$PWD/dump_bench.txt}
mkdir -p "$(dirname "$LOG")"
D=${TMPDIR:-/tmp}/jf_dump_bench_$$
mkdir -p $D || exit 1
trap 'rm -rf $D' EXIT
CLI=${CLI:-$PWD/bin/jellyfish-amd}
export SOURCE_DATE_EPOCH=1700000000 JFGPU_DUMP_TRACE=1
{
echo "# $(date -u) ; scratch $D ; $(df -h $D | tail -1)"
timeout -k 10 200 python tools/gen_random_reads.py $D/reads.fa ${N_READS:-800000} 150 7 || exit 1
ls -l $D/reads.fa
t0=$(date +%s.%N)
timeout -k 10 300 $CLI count -m 21 -C -s ${SIZE:-256M} -o $D/db.jf $D/reads.fa || exit 1
echo "count: $(awk "BEGIN{print $(date +%s.%N) - $t0}") s"
ls -l $D/db.jf
HDR=$((9 + 10#$(head -c 9 $D/db.jf)))
RB=10                                                          # 6 key bytes + 4 count bytes
NREC=$(( ($(stat -c %s $D/db.jf) - HDR) / RB ))
echo "records=$NREC header_bytes=$HDR"
one() {   # name, database, dump arguments, env...
  name=$1; db=$2; args=$3; shift 3
  t0=$(date +%s.%N)
  env "$@" timeout -k 10 300 $CLI dump $args -o $D/$name.txt $db 2> $D/err || { cat $D/err; return 1; }
  t1=$(date +%s.%N)
  echo "$name wall_s=$(awk "BEGIN{print $t1 - $t0}") $(grep '^dump: ' $D/err)"
}
DEV="JFGPU_DUMP_DEVICE_MIN=0"
one dev_warm $D/db.jf -c $DEV || exit 1
one host_warm $D/db.jf -c JFGPU_DUMP_HOST=1 || exit 1
cmp $D/dev_warm.txt $D/host_warm.txt && echo "outputs identical: $(stat -c %s $D/dev_warm.txt) bytes" || { echo "OUTPUTS DIFFER"; exit 1; }
rm -f $D/dev_warm.txt $D/host_warm.txt
for i in 1 2 3; do
  one dev $D/db.jf -c $DEV || exit 1
  one host $D/db.jf -c JFGPU_DUMP_HOST=1 || exit 1
done
cmp $D/dev.txt $D/host.txt && echo "outputs identical" || { echo "OUTPUTS DIFFER"; exit 1; }
for w in ${WINDOWS:-262144 1048576 4194304 16777216 67108864}; do
  one dev_w$w $D/db.jf -c $DEV JFGPU_TEXT_WINDOW=$w || exit 1
  cmp $D/dev_w$w.txt $D/host.txt || { echo "OUTPUTS DIFFER at window $w"; exit 1; }
  rm -f $D/dev_w$w.txt
done
rm -f $D/dev.txt $D/host.txt
one dev_fasta $D/db.jf "" $DEV || exit 1
one host_fasta $D/db.jf "" JFGPU_DUMP_HOST=1 || exit 1
cmp $D/dev_fasta.txt $D/host_fasta.txt && echo "FASTA outputs identical: $(stat -c %s $D/dev_fasta.txt) bytes" || { echo "OUTPUTS DIFFER (FASTA)"; exit 1; }
rm -f $D/dev_fasta.txt $D/host_fasta.txt
# ---- count --text: the Writing phase with the device formatter and with the host loop
for p in dev host; do
  mkdir -p $D/ct_$p
  e=X=1; [ $p = host ] && e=JFGPU_DUMP_HOST=1
  (cd $D/ct_$p && env $e timeout -k 10 400 $CLI count -m 21 -C -s ${SIZE:-256M} --text --timing timing.txt -o out.jf $D/reads.fa 2> $D/err) || { cat $D/err; exit 1; }
  echo "count --text $p: $(grep -v '^$' $D/err | tr '\n' ' ') $(tr '\n' ' ' < $D/ct_$p/timing.txt)"
done
cmp $D/ct_dev/out.jf $D/ct_host/out.jf && echo "count --text outputs identical: $(stat -c %s $D/ct_dev/out.jf) bytes" || { echo "OUTPUTS DIFFER (count --text)"; exit 1; }
rm -rf $D/ct_dev $D/ct_host
# ---- the threshold: wall time of the whole process, start and HIP initialisation included, by database size
for b in ${SWEEP_BITS:-10 11 12 13 14 15 16 17 18 19 20 21 22 23 24}; do
  n=$((1 << b))
  [ $n -le $NREC ] || break
  head -c $((HDR + n * RB)) $D/db.jf > $D/cut.jf
  for i in 1 2 3; do
    one sweep_2^${b}_dev $D/cut.jf -c $DEV || exit 1
    one sweep_2^${b}_host $D/cut.jf -c JFGPU_DUMP_HOST=1 || exit 1
  done
  cmp "$D/sweep_2^${b}_dev.txt" "$D/sweep_2^${b}_host.txt" || { echo "OUTPUTS DIFFER at 2^$b records"; exit 1; }
  rm -f $D/sweep_*.txt
done
} 2>&1 | tee $LOG
