#!/bin/bash
# tools/query_sorted_bench.sh [LOG] -- `jellyfish-amd query -s` of a binary/sorted database at scale on one GPU: the look-up in
# the sorted records (this tree's default) against the parent commit's CLI, which loads the records into a hash table, on the
# same files, in the manner of tools/query_text_bench.sh.  $N_READS random reads of 150 bases (tools/gen_random_reads.py;
# 630000 reads are a 97 MB FASTA) are counted into a 21-mer database (count -m 21 -C) and into a 100-mer one (count -m 100
# -C), and the same FASTA is the query of both.  Per database: one warm-up of each CLI, then $RUNS timed runs alternating, wall
# time and the JFGPU_QUERY_TRACE line of every run, the output written to a file on local scratch, outputs compared with cmp;
# the medians of wall_s, load_ms and kernels_ms; this tree's own table path (JFGPU_QUERY_TABLE=1) once; 4, 8 and 16 records
# a bucket (JFGPU_QUERY_PER_BUCKET), $RUNS runs each; and the device bytes of both paths (tools/sorted_info.py: jfgpu_sorted_info
# of the file's records, jfgpu_get_info of a table of the header's size).
# The parent's CLI is $PARENT_CLI, by default build/parent/bin/jellyfish-amd: the parent commit's tree exported into
# build/parent and built there (where there is no GPU and git is at hand), which git ignores.
# Everything else lives under $TMPDIR (local scratch) and is removed at the end.  Every step has its own time limit and the
# script stops at the first one that fails.  profiles/query_sorted_bench.txt is its output.
set -o pipefail
cd "$(dirname "$0")/.."
LOG=${1:-$PWD/query_sorted_bench.txt}
mkdir -p "$(dirname "$LOG")"
CLI=${CLI:-$PWD/bin/jellyfish-amd}
PARENT_CLI=${PARENT_CLI:-$PWD/build/parent/bin/jellyfish-amd}
if [ ! -x "$PARENT_CLI" ]; then
  echo "building the parent commit's CLI into build/parent" >&2
  rm -rf build/parent && mkdir -p build/parent || exit 1
  git archive ${PARENT:-HEAD^} | tar -x -C build/parent || exit 1
  make -s -C build/parent engine cli || exit 1
fi
[ "${BUILD_ONLY:-0}" = 1 ] && exit 0
D=${TMPDIR:-/tmp}/jf_query_sorted_bench_$$
mkdir -p $D || exit 1
trap 'rm -rf $D' EXIT
RUNS=${RUNS:-5}
LIMIT=${LIMIT:-600}                                            # seconds a single query may take
export SOURCE_DATE_EPOCH=1700000000 JFGPU_QUERY_TRACE=1
{
echo "# $(date -u) ; scratch $D ; $(df -h $D | tail -1)"
timeout -k 10 300 python tools/gen_random_reads.py $D/reads.fa ${N_READS:-630000} 150 7 || exit 1
ls -l $D/reads.fa
for k in 21 100; do
  t0=$(date +%s.%N)
  timeout -k 10 300 $CLI count -m $k -C -s ${SIZE:-256M} -o $D/db$k.jf $D/reads.fa || exit 1
  echo "count -m $k: $(awk "BEGIN{print $(date +%s.%N) - $t0}") s"
done
ls -l $D/db21.jf $D/db100.jf
one() {   # name, cli, database, env...
  name=$1; cli=$2; db=$3; shift 3
  t0=$(date +%s.%N)
  env "$@" timeout -k 10 $LIMIT $cli query $db -s $D/reads.fa -o $D/$name.txt 2> $D/err || { cat $D/err; return 1; }
  t1=$(date +%s.%N)
  echo "$name wall_s=$(awk "BEGIN{print $t1 - $t0}") $(grep '^query: ' $D/err)"
}
median() {  # name, field: the median of that field over the lines of $D/log that begin with the name
  grep "^$1 " $D/log | tr ' ' '\n' | grep "^$2=" | cut -d= -f2 | sort -g | awk '{v[NR] = $1} END {if(NR) print v[int((NR + 1) / 2)]; else print "-"}'
}
medians() { echo "$1 medians of $(grep -c "^$1 " $D/log): wall_s=$(median $1 wall_s) load_ms=$(median $1 load_ms) kernels_ms=$(median $1 kernels_ms)"; }
pair() {  # label, database
  label=$1; db=$2
  : > $D/log
  one ${label}_records_warm $CLI $db X=1 || return 1
  one ${label}_parent_warm $PARENT_CLI $db X=1 || return 1
  cmp $D/${label}_records_warm.txt $D/${label}_parent_warm.txt && echo "$label: outputs identical: $(stat -c %s $D/${label}_records_warm.txt) bytes, $(wc -l < $D/${label}_records_warm.txt) lines" || { echo "$label: OUTPUTS DIFFER"; return 1; }
  rm -f $D/${label}_records_warm.txt $D/${label}_parent_warm.txt
  for i in $(seq 1 $RUNS); do
    one ${label}_records $CLI $db X=1 | tee -a $D/log || return 1
    one ${label}_parent $PARENT_CLI $db X=1 | tee -a $D/log || return 1
  done
  cmp $D/${label}_records.txt $D/${label}_parent.txt && echo "$label: outputs identical" || { echo "$label: OUTPUTS DIFFER"; return 1; }
  medians ${label}_records; medians ${label}_parent
  one ${label}_table $CLI $db JFGPU_QUERY_TABLE=1 || return 1
  cmp $D/${label}_table.txt $D/${label}_parent.txt || { echo "$label: OUTPUTS DIFFER (this tree's table path)"; return 1; }
  rm -f $D/${label}_records.txt $D/${label}_table.txt
  for per in 4 8 16; do
    for i in $(seq 1 $RUNS); do one ${label}_per$per $CLI $db JFGPU_QUERY_PER_BUCKET=$per | tee -a $D/log || return 1; done
    cmp $D/${label}_per$per.txt $D/${label}_parent.txt || { echo "$label: OUTPUTS DIFFER ($per records a bucket)"; return 1; }
    medians ${label}_per$per
    rm -f $D/${label}_per$per.txt
  done
  rm -f $D/${label}_*.txt
  timeout -k 10 300 python tools/sorted_info.py $db || return 1
}
pair k21 $D/db21.jf || exit 1
pair k100 $D/db100.jf || exit 1
} 2>&1 | tee $LOG
