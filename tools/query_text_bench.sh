#!/bin/bash
# tools/query_text_bench.sh [LOG] -- `jellyfish-amd query -s` at scale on one GPU, this tree's CLI against the parent
# commit's on the same databases: the case DESIGN.md 3.7a records.  $N_READS random reads of 150 bases
# (tools/gen_random_reads.py; 630000 reads are a 100 MB FASTA and 82 M 21-mers) are counted into a binary/sorted database
# (count -m 21 -C) and inserted into a Bloom counter (bc -m 21 -C), and the same FASTA is the query of both.  Per database:
# one warm-up of each CLI, then $RUNS timed runs alternating (Bloom counter: $BLOOM_RUNS; the parent answers those on one host
# thread), wall time and the JFGPU_QUERY_TRACE line of every run, the output written to a file on local scratch, outputs
# compared with cmp.  Then this tree's CLI once with the lines built on the host (JFGPU_QUERY_FORMAT_HOST=1) and once with
# everything on the host, for the split of its wall time.
# The parent's CLI is $PARENT_CLI, by default build/parent/bin/jellyfish-amd: the parent commit's tree exported into
# build/parent and built there (where there is no GPU and git is at hand), which git ignores.
# Everything else lives under $TMPDIR (local scratch) and is removed at the end.  Every step has its own time limit and the
# script stops at the first one that fails.  profiles/query_text_bench.txt is its output.
set -o pipefail
cd "$(dirname "$0")/.."
LOG=${1:-$PWD/query_text_bench.txt}
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
D=${TMPDIR:-/tmp}/jf_query_text_bench_$$
mkdir -p $D || exit 1
trap 'rm -rf $D' EXIT
RUNS=${RUNS:-5}
BLOOM_RUNS=${BLOOM_RUNS:-$RUNS}
LIMIT=${LIMIT:-900}                                            # seconds a single query may take
export SOURCE_DATE_EPOCH=1700000000 JFGPU_QUERY_TRACE=1
{
echo "# $(date -u) ; scratch $D ; $(df -h $D | tail -1)"
timeout -k 10 300 python tools/gen_random_reads.py $D/reads.fa ${N_READS:-630000} 150 7 || exit 1
ls -l $D/reads.fa
t0=$(date +%s.%N)
timeout -k 10 300 $CLI count -m 21 -C -s ${SIZE:-256M} -o $D/db.jf $D/reads.fa || exit 1
echo "count: $(awk "BEGIN{print $(date +%s.%N) - $t0}") s"
t0=$(date +%s.%N)
timeout -k 10 300 $CLI bc -m 21 -C -s ${BC_SIZE:-100M} -o $D/db.bc $D/reads.fa || exit 1
echo "bc: $(awk "BEGIN{print $(date +%s.%N) - $t0}") s"
ls -l $D/db.jf $D/db.bc
one() {   # name, cli, database, env...
  name=$1; cli=$2; db=$3; shift 3
  t0=$(date +%s.%N)
  env "$@" timeout -k 10 $LIMIT $cli query $db -s $D/reads.fa -o $D/$name.txt 2> $D/err || { cat $D/err; return 1; }
  t1=$(date +%s.%N)
  echo "$name wall_s=$(awk "BEGIN{print $t1 - $t0}") $(grep '^query: ' $D/err)"
}
pair() {  # label, database, timed runs
  label=$1; db=$2; runs=$3
  one ${label}_new_warm $CLI $db X=1 || return 1
  one ${label}_parent_warm $PARENT_CLI $db X=1 || return 1
  cmp $D/${label}_new_warm.txt $D/${label}_parent_warm.txt && echo "$label: outputs identical: $(stat -c %s $D/${label}_new_warm.txt) bytes, $(wc -l < $D/${label}_new_warm.txt) lines" || { echo "$label: OUTPUTS DIFFER"; return 1; }
  rm -f $D/${label}_new_warm.txt $D/${label}_parent_warm.txt
  for i in $(seq 1 $runs); do
    one ${label}_new $CLI $db X=1 || return 1
    one ${label}_parent $PARENT_CLI $db X=1 || return 1
  done
  cmp $D/${label}_new.txt $D/${label}_parent.txt && echo "$label: outputs identical" || { echo "$label: OUTPUTS DIFFER"; return 1; }
  one ${label}_new_format_host $CLI $db JFGPU_QUERY_FORMAT_HOST=1 || return 1
  cmp $D/${label}_new_format_host.txt $D/${label}_parent.txt || { echo "$label: OUTPUTS DIFFER (format on the host)"; return 1; }
  rm -f $D/${label}_new.txt $D/${label}_new_format_host.txt
  if [ "${HOST_RUN:-1}" = 1 ]; then
    one ${label}_new_all_host $CLI $db JFGPU_QUERY_HOST=1 || return 1
    cmp $D/${label}_new_all_host.txt $D/${label}_parent.txt || { echo "$label: OUTPUTS DIFFER (all on the host)"; return 1; }
  fi
  rm -f $D/${label}_*.txt
}
pair binary $D/db.jf $RUNS || exit 1
pair bloom $D/db.bc $BLOOM_RUNS || exit 1
} 2>&1 | tee $LOG
