#!/usr/bin/env python3
"""Rate of jfgpu_query_ascii_dev (query_ascii_kernel: roll + canonical + look-up fused) next to jfgpu_lookup_dev
(lookup_kernel) on the same k-mers already encoded in device memory -- the numbers of profiles/query_bench.txt and
DESIGN.md.

Shape: k = 21 -C and k = 31 -C; a table of 2^30 slots counted from the synthetic-read generator (jfgpu_gen_reads_dev, 150 bp
reads) to a load of about one half; a query buffer of 1 Gbp from the same generator whose read range overlaps the counted
one in part, so that some windows are present and the rest absent.  The keys lookup_kernel gets are the query buffer's
canonical k-mers, written by the routing pass of a one-shard table (jfgpu_partition_ascii_dev).

Timing: the engine's own device-event pairs around each launch (jfgpu_profile_enable: slot 8 query, slot 3 look-up), two
warm-up launches of each, then the two kernels alternate for --reps timed launches each; median, min and max.
usage: python tools/query_bench.py [--reps 12] [--gbp 1.0] [--out profiles/query_bench.txt]"""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jellyfish_amd import capi

L = 150
SLOT_QUERY, SLOT_LOOKUP = 8, 3


def spread(ms):
    return "median %.2f ms (min %.2f, max %.2f, n = %d)" % (statistics.median(ms), min(ms), max(ms), len(ms))


def run(k, lsize, n_count, n_query, reps, say):
    stride = L + 1
    with capi.Table(k, 1 << lsize, canonical=True) as t:
        nq = n_query * stride
        d_cnt = t.malloc(n_count * stride + 16)
        d_q = t.malloc(nq + 16)
        d_vals = t.malloc(8 * nq)
        d_flags = t.malloc(nq)
        d_keys = t.malloc(8 * nq)
        try:
            t.gen_reads_dev(d_cnt, 0, n_count, L, 42)
            t.gen_reads_dev(d_q, n_count - n_count // 3, n_query, L, 42)      # the first n_count / 3 reads were counted
            t.reserve(n_count * stride)
            t.count_ascii_dev(d_cnt, n_count * stride)
            t.sync()
            st = t.stats()
            n_keys = int(t.partition_ascii_dev(d_q, nq, d_keys, nq)[0])
            # the two kernels agree on a small piece (sums over its windows), then the timed launches
            small = 1000 * stride
            t.query_ascii_dev(d_q, small, d_vals, d_flags)
            t.wait()
            qv = t.d2h(d_vals, 8 * small).view(np.uint64)
            qf = t.d2h(d_flags, small)
            n_small = int(t.partition_ascii_dev(d_q, small, d_keys + 8 * (nq - small), small)[0])
            t.lookup_dev(d_keys + 8 * (nq - small), n_small, d_vals, d_flags)
            t.wait()
            lv = t.d2h(d_vals, 8 * n_small).view(np.uint64)
            lf = t.d2h(d_flags, n_small)
            assert int((qf & 1).sum()) == n_small and int(((qf & 2) != 0).sum()) == int(lf.sum()) and int(qv.sum()) == int(lv.sum()), \
                "query_ascii and lookup disagree"
            n_keys = int(t.partition_ascii_dev(d_q, nq, d_keys, nq)[0])
            t.profile_enable(True)
            for rep in range(reps + 2):
                if rep == 2:
                    t.wait(); t.profile_reset()
                t.query_ascii_dev(d_q, nq, d_vals, d_flags)
                t.lookup_dev(d_keys, n_keys, d_vals, d_flags)
            t.wait()
            spans = t.profile_spans()
            q_ms = [ms for w, ms in spans if w == SLOT_QUERY]
            l_ms = [ms for w, ms in spans if w == SLOT_LOOKUP]
            found = int(t.d2h(d_flags, min(n_keys, 1 << 24)).sum())
            qm, lm = statistics.median(q_ms), statistics.median(l_ms)
            say("k = %d -C, table 2^%d slots of %d bytes, %d distinct k-mers (load %.2f); query buffer %d bytes, %d k-mers, "
                "%.0f %% of the first 2^24 found" % (k, t.info.lsize, t.info.slot_bytes, st.distinct, st.distinct / float(1 << t.info.lsize),
                                                    nq, n_keys, 100.0 * found / min(n_keys, 1 << 24)))
            say("  query_ascii_kernel  %s  %.2f G positions/s  %.2f G k-mers/s" % (spread(q_ms), nq / qm / 1e6, n_keys / qm / 1e6))
            say("  lookup_kernel       %s  %.2f G k-mers/s (keys encoded beforehand, 8 bytes each)" % (spread(l_ms), n_keys / lm / 1e6))
            say("  query / lookup time ratio %.3f; lookup's own spread (max - min) / median %.3f" % (qm / lm, (max(l_ms) - min(l_ms)) / lm))
        finally:
            for p in (d_cnt, d_q, d_vals, d_flags, d_keys):
                t.free(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--gbp", type=float, default=1.0)
    ap.add_argument("--lsize", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert capi.device_count() > 0, "query_bench needs a GPU"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    n_query = int(a.gbp * 1e9 / (L + 1))
    n_count = (1 << a.lsize) // 2 // (L - 21 + 1)
    for k in (21, 31):
        run(k, a.lsize, n_count, n_query, a.reps, say)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
