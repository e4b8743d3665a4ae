#!/usr/bin/env python3
"""Rate of the two insert paths for keys of three and four words (65 <= k <= 128): mode 1, the direct kernel (global
atomics), against mode 2, the partitioned path (kernels_nword_part.hip.hpp: P1n, the exact P2 on 256-bit items, Tn).

  headline   the workload of tools/k100_rate.py -- k = 100, canonical, 2 Gbp of 150 bp reads in ten batches into 2^30 slots --
             one timed run a process start being one number: `--headline MODE` prints the rate of the second of two runs, as
             k100_rate.py does, and with --stages the per-stage device times of that run (jfgpu_profile_spans: 0 direct
             count, 4 P1, 5 P2, 6 tile insert, 7 items direct).  The baseline of a comparison is the PARENT commit's own build
             running its own tools/k100_rate.py, never this branch's mode 1.
  sweep      `--sweep`: k = 65, 96, 100, 128, one batch of 1 MiB .. 1 GiB of reads counted and synced into 2^30 slots (2^31 at
             k = 128, the smallest table it has), mode 1 against mode 2, five timed runs each after one warm-up: median and
             spread (max - min); then mode 0 once: which path AUTO took, and the same content digest in all three modes.  The AUTO threshold (host_partition.inl: kNWordPartMinBytes) is read from it: the smallest
             batch at which mode 2 wins by more than the spread, "never" when there is none.

usage: python tools/nword_part_rate.py --headline 2 [--stages] | --sweep [--max-mib 1024]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jellyfish_amd import capi

L = 150
STAGES = {0: "direct count", 1: "add_keys", 4: "P1", 5: "P2", 6: "tile insert", 7: "items direct"}


def headline(mode, stages):
    k, lsize, n_reads = 100, 30, 13_333_333
    with capi.Table(k, 1 << lsize, canonical=True) as t:
        t.set_mode(mode)
        buf = t.malloc(n_reads * (L + 1) + 16)
        t.gen_reads_dev(buf, 0, n_reads, L, 42)
        t.reserve(n_reads * (L + 1))
        t.sync()
        for rep in range(2):
            t.clear()
            if stages and rep == 1:
                t.profile_enable(True)
                t.profile_reset()
            t0 = time.time()
            for i in range(10):
                a, b = n_reads * i // 10, n_reads * (i + 1) // 10
                t.count_ascii_dev(buf + a * (L + 1), (b - a) * (L + 1))
            t.sync()
            dt = time.time() - t0
        st = t.stats()
        c = t.counters()
        print("headline k", k, "mode", mode, "slots 2^%d" % t.info.lsize, "total", st.total, "distinct", st.distinct, "%.1f ms" % (dt * 1e3),
              "%.2f G k-mers/s" % (st.total / dt / 1e9), "direct", c["direct"], "tile_nword", c["tile_nword"], "p2_exact", c["p2_exact"],
              "stages on" if stages else "", flush=True)
        if stages:
            tot = {}
            for which, ms in t.profile_spans():
                tot[which] = tot.get(which, 0.0) + ms
            for which in sorted(tot):
                print("  stage %d (%s): %.2f ms" % (which, STAGES.get(which, "?"), tot[which]), flush=True)
        t.free(buf)


def one_batch(t, buf, nbytes, reps=5):
    times = []
    for rep in range(reps + 1):
        t.clear()
        t0 = time.time()
        t.count_ascii_dev(buf, nbytes)
        t.sync()
        if rep:
            times.append(time.time() - t0)
    return times


def sweep(max_mib):
    sizes = [m for m in (1, 4, 16, 64, 256, 1024) if m <= max_mib]
    for k in (65, 96, 100, 128):
        lsize = 31 if k == 128 else 30
        n_reads = (sizes[-1] << 20) // (L + 1)
        with capi.Table(k, 1 << lsize, canonical=True) as t:
            t.set_growth(False)
            buf = t.malloc(n_reads * (L + 1) + 16)
            t.gen_reads_dev(buf, 0, n_reads, L, 42)
            t.sync()
            for mib in sizes:
                nbytes = (mib << 20) // (L + 1) * (L + 1)
                row = {}
                digests = {}
                for mode in (1, 2, 0):
                    t.set_mode(mode)
                    ts = one_batch(t, buf, nbytes, reps=5 if mode else 1)
                    total = t.stats().total
                    row[mode] = (statistics.median(ts), max(ts) - min(ts), total)
                    digests[mode] = t.digest()
                    auto_took = "partitioned" if t.counters()["tile_nword"] else "direct"      # (mode 0 runs last)
                (m1, s1, n1), (m2, s2, n2) = row[1], row[2]
                assert n1 == n2 and digests[1] == digests[2] == digests[0], "the three modes hold different tables"
                wins = m2 + max(s1, s2) < m1
                print("sweep k %3d slots 2^%d batch %4d MiB  k-mers %10d  mode 1 %9.3f ms (spread %.3f) %6.2f G/s   mode 2 %9.3f ms (spread %.3f) %6.2f G/s   %s" % (
                    k, lsize, mib, n1, m1 * 1e3, s1 * 1e3, n1 / m1 / 1e9, m2 * 1e3, s2 * 1e3, n2 / m2 / 1e9,
                    "mode 2 wins by more than the spread" if wins else "mode 2 does not win") + "; auto: " + auto_took, flush=True)
            t.free(buf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--headline", type=int, choices=(1, 2))
    ap.add_argument("--stages", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--max-mib", type=int, default=1024)
    a = ap.parse_args()
    if capi.device_count() < 1:
        sys.exit("nword_part_rate: no device: a rate is measured on the GPU or not at all")
    if a.headline:
        headline(a.headline, a.stages)
    if a.sweep:
        sweep(a.max_mib)


if __name__ == "__main__":
    main()
