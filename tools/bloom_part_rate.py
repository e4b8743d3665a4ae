#!/usr/bin/env python3
"""Rate of the two insert paths of a Bloom counter for mers of 33 to 128 bases: mode 1, the direct kernels (one global
compare-and-swap per cell), against mode 2, the partitioned path (kernels_bloom_part_keys.hip.hpp: P1b over keys of two to
four words, then the one-word keys' P2 and segment kernel).

  workload   canonical, k = 63 and k = 100, 2 Gbp of 150 bp reads generated on the device, a counter of opt_m(0.001, n) cells
             and opt_k(0.001) hashes for the n k-mers of the input.  A timed run is insert_ascii_dev x 10 (ten batches) plus
             sync; one warm-up, then five timed runs in one session: median and spread (max - min).  --stages: the per-stage
             device times of mode 2's last run (jfgpu_bc_profile_get 0 .. 4).
  sweep      `--sweep`: one batch of 1 MiB .. 1 GiB of reads inserted and synced, the same five runs after a warm-up.
  baseline   The baseline of any claim is the PARENT commit's own build running this script's mode-1 workload (JFGPU_LIB names
             that build's library; it refuses mode 2 for these keys, so `--modes 1`), never this branch's mode 1.
  k = 31     `--k 31 --modes 0`: the one-word counter on the same workload, as the engine chooses (the regression line: its
             kernels are not supposed to change).

The AUTO rule (bloom_partition.inl: kBloomKeysPartMinBytes) is read from the sweep: the smallest batch from which mode 2
beats the parent's mode 1 by more than the larger of the two spreads, "never" when there is none.

usage: python tools/bloom_part_rate.py [--k 63,100] [--modes 1,2] [--stages] [--sweep [--max-mib 1024]]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from jellyfish_amd import capi

L = 150
STAGES = {0: "direct", 1: "P1b", 2: "P2", 3: "segments", 4: "(ring P2 launches, inside P2)"}


def timed(b, buf, pieces, reps=5):
    """one warm-up, then `reps` timed runs of clear + inserts + sync; seconds each, and the k-mers fed"""
    times, fed = [], 0
    for rep in range(reps + 1):
        b.clear()
        b.sync()
        if rep == reps:
            b.profile_reset()
        t0 = time.time()
        for off, n in pieces:
            b.insert_ascii_dev(buf + off, n)
        fed = b.sync()
        if rep:
            times.append(time.time() - t0)
    return times, fed


def counter(k, n_reads):
    n = n_reads * (L - k + 1)
    return capi.Bloom(k, capi.opt_m(0.001, n), capi.opt_k(0.001), canonical=True), n


def set_mode(b, mode):
    try:
        b.set_mode(mode)
        return True
    except capi.JfgpuError as e:
        print("  mode %d refused: %s" % (mode, e), flush=True)
        return False


def report(tag, k, mode, times, fed):
    med, spread = statistics.median(times), max(times) - min(times)
    print("%s k %3d mode %d  k-mers %11d  median %9.3f ms  spread %8.3f ms  %6.3f G k-mers/s   runs %s" % (
        tag, k, mode, fed, med * 1e3, spread * 1e3, fed / med / 1e9, " ".join("%.1f" % (t * 1e3) for t in times)), flush=True)


def headline(t, ks, modes, stages):
    n_reads = 13_333_333                                          # 2 Gbp
    buf = t.malloc(n_reads * (L + 1) + 16)
    t.gen_reads_dev(buf, 0, n_reads, L, 42)
    t.sync()
    pieces = [(n_reads * i // 10 * (L + 1), (n_reads * (i + 1) // 10 - n_reads * i // 10) * (L + 1)) for i in range(10)]
    for k in ks:
        b, n = counter(k, n_reads)
        with b:
            print("headline k %d: %d cells (%.2f GB), %d hashes" % (k, b.m, b.nb_bytes / 1e9, b.nb_hashes), flush=True)
            for mode in modes:
                if not set_mode(b, mode):
                    continue
                b.profile_enable(bool(stages))
                times, fed = timed(b, buf, pieces)
                assert fed == n, (fed, n)
                report("headline", k, mode, times, fed)
                if stages:
                    for i in range(5):
                        ms, launches, units = b.profile_get(i)
                        print("  stage %d (%s): %.2f ms, %d launches" % (i, STAGES[i], ms, launches), flush=True)
    t.free(buf)


def sweep(t, ks, modes, max_mib):
    sizes = [m for m in (1, 4, 16, 64, 256, 1024) if m <= max_mib]
    n_reads = (sizes[-1] << 20) // (L + 1)
    buf = t.malloc(n_reads * (L + 1) + 16)
    t.gen_reads_dev(buf, 0, n_reads, L, 42)
    t.sync()
    for k in ks:
        for mib in sizes:
            nr = (mib << 20) // (L + 1)
            b, n = counter(k, nr)
            with b:
                for mode in modes:
                    if not set_mode(b, mode):
                        continue
                    times, fed = timed(b, buf, [(0, nr * (L + 1))])
                    assert fed == n, (fed, n)
                    report("sweep %4d MiB" % mib, k, mode, times, fed)
    t.free(buf)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", default="63,100")
    ap.add_argument("--modes", default="1,2")
    ap.add_argument("--stages", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--no-headline", action="store_true")
    ap.add_argument("--max-mib", type=int, default=1024)
    a = ap.parse_args()
    if capi.device_count() < 1:
        sys.exit("bloom_part_rate: no device: a rate is measured on the GPU or not at all")
    ks = [int(x) for x in a.k.split(",")]
    modes = [int(x) for x in a.modes.split(",")]
    print("library:", capi.LIB_PATH, flush=True)
    with capi.Table(21, 1 << 16, canonical=True) as t:             # (the reads' generator and the device allocator are the table's)
        if not a.no_headline:
            headline(t, ks, modes, a.stages)
        if a.sweep:
            sweep(t, ks, modes, a.max_mib)


if __name__ == "__main__":
    main()
