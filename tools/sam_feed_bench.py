#!/usr/bin/env python3
"""`count --sam` feed on one MI355X: BGZF inflate and BAM decode on the device against the FASTQ feed and host zlib.

Builds, once, under --workdir (local disk; removed at the end unless --keep): a BAM of --gbp Gbp of 150 bp reads with
qualities (windows of a random genome of --genome bases, so the table stays small), compressed at zlib level 6 like
bgzip, and the same reads as FASTQ.  Then reports, as one JSON object (stdout, and --out):

  inflate_GBps          device inflate, uncompressed bytes out per second of kernel time (HIP events, jfgpu_parser_last_ms)
  decode_GBps           BAM record decode (guess / fix / list / emit kernels), inflated bytes per second of kernel time
  sam_count_Gkmers_s    `jellyfish-amd count -m 21 -C --sam x.bam`: k-mers over the Counting phase (--timing)
  fastq_count_Gkmers_s  the same reads as FASTQ through the existing device parser, same measure
  host_zlib_GBps        16 processes of zlib.decompress over the members, each with its members already in memory:
                        uncompressed bytes per second of the decompression (first start to last end)

Every number needs the GPU: without one the tool stops."""
import argparse
import json
import multiprocessing as mp
import os
import shutil
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sam_fixtures as F  # noqa: E402

L = 150
NAME = 12                                  # "r%010d" + NUL
REC = 4 + 32 + NAME + L // 2 + L          # 273 bytes per BAM record


def reads(genome, first, n, seed):
    rng = np.random.default_rng(seed + first)
    pos = rng.integers(0, len(genome) - L, n)
    codes = genome[pos[:, None] + np.arange(L)[None, :]]            # 0..3 = A C G T
    qual = rng.integers(2, 42, (n, L), dtype=np.uint8)
    return codes, qual


def bam_records(codes, qual, first):
    n = len(codes)
    rec = np.zeros((n, REC), dtype=np.uint8)
    fixed = np.zeros(n, dtype=np.dtype([("bs", "<i4"), ("ref", "<i4"), ("pos", "<i4"), ("lname", "u1"), ("mapq", "u1"), ("bin", "<u2"),
                                         ("ncig", "<u2"), ("flag", "<u2"), ("lseq", "<i4"), ("nref", "<i4"), ("npos", "<i4"), ("tlen", "<i4")]))
    fixed["bs"] = REC - 4; fixed["ref"] = -1; fixed["pos"] = -1; fixed["lname"] = NAME; fixed["bin"] = 4680; fixed["flag"] = 4
    fixed["lseq"] = L; fixed["nref"] = -1; fixed["npos"] = -1
    rec[:, :36] = fixed.view(np.uint8).reshape(n, 36)
    names = np.frombuffer(b"".join(b"r%010d\0" % (first + i) for i in range(n)), dtype=np.uint8).reshape(n, NAME)
    rec[:, 36:36 + NAME] = names
    nib = np.array([1, 2, 4, 8], dtype=np.uint8)[codes]
    rec[:, 36 + NAME:36 + NAME + L // 2] = (nib[:, 0::2] << 4) | nib[:, 1::2]
    rec[:, 36 + NAME + L // 2:] = qual
    return rec


def fastq_records(codes, qual, first):
    n = len(codes)
    w = 12 + L + 3 + L + 1
    out = np.empty((n, w), dtype=np.uint8)
    out[:, :12] = np.frombuffer(b"".join(b"@r%09d\n" % (first + i) for i in range(n)), dtype=np.uint8).reshape(n, 12)
    out[:, 12:12 + L] = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
    out[:, 12 + L:15 + L] = np.frombuffer(b"\n+\n", dtype=np.uint8)
    out[:, 15 + L:15 + 2 * L] = qual + 33
    out[:, -1] = ord("\n")
    return out


def _member(piece):
    return F.bgzf_member(piece, "default")


_BARRIER = None


def _init(barrier):
    global _BARRIER
    _BARRIER = barrier


def _inflate(task):
    """One worker's share: its members read from the file first, then (all workers at once) only the decompression timed."""
    path, spans = task
    with open(path, "rb") as f:
        raws = [os.pread(f.fileno(), n, off) for off, n in spans]
    _BARRIER.wait(timeout=600)
    t0 = time.perf_counter()
    out = sum(len(zlib.decompress(m, -15)) for m in raws)
    return out, t0, time.perf_counter()


def build_inputs(wd, n_reads, genome_len, seed, pool):
    genome = np.random.default_rng(seed).integers(0, 4, genome_len, dtype=np.uint8)
    bam, fq = os.path.join(wd, "reads.bam"), os.path.join(wd, "reads.fq")
    with open(bam, "wb") as fb, open(fq, "wb") as ff:
        pending = F.bam_header((("chr1", genome_len),))
        step = 1 << 20
        for first in range(0, n_reads, step):
            n = min(step, n_reads - first)
            codes, qual = reads(genome, first, n, seed)
            ff.write(fastq_records(codes, qual, first).tobytes())
            data = pending + bam_records(codes, qual, first).tobytes()
            cut = len(data) - len(data) % 65280 if first + n < n_reads else len(data)
            fb.write(b"".join(pool.map(_member, [data[i:i + 65280] for i in range(0, cut, 65280)])))
            pending = data[cut:]
        fb.write(F.EOF_MARKER)
    return bam, fq


def device_inflate_and_decode(bam, chunk):
    from jellyfish_amd import capi
    p = capi.Parser(21, 0)
    z = open(bam, "rb").read()
    blocks, used = capi.bgzf_scan(z)
    starts = [b.c_off - 18 for b in blocks] + [used]
    per = max(1, chunk // 30000)
    inf_ms = dec_ms = 0.0
    out_bytes = dec_bytes = records = 0
    skip_hdr = None
    for ci, i in enumerate(range(0, len(blocks), per)):
        a, b = starts[i], starts[min(i + per, len(blocks))]
        n = p.inflate(z[a:b], which=ci % 2)
        inf_ms += p.last_ms()
        out_bytes += sum(bl.isize for bl in blocks[i:i + per])
        skip = 0
        if skip_hdr is None:
            skip_hdr = len(F.bam_header((("chr1", 1),)))       # one reference: the header length does not depend on its length
            skip = skip_hdr
        _, _, recs, _ = p.bam_decode(skip, 1)
        dec_ms += p.last_ms()
        dec_bytes += n - skip
        records += recs
    p.close()
    return out_bytes / inf_ms / 1e6, dec_bytes / dec_ms / 1e6, records


def count_rate(cli, wd, args, n_reads, size):
    t = os.path.join(wd, "timing")
    subprocess.check_call([cli, "count", "-m", "21", "-C", "-s", size, "-o", os.path.join(wd, "o.jf"), "--timing", t] + args)
    counting = float(open(t).read().split()[3])
    return n_reads * (L - 21 + 1) / counting / 1e9, counting


def host_zlib(bam, procs, pool):
    """16 (procs) workers inflating every member of the file, each its share read into memory beforehand: uncompressed
    bytes over the span from the first worker's start to the last one's end (CLOCK_MONOTONIC, shared by the processes)."""
    from jellyfish_amd import capi
    z = open(bam, "rb").read()
    blocks, _ = capi.bgzf_scan(z)
    del z
    spans = [(b.c_off, b.c_len) for b in blocks]
    res = pool.map(_inflate, [(bam, spans[i::procs]) for i in range(procs)], chunksize=1)
    total = sum(r[0] for r in res)
    return total / (max(r[2] for r in res) - min(r[1] for r in res)) / 1e9


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gbp", type=float, default=2.0)
    ap.add_argument("--genome", type=int, default=20_000_000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--workdir", default=None)
    ap.add_argument("--keep", action="store_true")
    ap.add_argument("--procs", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cli = os.environ.get("JFGPU_CLI") or os.path.join(ROOT, "bin", "jellyfish-amd")
    wd = a.workdir or tempfile.mkdtemp(prefix="sam_feed_bench_")
    os.makedirs(wd, exist_ok=True)
    n_reads = int(a.gbp * 1e9 / L)
    res = {"gbp": a.gbp, "reads": n_reads, "read_len": L}
    try:
        ctx = mp.get_context("fork")
        with ctx.Pool(a.procs, initializer=_init, initargs=(ctx.Barrier(a.procs),)) as pool:   # (forked before this process touches the GPU)
            t0 = time.perf_counter()
            bam, fq = build_inputs(wd, n_reads, a.genome, a.seed, pool)
            res["build_s"] = round(time.perf_counter() - t0, 1)
            res["bam_bytes"], res["fastq_bytes"] = os.path.getsize(bam), os.path.getsize(fq)
            res["host_zlib_GBps"] = round(host_zlib(bam, a.procs, pool), 3)
        from jellyfish_amd import capi
        if capi.device_count() == 0:
            sys.exit("sam_feed_bench: no GPU")
        inf, dec, recs = device_inflate_and_decode(bam, 64 << 20)
        assert recs == n_reads, (recs, n_reads)
        res["inflate_GBps"], res["decode_GBps"] = round(inf, 3), round(dec, 3)
        subprocess.check_call(["cat", bam], stdout=subprocess.DEVNULL)          # both inputs in the page cache alike
        subprocess.check_call(["cat", fq], stdout=subprocess.DEVNULL)
        r, s = count_rate(cli, wd, ["--sam", bam], n_reads, "64M")
        res["sam_count_Gkmers_s"], res["sam_counting_s"] = round(r, 3), round(s, 3)
        r, s = count_rate(cli, wd, [fq], n_reads, "64M")
        res["fastq_count_Gkmers_s"], res["fastq_counting_s"] = round(r, 3), round(s, 3)
        res["sam_over_fastq_time"] = round(res["sam_counting_s"] / res["fastq_counting_s"], 2)
    finally:
        if not a.keep:
            shutil.rmtree(wd, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
