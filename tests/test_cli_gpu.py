"""Drop-in check of the whole `count` verb on the GPU (-m gpu): jellyfish-amd count writes a
binary/sorted (or text/sorted) file that (a) decodes to the reference's golden dump and (b) is
read, order-checked and queried by the REFERENCE's own readers (oracle/_ref/ref_jf travels to the
GPU box prebuilt; /root/reference itself is never touched at run time)."""
import json
import os
import subprocess

import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MANIFEST = json.load(open(os.path.join(GOLD, "manifest.json")))
CLI = os.environ.get("JFGPU_CLI") or os.path.join(ROOT, "bin", "jellyfish-amd")    # JFGPU_CLI: tests/host/build_emu.sh debugging build


@pytest.fixture(scope="module")
def cli(gpu):
    if not os.environ.get("JFGPU_CLI"):
        subprocess.check_call(["make", "-s", "cli"], cwd=ROOT)
    return CLI


@pytest.mark.parametrize("case", MANIFEST["cases"], ids=lambda c: c["name"])
def test_count_file_matches_reference_golden(cli, case, tmp_path):
    name, k = case["name"], case["k"]
    out = str(tmp_path / "out.jf")
    cmd = [cli, "count", "-m", str(k), "-s", case["size"], "-t", "4", "-o", out, "--timing", str(tmp_path / "timing")]
    if case["canonical"]:
        cmd.append("-C")
    subprocess.check_call(cmd + [os.path.join(GOLD, case["input"])])
    golden = open(os.path.join(GOLD, name + ".dump")).read().splitlines()
    mine = subprocess.check_output([cli, "dump", "-c", out]).decode().splitlines()
    assert sorted(mine) == golden
    assert subprocess.check_output([cli, "histo", out]).decode() == open(os.path.join(GOLD, name + ".histo")).read()
    assert subprocess.check_output([cli, "stats", out]).decode() == open(os.path.join(GOLD, name + ".stats")).read()
    t = open(tmp_path / "timing").read().split()
    assert t[0::2] == ["Init", "Counting", "Writing"]                      # count_main.cc:377-382 labels
    if O.have_ref():
        # the reference's binary_reader / binary_query consume our file unchanged
        ref = subprocess.check_output([O.REF_JF, "dump", "-c", out]).decode().splitlines()
        assert ref == mine
        assert subprocess.check_output([O.REF_JF, "dump", "--check-order", out]).decode().startswith("ORDER OK %d" % len(golden))
        assert subprocess.check_output([O.REF_JF, "histo", out]).decode() == open(os.path.join(GOLD, name + ".histo")).read()
        assert subprocess.check_output([O.REF_JF, "stats", out]).decode() == open(os.path.join(GOLD, name + ".stats")).read()
        sample = golden[:: max(1, len(golden) // 100)]
        q = subprocess.check_output([O.REF_JF, "query", out] + [l.split()[0] for l in sample]).decode().splitlines()
        assert q == sample


@pytest.mark.parametrize("name", ["reads150_k21C", "reads150_k63C", "reads150_k32"])
def test_count_digest_equals_the_reference_tables_digest(cli, name, tmp_path):
    """The at-scale parity instrument (tools/at_scale_parity.sh) on a small case: `jellyfish-amd count --digest`
    (jfgpu_digest over the device table) == `ref_jf count --digest` (the reference's in-memory table) == the digest
    of the written file."""
    from jellyfish_amd import capi
    case = next(c for c in MANIFEST["cases"] if c["name"] == name)
    inp, k = os.path.join(GOLD, case["input"]), case["k"]
    can = ["-C"] if case["canonical"] else []
    out, dg = str(tmp_path / "o.jf"), str(tmp_path / "d.txt")
    subprocess.check_call([cli, "count", "-m", str(k), "-s", case["size"], "-o", out, "--digest", dg] + can + [inp])
    mine = open(dg).read()
    assert subprocess.check_output([cli, "digest", out]).decode() == mine
    keys, cnt = O.count(O.parse_file(open(inp, "rb").read()), k, case["canonical"])
    assert tuple(int(l.split()[1]) for l in mine.splitlines()) == capi.digest_of(keys, cnt)
    if O.have_ref():
        subprocess.check_call([O.REF_JF, "count", "-m", str(k), "-s", case["size"], "-t", "2", "--no-write", "--digest", str(tmp_path / "r.txt")] + can + [inp])
        assert open(tmp_path / "r.txt").read() == mine
        assert subprocess.check_output([O.REF_JF, "digest", out]).decode() == mine


def test_config1_recorded_md5s_through_the_engine(cli, tmp_path):
    """BASELINE configs[0] on the engine: the reference generator's 10 MB file (md5 recorded by the
    survey) counted with `-m 21 -C -s 16M`, and `histo` of the result has the recorded md5 `08762de4...`; the file the
    engine wrote is read by the reference's own `histo` with the same result."""
    import hashlib
    if not os.access(O.REF_GEN, os.X_OK):
        pytest.skip("oracle/_ref not built")
    d = str(tmp_path)
    subprocess.check_call([O.REF_GEN, "-s", "42", "-r", "150", "-o", "reads150", "10000000"], cwd=d)
    assert hashlib.md5(open(os.path.join(d, "reads150.fa"), "rb").read()).hexdigest() == "e539471302c480c328f8908dad38ff67"
    for mode in ("direct", "partitioned"):
        subprocess.check_call([cli, "count", "-m", "21", "-C", "-s", "16M", "-t", "1", "-o", "c1.jf", "reads150.fa"], cwd=d, env=dict(os.environ, JFGPU_MODE=mode))
        histo = subprocess.check_output([cli, "histo", "c1.jf"], cwd=d)
        assert histo == b"1 8666626\n2 17\n" and hashlib.md5(histo).hexdigest() == "08762de4d79a53b64b58517437425c3e", mode
    if O.have_ref():
        assert subprocess.check_output([O.REF_JF, "histo", "c1.jf"], cwd=d) == histo


@pytest.fixture(scope="module")
def half_gbp_reads(tmp_path_factory):
    """0.5 Gbp of 150 bp reads from the REFERENCE's generator (generate_sequence -s 42 -r 150: one-line records of 150
    bases) in /dev/shm: the input of the at-scale parity tests below."""
    if not O.have_ref() or not os.access(O.REF_GEN, os.X_OK):
        pytest.skip("oracle/_ref not built")
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    d = tmp_path_factory.mktemp("halfgbp") if base is None else __import__("tempfile").mkdtemp(prefix="jf_halfgbp_", dir=base)
    subprocess.check_call([O.REF_GEN, "-s", "42", "-r", "150", "-o", "reads", "500000000"], cwd=str(d))
    yield os.path.join(str(d), "reads.fa")
    __import__("shutil").rmtree(str(d), ignore_errors=True)


def timing_counters(path):
    """`count --timing` with JFGPU_TIMING_DETAIL=1: the reference's three lines, then the engine's counters (which kernels ran)."""
    return {l.split()[0]: l.split()[1] for l in open(path).read().splitlines() if len(l.split()) >= 2}


@pytest.mark.parametrize("cfg,k,size", [("C2", 21, "2G"), ("C2", 21, "8G"), ("C2", 21, "16G"), ("C5", 63, "512M"), ("C3", 31, "512M")])
def test_half_gbp_reference_file_digest_equals_the_reference(cli, half_gbp_reads, tmp_path, cfg, k, size):
    """Parity at a size where every stage of the partitioned path works at realistic fill (P1 buckets, P2 regions, LDS
    tiles: 433 M k-mers at k = 21 into 2^31 slots; 16-byte items at k = 63; the Bloom pass + filtered count at k = 31) on
    a file written by the reference's own generator: the content digest of the whole table from `jellyfish-amd count
    --digest` must equal `ref_jf count --digest` (the reference's in-memory table walked by its own iterators), counted
    here on the host cores.  For C3 both sides first write their Bloom counter (`bc`), which must be byte-identical.
    `-s 8G` and `-s 16G` are the HEADLINE geometries (4-byte items and slots, 512 / 1024 destinations per P1 bucket): there --
    and only there -- the flush takes p1_ring_kernel, p2_ring_roles_kernel<.., 1 / 2> and the pair tile kernel, the kernels
    bench.py times; the content digest depends neither on the table's size nor on its matrix, so the reference counts the
    same file with `-s 2G`, and the engine's counters (count --timing) say the ring kernels ran (round-4 review, weak #1)."""
    nproc = str(min(os.cpu_count() or 1, 64))
    env = dict(os.environ, JFGPU_QUIET="1", JFGPU_MODE="partitioned", JFGPU_TIMING_DETAIL="1")
    mine, ref = str(tmp_path / "mine.digest"), str(tmp_path / "ref.digest")
    ref_size = "2G" if cfg == "C2" else size
    extra_m, extra_r = [], []
    if cfg == "C3":
        bm, br = str(tmp_path / "mine.bc"), str(tmp_path / "ref.bc")
        subprocess.check_call([cli, "bc", "-m", str(k), "-C", "-s", "500M", "-o", bm, half_gbp_reads], env=env)
        subprocess.check_call([O.REF_JF, "bc", "-m", str(k), "-C", "-s", "500M", "-t", nproc, "-o", br, half_gbp_reads])
        offs = [9 + int(open(f, "rb").read(9)) for f in (bm, br)]          # (the headers carry command lines and times: bodies only)
        assert subprocess.call(["cmp", "-s", "-i", "%d:%d" % tuple(offs), bm, br]) == 0, "Bloom counter bodies differ"
        assert os.path.getsize(bm) - offs[0] == os.path.getsize(br) - offs[1] > 1_000_000_000
        extra_m, extra_r = ["--bc", bm], ["--bc", br]
    subprocess.check_call([cli, "count", "-m", str(k), "-C", "-s", size, "--no-write", "--digest", mine, "--timing", str(tmp_path / "timing")] + extra_m + [half_gbp_reads], env=env)
    subprocess.check_call([O.REF_JF, "count", "-m", str(k), "-C", "-s", ref_size, "-t", nproc, "--no-write", "--digest", ref] + extra_r + [half_gbp_reads])
    assert open(mine).read() == open(ref).read()
    assert int(open(mine).read().split()[1]) > (1000 if cfg == "C3" else 100_000_000)
    tm = timing_counters(tmp_path / "timing")
    if size in ("8G", "16G"):
        # (the file's short last chunk is an exact two-pass P1 batch -- P1Other 1 -- which the loader / storer kernel takes item by item)
        assert int(tm["P1Ring"]) >= 1 and int(tm["P1Other"]) <= 1 and int(tm["P2Roles"]) >= 1 and int(tm["P2Sort"]) == 0 and int(tm["P2Exact"]) == 0, tm
        assert int(tm["DirectInserts"]) < 1_000_000, tm


@pytest.fixture(scope="module")
def half_gbp_genome_reads(tmp_path_factory):
    """0.5 Gbp of 150 bp reads sampled from a 5 Mbp random genome with 1 % substitutions (~100 x coverage: BASELINE.md's
    secondary distribution, what sequencing data looks like), written by the engine's device generator to a FASTA file in
    /dev/shm the way bench.py writes its end-to-end input."""
    if not O.have_ref():
        pytest.skip("oracle/_ref not built")
    import numpy as np
    from jellyfish_amd import capi
    base = "/dev/shm" if os.path.isdir("/dev/shm") else None
    d = str(tmp_path_factory.mktemp("halfgbpG")) if base is None else __import__("tempfile").mkdtemp(prefix="jf_halfgbpG_", dir=base)
    L, n_reads, path = 150, 3_333_333, os.path.join(d, "readsG.fa")
    with capi.Table(21, 1 << 20) as t, open(path, "wb") as f:
        step = 1 << 20
        dbuf = t.malloc(step * (L + 1) + 16)
        hdr = np.frombuffer(b">r\n", dtype=np.uint8)
        for r0 in range(0, n_reads, step):
            n = min(step, n_reads - r0)
            t.gen_genome_reads_dev(dbuf, r0, n, L, 5_000_000, 0.01, 4242)
            t.wait()
            body = t.d2h(dbuf, n * (L + 1)).reshape(n, L + 1)
            body[:, L] = ord("\n")
            np.concatenate([np.tile(hdr, (n, 1)), body], axis=1).tofile(f)
        t.free(dbuf)
    yield path
    __import__("shutil").rmtree(d, ignore_errors=True)


@pytest.mark.parametrize("cfg,k,size", [("C2", 21, "2G"), ("C2", 21, "16G"), ("C3", 31, "512M")])
def test_half_gbp_high_coverage_file_digest_equals_the_reference(cli, half_gbp_genome_reads, tmp_path, cfg, k, size):
    """The same check on high-coverage input (round-3 review, item 1b): every true k-mer ~100 times, so the tile stage's
    merge, its queue and -- chosen by the flush's own sample -- its HEAVY instantiation carry the work, and in C3 geometry
    most k-mers pass the Bloom filter (ten cell reads each).  Content digest of the whole table against `ref_jf count
    --digest`; the Bloom counter bodies byte-identical."""
    nproc = str(min(os.cpu_count() or 1, 64))
    env = dict(os.environ, JFGPU_QUIET="1", JFGPU_MODE="partitioned")
    mine, ref = str(tmp_path / "mine.digest"), str(tmp_path / "ref.digest")
    ref_size = "2G" if cfg == "C2" else size      # (the digest does not depend on the size: -s 16G is the headline geometry, ring kernels)
    extra_m, extra_r = [], []
    if cfg == "C3":
        bm, br = str(tmp_path / "mine.bc"), str(tmp_path / "ref.bc")
        subprocess.check_call([cli, "bc", "-m", str(k), "-C", "-s", "500M", "-o", bm, half_gbp_genome_reads], env=env)
        subprocess.check_call([O.REF_JF, "bc", "-m", str(k), "-C", "-s", "500M", "-t", nproc, "-o", br, half_gbp_genome_reads])
        offs = [9 + int(open(f, "rb").read(9)) for f in (bm, br)]
        assert subprocess.call(["cmp", "-s", "-i", "%d:%d" % tuple(offs), bm, br]) == 0, "Bloom counter bodies differ"
        extra_m, extra_r = ["--bc", bm], ["--bc", br]
    subprocess.run([cli, "count", "-m", str(k), "-C", "-s", size, "--no-write", "--digest", mine, "--timing", str(tmp_path / "timing")] + extra_m + [half_gbp_genome_reads],
                   env=dict(env, JFGPU_TIMING_DETAIL="1"), check=True)
    subprocess.check_call([O.REF_JF, "count", "-m", str(k), "-C", "-s", ref_size, "-t", nproc, "--no-write", "--digest", ref] + extra_r + [half_gbp_genome_reads])
    assert open(mine).read() == open(ref).read()
    records, total = (int(x.split()[1]) for x in open(mine).read().splitlines()[:2])
    assert total > 3 * records > 3_000_000      # high coverage: the true k-mers ~100 times each beside the error k-mers (one third of the occurrences)
    if cfg == "C2":      # the flush chose the HEAVY tile kernel from its own sample (count --timing reports the counters)
        tm = timing_counters(tmp_path / "timing")
        assert int(tm.get("FlushesHeavy", 0)) >= 1, tm
        if size == "16G":
            assert int(tm["P1Ring"]) >= 1 and int(tm["P2Roles"]) >= 1 and int(tm["P2Sort"]) == 0 and int(tm["P2Exact"]) == 0, tm


def test_count_text_format_and_bounds(cli, tmp_path):
    case = next(c for c in MANIFEST["cases"] if c["name"] == "reads150_k5C")
    inp = os.path.join(GOLD, case["input"])
    golden = [l.split() for l in open(os.path.join(GOLD, "reads150_k5C.dump"))]
    txt = str(tmp_path / "t.jf")
    subprocess.check_call([cli, "count", "-m", "5", "-C", "-s", "4k", "--text", "-o", txt, inp])
    got = sorted(subprocess.check_output([cli, "dump", "-c", txt]).decode().splitlines())
    assert got == [" ".join(g) for g in golden]
    lo, hi = 10, 14
    lu = str(tmp_path / "lu.jf")
    subprocess.check_call([cli, "count", "-m", "5", "-C", "-s", "4k", "-L", str(lo), "-U", str(hi), "-o", lu, inp])
    got = sorted(subprocess.check_output([cli, "dump", "-c", lu]).decode().splitlines())
    assert got == [" ".join(g) for g in golden if lo <= int(g[1]) <= hi]
    if O.have_ref():
        assert sorted(subprocess.check_output([O.REF_JF, "dump", "-c", txt]).decode().splitlines()) == [" ".join(g) for g in golden]


def test_count_multiple_files_and_hash_full(cli, tmp_path):
    fa = os.path.join(GOLD, "reads150_s42.fa")
    fq = os.path.join(GOLD, "reads_fq_s1473540700.fq")
    out = str(tmp_path / "two.jf")
    subprocess.check_call([cli, "count", "-m", "21", "-C", "-s", "64k", "-o", out, fa, fq])
    exp = {}
    for n in ("reads150_k21C", "fastq_k21C"):
        for l in open(os.path.join(GOLD, n + ".dump")):
            a, c = l.split()
            exp[a] = exp.get(a, 0) + int(c)
    got = dict((a, int(c)) for a, c in (l.split() for l in subprocess.check_output([cli, "dump", "-c", out]).decode().splitlines()))
    assert got == exp
    # -s is only a hint (doc/Readme.md:67-72): a tiny table doubles itself and gives the same counts ...
    small = str(tmp_path / "small.jf")
    subprocess.check_call([cli, "count", "-m", "21", "-C", "-s", "1k", "-o", small, fa, fq])
    assert dict((a, int(c)) for a, c in (l.split() for l in subprocess.check_output([cli, "dump", "-c", small]).decode().splitlines())) == exp
    if O.have_ref():
        assert subprocess.check_output([O.REF_JF, "dump", "--check-order", small]).decode().startswith("ORDER OK %d" % len(exp))
    # ... and with doubling switched off (--disk, count_main.cc:276-277) it is written out in sorted runs that are merged at the end
    disk = str(tmp_path / "disk.jf")
    subprocess.run([cli, "count", "-m", "21", "-C", "-s", "1k", "--disk", "-o", disk, fa, fq], check=True, timeout=120)
    assert dict((a, int(c)) for a, c in (l.split() for l in subprocess.check_output([cli, "dump", "-c", disk]).decode().splitlines())) == exp
    # nowhere to spill to (--no-write): "Hash full" (hash_counter.hpp:194-195), exit code 1
    r = subprocess.run([cli, "count", "-m", "21", "-C", "-s", "1k", "--disk", "--no-write", "-o", str(tmp_path / "full.jf"), fa], capture_output=True, timeout=120)
    assert r.returncode == 1 and b"Hash full" in r.stderr
    r = subprocess.run([cli, "count", "-m", "21", "-s", "64k", "-o", str(tmp_path / "bad.jf"), os.path.join(GOLD, "manifest.json")],
                       capture_output=True)
    assert r.returncode == 1 and b"Unsupported format" in r.stderr


def _wrapped_fastq(n):
    import random
    rng = random.Random(5)
    out = []
    for r in range(n):
        seq = "".join(rng.choice("ACGT") for _ in range(120))
        out.append("@r%d\n%s\n%s\n+\n%s\n%s\n" % (r, seq[:70], seq[70:], "I" * 70, "I" * 50))
    return "".join(out).encode()


def test_device_parse_equals_host_parse(cli, tmp_path):
    """The default feed (device parser) and --host-parse write byte-identical files, for FASTA, strict
    FASTQ, and wrapped FASTQ (which the device parser hands back to the host reader)."""
    inputs = {"fa": os.path.join(GOLD, "edge_cases.fa"),
              "fq": os.path.join(GOLD, [f for f in os.listdir(GOLD) if f.endswith(".fq")][0])}
    w = tmp_path / "wrapped.fq"
    w.write_bytes(_wrapped_fastq(500))
    inputs["wrapped"] = str(w)
    for tag, inp in inputs.items():
        a, b = str(tmp_path / (tag + ".dev.jf")), str(tmp_path / (tag + ".host.jf"))
        base = [cli, "count", "-m", "21", "-C", "-s", "1M"]
        for pinned in ("1", "0"):
            env = dict(os.environ, JFGPU_TIMING_DETAIL="1", JFGPU_FEED_PINNED=pinned, JFGPU_PARSE_CHUNK="16384")
            subprocess.check_call(base + ["-o", a, "--timing", str(tmp_path / "tm"), inp], env=env)
            if pinned == "1":
                first = subprocess.check_output([cli, "dump", "-c", a])
        assert first == subprocess.check_output([cli, "dump", "-c", a])
        subprocess.check_call(base + ["-o", b, "--host-parse", inp])
        da = subprocess.check_output([cli, "dump", "-c", a])
        assert da == subprocess.check_output([cli, "dump", "-c", b]) and len(da) > 0
        tm = dict(l.split() for l in open(tmp_path / "tm"))
        assert (int(tm["HostParsedBytes"]) > 0) == (tag == "wrapped")
    bad = tmp_path / "bad.fq"
    bad.write_bytes(b"@r\nACGTACGTACGTACGTACGTACGT\n+\nIIII\n")
    r = subprocess.run([cli, "count", "-m", "21", "-s", "1M", "-o", str(tmp_path / "x.jf"), str(bad)], capture_output=True)
    assert r.returncode != 0 and b"Invalid fastq sequence" in r.stderr      # mer_overlap_sequence_parser.hpp:308


def test_many_chunks_equal_one(cli, tmp_path):
    """Small device chunks (JFGPU_PARSE_CHUNK) cut a multi-line FASTA and a FASTQ in many places."""
    import random
    rng = random.Random(11)
    fa = tmp_path / "multi.fa"
    with open(fa, "wb") as f:
        for r in range(300):
            seq = "".join(rng.choice("ACGT") for _ in range(rng.choice([30, 500, 3000])))
            f.write((">s%d\n" % r).encode())
            for i in range(0, len(seq), 60):
                f.write(seq[i:i + 60].encode() + b"\n")
    fq = os.path.join(GOLD, [f for f in os.listdir(GOLD) if f.endswith(".fq")][0])
    for inp in (str(fa), fq):
        outs = []
        for chunk, pinned in (("65536", "0"), ("1073741824", "0"), ("65536", "1"), ("20000", "1")):
            o = str(tmp_path / ("c" + chunk + pinned + ".jf"))
            # pinned = 1: the large-file feed (parallel pread into two pinned buffers, tails carried over)
            subprocess.check_call([cli, "count", "-m", "25", "-C", "-s", "2M", "-o", o, inp],
                                  env=dict(os.environ, JFGPU_PARSE_CHUNK=chunk, JFGPU_FEED_PINNED=pinned))
            outs.append(subprocess.check_output([cli, "dump", "-c", o]))
        assert all(x == outs[0] for x in outs) and len(outs[0]) > 0


@pytest.mark.parametrize("k,canonical", [(21, True), (12, False)])
def test_count_if_equals_reference(cli, tmp_path, k, canonical):
    """`count --if`: prime the table with the k-mers of the filter file, then only update
    (count_main.cc:160-181,289-295).  k-mers of the filter absent from the reads stay with count 0 and are
    written, counted by stats and shown by histo -- exactly like the reference binary on the same files."""
    if not O.have_ref():
        pytest.skip("oracle/_ref not built")
    import random
    rng = random.Random(k)
    genome = "".join(rng.choice("ACGT") for _ in range(20000))
    other = "".join(rng.choice("ACGT") for _ in range(3000))
    filt = tmp_path / "filter.fa"
    filt.write_text(">wanted\n%s\n>absent\n%s\n" % (genome[2000:7000], other))
    reads = tmp_path / "reads.fa"
    with open(reads, "w") as f:
        for r in range(3000):
            p = rng.randrange(0, len(genome) - 150)
            f.write(">r%d\n%s\n" % (r, genome[p:p + 150]))
    flags = ["-m", str(k), "-s", "200k"] + (["-C"] if canonical else [])
    mine, ref = str(tmp_path / "mine.jf"), str(tmp_path / "ref.jf")
    subprocess.check_call([cli, "count"] + flags + ["--if", str(filt), "-o", mine, str(reads)])
    subprocess.check_call([O.REF_JF, "count"] + flags + ["--if", str(filt), "-o", ref, str(reads)])
    a = sorted(subprocess.check_output([cli, "dump", "-c", mine]).decode().splitlines())
    b = sorted(subprocess.check_output([O.REF_JF, "dump", "-c", ref]).decode().splitlines())
    assert a == b and any(l.endswith(" 0") for l in a) and any(not l.endswith(" 0") for l in a)
    for verb in ("stats", "histo"):
        assert subprocess.check_output([cli, verb, mine]) == subprocess.check_output([O.REF_JF, verb, ref])
    # the reference's own readers on our file
    assert sorted(subprocess.check_output([O.REF_JF, "dump", "-c", mine]).decode().splitlines()) == b
    assert subprocess.check_output([O.REF_JF, "dump", "--check-order", mine]).decode().startswith("ORDER OK %d" % len(b))


def test_generator_commands(cli, tmp_path):
    """-g: input produced by shell commands (the reference's way to read compressed files,
    lib/generator_manager.cc): same result as counting the files directly."""
    import gzip
    inp = os.path.join(GOLD, "reads150_s42.fa")
    gz = tmp_path / "reads.fa.gz"
    with open(inp, "rb") as f, gzip.open(gz, "wb") as g:
        g.write(f.read())
    gen = tmp_path / "generators"
    gen.write_text("gzip -dc %s\n\ncat %s\n" % (gz, os.path.join(GOLD, "edge_cases.fa")))
    a, b = str(tmp_path / "gen.jf"), str(tmp_path / "plain.jf")
    subprocess.check_call([cli, "count", "-m", "21", "-C", "-s", "1M", "-o", a, "-g", str(gen)])
    subprocess.check_call([cli, "count", "-m", "21", "-C", "-s", "1M", "-o", b, inp, os.path.join(GOLD, "edge_cases.fa")])
    da = subprocess.check_output([cli, "dump", "-c", a])
    assert da == subprocess.check_output([cli, "dump", "-c", b]) and len(da) > 0
    bad = tmp_path / "badgen"
    bad.write_text("exit 3\n")
    r = subprocess.run([cli, "count", "-m", "21", "-s", "1M", "-o", a, "-g", str(bad)], capture_output=True)
    assert r.returncode != 0 and b"Generator command failed" in r.stderr


def _body(path):
    d = open(path, "rb").read()
    return d[9 + int(d[:9]):]


@pytest.mark.parametrize("name", ["reads150_k21C", "edge_k8C"])
def test_file_body_is_byte_identical_to_the_reference(cli, tmp_path, name):
    """With the default (reference-identical) hash matrix the records come out in the reference's own order: the
    body of our binary/sorted file equals, byte for byte, the body of the file the reference wrote for the same
    command line (tests/golden/*.ref.jf, produced by oracle/_ref)."""
    case = next(c for c in MANIFEST["cases"] if c["name"] == name)
    out = str(tmp_path / "out.jf")
    cmd = [cli, "count", "-m", str(case["k"]), "-s", case["size"], "-o", out, "--matrix", "reference"] + (["-C"] if case["canonical"] else [])
    subprocess.check_call(cmd + [os.path.join(GOLD, case["input"])])       # (the family is named: a suite run under JFGPU_MATRIX=xs keeps this test meaningful)
    ref = os.path.join(GOLD, name + ".ref.jf")
    assert _body(out) == _body(ref)
    import json as _json
    h_mine = _json.loads(open(out, "rb").read()[9:9 + int(open(out, "rb").read()[:9])].decode().rstrip("\0 \n"))
    h_ref = _json.loads(open(ref, "rb").read()[9:9 + int(open(ref, "rb").read()[:9])].decode().rstrip("\0 \n"))
    for key in ("matrix1", "size", "key_len", "counter_len", "format", "canonical"):
        assert h_mine[key] == h_ref[key], key


@pytest.mark.parametrize("k,flags,size", [(21, ["-C"], "4M"), (21, [], "4M"), (21, ["-C"], "2k"), (31, ["-C"], "4M"), (32, [], "1M"),
                                          (40, ["-C"], "4M"), (63, ["-C"], "2k"), (10, ["-C"], "4M"), (17, ["-C"], "16M")])
def test_xorshift_matrix_files_are_read_by_the_reference(cli, tmp_path, k, flags, size):
    """`count --matrix xs` (include/jfgpu.h: JFGPU_MATRIX_XORSHIFT; kmer_core.hpp: xs_hash): the hash matrix is any matrix with
    an invertible low block as far as the file format goes -- readers take it from the header (include/jellyfish/file_header.hpp:35-64,
    rectangular_binary_matrix.hpp:155-164).  The file written under the xor-shift family holds the counts of the file written
    under the reference's own matrix; the reference's reader accepts its record order (--check-order walks the (pos, key)
    order under the header's matrix), dumps the same records, answers queries from it (binary search by position) and
    draws the same histogram.  -s 2k: the table doubles many times, every doubling under the next member of the family;
    k = 10 and k = 17 -s 16M: the identity cases (table bits >= key bits) and the 32-bit-position members."""
    import random
    rng = random.Random(1000 + k)
    fa = tmp_path / "reads.fa"
    genome = "".join(rng.choice("ACGT") for _ in range(30000))
    with open(fa, "w") as f:
        for r in range(2500):
            a = rng.randrange(len(genome) - 150)
            read = list(genome[a:a + 150])
            if r % 97 == 0:
                read[rng.randrange(150)] = "N"
            if r % 211 == 0:
                read[40:110] = "A" * 70                                        # a homopolymer run: one k-mer many times in a row
            f.write(">r%d\n%s\n" % (r, "".join(read)))
    xs, rf = str(tmp_path / "xs.jf"), str(tmp_path / "ref.jf")
    subprocess.check_call([cli, "count", "-m", str(k), "-s", size, "-o", xs, "--matrix", "xs"] + flags + [str(fa)])
    subprocess.check_call([cli, "count", "-m", str(k), "-s", size, "-o", rf, "--matrix", "reference"] + flags + [str(fa)])
    mine_xs = subprocess.check_output([cli, "dump", "-c", xs]).splitlines()
    mine_rf = subprocess.check_output([cli, "dump", "-c", rf]).splitlines()
    assert sorted(mine_xs) == sorted(mine_rf) and len(mine_xs) > 1000
    info = subprocess.check_output([cli, "info", xs]).decode()
    if 2 * k > {"4M": 22, "2k": 11, "1M": 20, "16M": 24}[size] and k > 10:
        assert mine_xs != mine_rf                                              # (another matrix, another order)
    if not O.have_ref():
        pytest.skip("oracle/_ref not built")
    assert subprocess.check_output([O.REF_JF, "dump", "--check-order", xs]).decode().startswith("ORDER OK"), info
    assert subprocess.check_output([O.REF_JF, "dump", "-c", xs]).splitlines() == mine_xs
    assert subprocess.check_output([O.REF_JF, "histo", xs]) == subprocess.check_output([O.REF_JF, "histo", rf])
    picks = [l.split()[0].decode() for l in mine_xs[:: max(1, len(mine_xs) // 7)]][:7] + ["A" * k]
    ans = subprocess.check_output([O.REF_JF, "query", xs] + picks).decode().split()
    want = dict(l.decode().split() for l in mine_xs)
    assert [ans[2 * i + 1] for i in range(len(picks))] == [want.get(q, "0") for q in picks]


@pytest.mark.parametrize("k,flags,matrix", [(21, ["-C"], "reference"), (21, ["-C"], "xs"), (40, ["-C"], "xs"), (12, [], "reference")])
def test_query_sequence_is_answered_from_the_device(cli, tmp_path, k, flags, matrix):
    """`query -s file` (sub_commands/query_main.cc:44-51: every k-mer of the sequence files, in order, with its count): the
    records of the database go back into a device table under the header's matrix (jfgpu_add_key_vals) and the k-mers are
    looked up in batches (jfgpu_lookup) -- the output is, byte for byte, the host path's (binary search in the mapped
    file, JFGPU_QUERY_HOST=1), and its counts are the dump's."""
    import random
    rng = random.Random(7 * k)
    genome = "".join(rng.choice("ACGT") for _ in range(20000))
    fa = tmp_path / "reads.fa"
    with open(fa, "w") as f:
        for r in range(1500):
            a = rng.randrange(len(genome) - 120)
            f.write(">r%d\n%s\n" % (r, genome[a:a + 120]))
    db = str(tmp_path / "db.jf")
    subprocess.check_call([cli, "count", "-m", str(k), "-s", "1M", "-o", db, "--matrix", matrix] + flags + [str(fa)])
    q = tmp_path / "q.fa"
    with open(q, "w") as f:
        f.write(">known\n%s\n>with_N\n%sN%s\n>novel\n%s\n" % (genome[100:700], genome[3000:3100], genome[3100:3200],
                                                              "".join(rng.choice("ACGT") for _ in range(300))))
    dev = subprocess.check_output([cli, "query", db, "-s", str(q)])
    host = subprocess.check_output([cli, "query", db, "-s", str(q)], env=dict(os.environ, JFGPU_QUERY_HOST="1"))
    assert dev == host
    lines = dev.decode().splitlines()
    assert len(lines) == (600 - k + 1) + 2 * (100 - k + 1) + (300 - k + 1)
    want = dict(l.split() for l in subprocess.check_output([cli, "dump", "-c", db]).decode().splitlines())
    assert all(want.get(l.split()[0], "0") == l.split()[1] for l in lines)
    assert sum(1 for l in lines if l.split()[1] != "0") >= (600 - k + 1)


@pytest.mark.parametrize("case", MANIFEST["bloom"], ids=lambda c: c["name"])
def test_bc_file_is_byte_identical_to_the_reference(cli, tmp_path, case):
    """`jellyfish-amd bc` draws the reference's default hash pair, so the whole bloomcounter body is the
    reference's."""
    out = str(tmp_path / "out.bc")
    cmd = [cli, "bc", "-m", str(case["k"]), "-s", str(case["n"]), "-f", str(case["fpr"]), "-o", out] + (["-C"] if case["canonical"] else [])
    subprocess.check_call(cmd + [os.path.join(GOLD, case["input"])])
    assert _body(out) == _body(os.path.join(GOLD, case["ref_bc"]))


@pytest.mark.parametrize("world", [1, 2, 4])
@pytest.mark.parametrize("case", MANIFEST["bloom"], ids=lambda c: c["name"])
def test_bc_gpus_n_file_is_byte_identical_to_the_reference(cli, tmp_path, case, world):
    """`jellyfish-amd bc --gpus 2 / 4` (sub_commands/bc_main.cc:84-161 with the input split between the GPUs): rank
    processes -- on this box's one GPU over the inter-process transport -- each insert their part of the file into their
    own counter, the counters are merged on the device (jfgpu_comm_bc_merge: cells saturate at 2 and increments commute,
    bloom_counter2.hpp:56-107) and rank 0 writes the file: its body must be the REFERENCE's golden file's, byte for byte,
    and `count --bc` through it must give the golden filtered dump.  World 1: the RCCL transport itself, the rank's
    own share sent through ncclSend / ncclRecv (JFGPU_COMM_SELF_RCCL=1) -- every RCCL call an N-rank merge makes."""
    out = str(tmp_path / "out.bc")
    env = dict(os.environ, JFGPU_PARSE_CHUNK="100000", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    env.update({"JFGPU_COMM_SELF_RCCL": "1"} if world == 1 else {"JFGPU_COMM_TRANSPORT": "ipc"})
    cmd = [cli, "bc", "-m", str(case["k"]), "-s", str(case["n"]), "-f", str(case["fpr"]), "-o", out, "--gpus", str(world)] + (["-C"] if case["canonical"] else [])
    subprocess.check_call(cmd + [os.path.join(GOLD, case["input"])], env=env, timeout=900)
    assert _body(out) == _body(os.path.join(GOLD, case["ref_bc"]))
    jf = str(tmp_path / "f.jf")
    subprocess.check_call([cli, "count", "-m", str(case["k"]), "-s", "64k", "--bc", out, "-o", jf] + (["-C"] if case["canonical"] else []) + [os.path.join(GOLD, case["input"])])
    got = sorted(subprocess.check_output([cli, "dump", "-c", jf]).decode().splitlines())
    assert got == open(os.path.join(GOLD, case["name"] + ".filtered.dump")).read().splitlines()


def test_cli_reproduces_the_reference_golden_md5s(cli, tmp_path):
    """The reference's own integration goldens (tests/parallel_hashing.sh:7-19) on its own seeded inputs
    (tests/generate_sequence.sh:6-7, generated here by the reference's generator built in oracle/_ref),
    computed by jellyfish-amd: histo / stats / sorted dump md5s, incl. table doubling from -s 2M, k = 40
    (two-word keys) and -L/-U."""
    import hashlib
    if not os.access(O.REF_GEN, os.X_OK):
        pytest.skip("oracle/_ref not built")
    g = MANIFEST["reference_md5"]
    d = str(tmp_path)
    subprocess.check_call([O.REF_GEN, "-o", "seq10m"] + g["seq10m"], cwd=d)
    subprocess.check_call([O.REF_GEN, "-o", "seq1m"] + g["seq1m"], cwd=d)

    def md5(cmd, post=None):
        out = subprocess.check_output(cmd, cwd=d)
        if post:
            out = post(out)
        return hashlib.md5(out).hexdigest()
    subprocess.check_call([cli, "count", "-t", "4", "-o", "m15.jf", "-s", "2M", "-C", "-m", "15", "seq10m.fa"], cwd=d)
    assert md5([cli, "histo", "m15.jf"]) == g["m15_s2M.histo"]
    assert md5([cli, "stats", "m15.jf"]) == g["m15.stats"]
    subprocess.check_call([cli, "count", "-t", "4", "-o", "m15b.jf", "-s", "16M", "-C", "-m", "15", "seq10m.fa"], cwd=d)
    assert md5([cli, "histo", "m15b.jf"]) == g["m15_s2M.histo"]                      # ..._m15_s16M.histo: same md5
    for flag, tag in (([], "bin"), (["--text"], "txt")):
        subprocess.check_call([cli, "count", "-m", "40", "-t", "4", "-o", tag + ".jf", "-s", "2M"] + flag + ["seq1m_0.fa"], cwd=d)
        assert md5([cli, "dump", "-c", tag + ".jf"], lambda o: b"".join(sorted(o.splitlines(True)))) == g["binary.dump"]
        assert md5([cli, "histo", tag + ".jf"]) == g["binary.histo"]
        assert md5([cli, "stats", tag + ".jf"]) == g["binary.stats"]
    subprocess.check_call([cli, "count", "-t", "4", "-o", "lu.jf", "-s", "2M", "-C", "-m", "15", "-L", "2", "-U", "3", "seq10m.fa"], cwd=d)
    assert md5([cli, "histo", "lu.jf"]) == g["m15_s2M_L2_U3.histo"]


def test_cli_reproduces_more_reference_goldens(cli, tmp_path):
    """Further md5 goldens of the reference's active integration tests, computed by jellyfish-amd:
    tests/multi_file.sh:7-27 (six files; gunzip generators with comments), tests/subset_hashing.sh:7-19
    (`--if`, k = 35 two-word keys and k = 10), tests/merge.sh:7-20 first block (k = 40 -C over five files),
    tests/small_mers.sh (k = 2..10: the histogram does not depend on the size hint).
    Same command lines as the scripts, size hints included (two-word tables double like the others)."""
    import gzip
    import hashlib
    if not os.access(O.REF_GEN, os.X_OK):
        pytest.skip("oracle/_ref not built")
    g = MANIFEST["reference_md5"]
    d = str(tmp_path)
    subprocess.check_call([O.REF_GEN, "-o", "seq10m"] + g["seq10m"], cwd=d)
    subprocess.check_call([O.REF_GEN, "-o", "seq1m"] + g["seq1m"], cwd=d)

    def histo_md5(jf):
        return hashlib.md5(subprocess.check_output([cli, "histo", jf], cwd=d)).hexdigest()
    seq1m = ["seq1m_%d.fa" % i for i in range(5)]
    # multi_file.sh
    subprocess.check_call([cli, "count", "-t", "4", "-F", "4", "-o", "mf.jf", "-s", "2M", "-C", "-m", "15",
                           "seq1m_0.fa", "seq1m_1.fa", "seq1m_2.fa", "seq10m.fa", "seq1m_3.fa", "seq1m_4.fa"], cwd=d)
    assert histo_md5("mf.jf") == "d93b7678037814c256d1d9120a0e6422"
    with open(os.path.join(d, "gunzip_cmds"), "w") as f:
        f.write("  \n  # Empty lines and comments just for fun\n")
        for name in seq1m:
            with open(os.path.join(d, name), "rb") as src, gzip.open(os.path.join(d, name + ".gz"), "wb") as dst:
                dst.write(src.read())
            f.write("gunzip -c ./%s.gz\n" % name)
    subprocess.check_call([cli, "count", "-t", "4", "-g", "gunzip_cmds", "-G", "2", "-C", "-m", "15", "-s", "2M", "-o", "mfz.jf", "seq10m.fa"], cwd=d)
    assert histo_md5("mfz.jf") == "d93b7678037814c256d1d9120a0e6422"
    with open(os.path.join(d, "fail_cmds"), "w") as f:
        f.write("false\n")
    assert subprocess.run([cli, "count", "-g", "fail_cmds", "-C", "-m", "15", "-s", "2M", "-o", "fail.jf"], cwd=d, capture_output=True).returncode != 0
    assert subprocess.run([cli, "count", "-C", "-m", "15", "-s", "2M", "-o", "fail.jf", "non_existent_sequence.fa"], cwd=d, capture_output=True).returncode != 0
    # subset_hashing.sh
    files = ["--if", "seq1m_0.fa", "--if", "seq1m_2.fa", "seq1m_1.fa", "seq1m_0.fa", "seq1m_3.fa", "seq1m_2.fa"]
    subprocess.check_call([cli, "count", "-t", "4", "-o", "if35.jf", "-s", "2M", "-C", "-m", "35"] + files, cwd=d)
    assert histo_md5("if35.jf") == "bd7a5f6ba000b282cd79cb9f342e7ede"
    subprocess.check_call([cli, "count", "-t", "4", "-o", "if10.jf", "-s", "6M", "-C", "-m", "10"] + files, cwd=d)
    assert histo_md5("if10.jf") == "8eb6d4a50aeba178e4847c2da71dbb70"
    # merge.sh, first block
    subprocess.check_call([cli, "count", "-t", "4", "-o", "m40.jf", "-s", "4M", "-C", "-m", "40",
                           "seq1m_0.fa", "seq1m_1.fa", "seq1m_0.fa", "seq1m_2.fa", "seq1m_2.fa"], cwd=d)
    assert histo_md5("m40.jf") == "72f1913b3503114c7df7a4dcc68ce867"
    # small_mers.sh
    for k in range(2, 11):
        subprocess.check_call([cli, "count", "-t", "4", "-o", "a.jf", "-s", "10M", "-c", "25", "-m", str(k), "-C", "seq10m.fa"], cwd=d)
        subprocess.check_call([cli, "count", "-t", "4", "-o", "b.jf", "-s", "1k", "-c", "5", "-m", str(k), "-C", "seq10m.fa"], cwd=d)
        assert subprocess.check_output([cli, "histo", "a.jf"], cwd=d) == subprocess.check_output([cli, "histo", "b.jf"], cwd=d)


def test_bloom_counter_two_word_keys_and_reference_golden(cli, tmp_path):
    """tests/bloom_counter.sh (k = 40): `bc` through generators, `count --bc` keeps exactly the k-mers seen twice
    (the histogram md5 of the script), a filter built from other files lets only collisions through; and the
    bloomcounter file itself is byte-identical to the one the reference binary writes for the same command."""
    import gzip
    import hashlib
    if not O.have_ref():
        pytest.skip("oracle/_ref not built")
    g = MANIFEST["reference_md5"]
    d = str(tmp_path)
    subprocess.check_call([O.REF_GEN, "-o", "seq1m"] + g["seq1m"], cwd=d)
    with open(os.path.join(d, "seq1m_0.fa"), "rb") as src, gzip.open(os.path.join(d, "seq1m_0.fa.gz"), "wb") as dst:
        dst.write(src.read())
    with open(os.path.join(d, "commands"), "w") as f:
        f.write("gunzip -c seq1m_0.fa.gz\ngunzip -c seq1m_0.fa.gz\n")
    subprocess.check_call([cli, "bc", "-t", "4", "-o", "twice.bc", "-s", "1M", "-C", "-m", "40", "-g", "commands", "-G", "2"], cwd=d)
    subprocess.check_call([cli, "count", "-t", "4", "-o", "plain.jf", "-s", "2M", "-C", "-m", "40", "seq1m_0.fa"], cwd=d)
    subprocess.check_call([cli, "count", "-t", "4", "-o", "filtered.jf", "--bc", "twice.bc", "-s", "2M", "-C", "-m", "40", "seq1m_0.fa"], cwd=d)
    subprocess.check_call([cli, "bc", "-t", "4", "-o", "none.bc", "-s", "2M", "-C", "-m", "40", "seq1m_0.fa", "seq1m_1.fa", "seq1m_1.fa"], cwd=d)
    subprocess.check_call([cli, "count", "-t", "4", "-o", "none.jf", "--bc", "none.bc", "-s", "1M", "-C", "-m", "40", "seq1m_0.fa"], cwd=d)
    histo = lambda jf: subprocess.check_output([cli, "histo", jf], cwd=d)
    assert hashlib.md5(histo("plain.jf")).hexdigest() == g["bloom_counter_noop.histo"]
    assert hashlib.md5(histo("filtered.jf")).hexdigest() == g["bloom_counter_noop.histo"]
    total = int(histo("plain.jf").split()[1])
    none = histo("none.jf").split()
    collisions = int(none[1]) if none else 0
    assert total // 500 > collisions
    # byte-identical to the reference's own bc on the same inputs (same default hash pair, same cells)
    subprocess.check_call([O.REF_JF, "bc", "-m", "40", "-s", "2000000", "-C", "-o", "ref_none.bc", "seq1m_0.fa", "seq1m_1.fa", "seq1m_1.fa"], cwd=d)
    assert _body(os.path.join(d, "none.bc")) == _body(os.path.join(d, "ref_none.bc"))
    subprocess.check_call([O.REF_JF, "count", "-m", "40", "-s", "1000000", "-C", "--bc", "none.bc", "-o", "ref_none.jf", "seq1m_0.fa"], cwd=d)
    assert sorted(subprocess.check_output([cli, "dump", "-c", "none.jf"], cwd=d).splitlines()) == \
        sorted(subprocess.check_output([O.REF_JF, "dump", "-c", "ref_none.jf"], cwd=d).splitlines())


def test_disk_spill_and_merge_reproduce_reference_goldens(cli, tmp_path):
    """tests/merge.sh:21-37: with --disk a table that fills up is written out as sorted runs <output>0, <output>1, ...
    which are merged at the end (or left alone with --no-merge and merged by the `merge` verb); binary and text;
    every route gives the histogram of the in-memory count (md5 72f1913b...).  tests/large_key.sh's --disk idea for
    one-word keys too: -s 2k --disk equals a big table."""
    import glob
    import hashlib
    if not os.access(O.REF_GEN, os.X_OK):
        pytest.skip("oracle/_ref not built")
    g = MANIFEST["reference_md5"]
    d = str(tmp_path)
    subprocess.check_call([O.REF_GEN, "-o", "seq1m"] + g["seq1m"], cwd=d)
    files = ["seq1m_0.fa", "seq1m_1.fa", "seq1m_0.fa", "seq1m_2.fa", "seq1m_2.fa"]
    histo_md5 = lambda jf: hashlib.md5(subprocess.check_output([cli, "histo", jf], cwd=d)).hexdigest()
    gold = "72f1913b3503114c7df7a4dcc68ce867"
    subprocess.check_call([cli, "count", "-t", "4", "-o", "parts", "-s", "1M", "--disk", "--no-merge", "-C", "-m", "40"] + files, cwd=d)
    parts = sorted(glob.glob(os.path.join(d, "parts[0-9]*")))
    assert len(parts) >= 3                                                     # 3 M distinct k-mers through a 1 M table
    subprocess.check_call([cli, "merge", "-o", "merged.jf"] + parts, cwd=d)
    assert histo_md5("merged.jf") == gold
    subprocess.check_call([cli, "count", "-t", "4", "-o", "auto.jf", "-s", "1M", "--disk", "-C", "-m", "40"] + files, cwd=d)
    assert histo_md5("auto.jf") == gold and not glob.glob(os.path.join(d, "auto.jf[0-9]*"))   # runs merged and unlinked
    subprocess.check_call([cli, "count", "-t", "4", "-o", "text.jf", "-s", "1M", "--text", "--disk", "-C", "-m", "40"] + files, cwd=d)
    assert histo_md5("text.jf") == gold
    if O.have_ref():                                                           # the reference reads the merged file
        assert hashlib.md5(subprocess.check_output([O.REF_JF, "histo", "auto.jf"], cwd=d)).hexdigest() == gold
        assert subprocess.check_output([O.REF_JF, "dump", "--check-order", "auto.jf"], cwd=d).decode().startswith("ORDER OK")
    # one-word keys, -L/-U applied at merge time (count_main.cc:360-363)
    subprocess.check_call([cli, "count", "-o", "big.jf", "-s", "8M", "-C", "-m", "21", "-L", "2"] + files, cwd=d)
    subprocess.check_call([cli, "count", "-o", "small.jf", "-s", "20k", "--disk", "-C", "-m", "21", "-L", "2"] + files, cwd=d)
    a = sorted(subprocess.check_output([cli, "dump", "-c", "big.jf"], cwd=d).splitlines())
    b = sorted(subprocess.check_output([cli, "dump", "-c", "small.jf"], cwd=d).splitlines())
    assert a == b and len(a) > 0


def test_large_key_golden_k100(cli, tmp_path):
    """tests/large_key.sh:7-18, the reference's own test of keys longer than two words: 100-mers of the first 10001 lines
    of seq1m_0.fa read from a pipe (/dev/fd/0), with a table that fits (-s 2M), a size hint 1000 times too small (-s 2k:
    the 256-bit-slot table doubles itself ten times) and -s 2k --disk (sorted runs merged at the end): the sorted k-mer
    list has the reference's golden md5 every time, and the reference's reader decodes our 25-byte keys."""
    import hashlib
    if not os.access(O.REF_GEN, os.X_OK):
        pytest.skip("oracle/_ref not built")
    g = MANIFEST["reference_md5"]
    d = str(tmp_path)
    subprocess.check_call([O.REF_GEN, "-o", "seq1m"] + g["seq1m"], cwd=d)
    head = b"".join(open(os.path.join(d, "seq1m_0.fa"), "rb").readlines()[:10001])

    def ordered_md5(jf, reader):
        out = subprocess.check_output([reader, "dump", "-c", jf], cwd=d)
        return hashlib.md5(b"".join(sorted(l.split(b" ")[0] + b"\n" for l in out.splitlines()))).hexdigest()
    for name, extra in (("m100_2M.jf", ["-s", "2M"]), ("m100_2k.jf", ["-s", "2k"]), ("m100_2k_disk.jf", ["-s", "2k", "--disk"])):
        subprocess.run([cli, "count", "-t", "4", "-o", name, "-m", "100"] + extra + ["/dev/fd/0"], input=head, cwd=d, check=True)
        assert ordered_md5(name, cli) == g["large_key_m100.ordered"], name
    if O.have_ref():
        assert ordered_md5("m100_2k.jf", O.REF_JF) == g["large_key_m100.ordered"]
        assert subprocess.check_output([O.REF_JF, "dump", "--check-order", "m100_2M.jf"], cwd=d).decode().startswith("ORDER OK")
        ref = subprocess.run([O.REF_JF, "count", "-m", "100", "-s", "2M", "-t", "2", "--no-write", "--digest", "r.txt", "/dev/fd/0"], input=head, cwd=d, check=True)
        assert subprocess.check_output([cli, "digest", "m100_2M.jf"], cwd=d).decode() == open(os.path.join(d, "r.txt")).read()


@pytest.mark.parametrize("flags", [["-Q", "5"], ["-Q", "P"], ["-Q", "Z"], ["-Q", "!"], ["--min-quality", "20"], ["-Q", "V", "--host-parse"]])
def test_min_quality_equals_the_reference(cli, flags, tmp_path):
    """count -Q / --min-quality (count_main.cc:234-256, mer_qual_iterator.hpp:75-84): bases whose quality character is below
    the threshold break k-mers like an N.  jellyfish-amd (device FASTQ parser with the masking kernel; host reader with
    --host-parse) against the reference driver running the reference's own whole_sequence_parser + mer_qual_iterator, on
    the reference generator's FASTQ (qualities uniform over the printable range) and on a wrapped (multi-line) copy that
    the device parser hands to the host reader; FASTA input is unaffected."""
    if not O.have_ref():
        pytest.skip("oracle/_ref not built")
    fq = os.path.join(GOLD, "reads_fq_s1473540700.fq")
    d = str(tmp_path)
    # a wrapped copy: sequence and quality lines cut at 40 columns (legal FASTQ, not the strict 4-line layout)
    lines = open(fq).read().splitlines()
    wrapped = []
    for i in range(0, len(lines) - 3, 4):
        wrapped.append(lines[i])
        wrapped += [lines[i + 1][j:j + 40] for j in range(0, len(lines[i + 1]), 40)]
        wrapped.append(lines[i + 2])
        wrapped += [lines[i + 3][j:j + 40] for j in range(0, len(lines[i + 3]), 40)]
    open(os.path.join(d, "wrapped.fq"), "w").write("\n".join(wrapped) + "\n")
    qchar = flags[1] if flags[0] == "-Q" else chr(64 + 20)       # --quality-start defaults to 64 (count_main_cmdline.yaggo)
    for name, path in (("strict", fq), ("wrapped", os.path.join(d, "wrapped.fq"))):
        subprocess.check_call([cli, "count", "-m", "4", "-C", "-s", "64k", "-o", name + ".jf"] + flags + [path], cwd=d)
        subprocess.check_call([O.REF_JF, "count", "-m", "4", "-C", "-s", "64k", "-t", "2", "-o", name + ".ref.jf", "-Q", qchar, path], cwd=d)
        mine = sorted(subprocess.check_output([cli, "dump", "-c", name + ".jf"], cwd=d).splitlines())
        ref = sorted(subprocess.check_output([O.REF_JF, "dump", "-c", name + ".ref.jf"], cwd=d).splitlines())
        assert mine == ref and len(ref) > 0, (name, flags)
    subprocess.check_call([O.REF_JF, "count", "-m", "4", "-C", "-s", "64k", "-o", "all.ref.jf", fq], cwd=d)
    unfiltered = sorted(subprocess.check_output([O.REF_JF, "dump", "-c", "all.ref.jf"], cwd=d).splitlines())
    if qchar <= "B":
        assert mine == unfiltered                               # the generator's qualities start at 'B': nothing is masked
    else:
        assert mine != unfiltered
    fa = os.path.join(GOLD, "reads150_s42.fa")
    subprocess.check_call([cli, "count", "-m", "21", "-C", "-s", "64k", "-o", "fa.jf"] + flags + [fa], cwd=d)
    assert sorted(subprocess.check_output([cli, "dump", "-c", "fa.jf"], cwd=d).decode().splitlines()) == \
        open(os.path.join(GOLD, "reads150_k21C.dump")).read().splitlines()


def test_bf_size_one_pass_filter_bound(cli, tmp_path):
    """tests/bloom_filter.sh:21-33 in small: files a b a c, `count --bf-size N --bf-fp 0.001`: the k-mers of a are seen twice
    and counted once, everything else only marks the filter; the sum of the histogram is |a| within the script's 2 % bound.
    (The reference's result is order- and thread-timing dependent too; the script only bounds it.)"""
    import random
    rng = random.Random(5)
    d = str(tmp_path)
    n = 100000
    for name in "abc":
        with open(os.path.join(d, name + ".fa"), "w") as fh:
            fh.write(">%s\n" % name)
            s = "".join(rng.choice("ACGT") for _ in range(n))
            fh.write("\n".join(s[i:i + 70] for i in range(0, n, 70)) + "\n")
    files = ["a.fa", "b.fa", "a.fa", "c.fa"]
    subprocess.check_call([cli, "count", "--bf-size", "300k", "--bf-fp", "0.001", "-t", "2", "-o", "bf.jf", "-s", "1M", "-m", "40"] + files, cwd=d)
    histo = subprocess.check_output([cli, "histo", "bf.jf"], cwd=d).decode().split()
    total = sum(int(x) for x in histo[1::2])
    expected = n - 39
    assert 0 <= total - expected <= 0.02 * expected, (total, expected)
    if O.have_ref():
        assert subprocess.check_output([O.REF_JF, "histo", "bf.jf"], cwd=d).decode().split() == histo
    r = subprocess.run([cli, "count", "--bf-size", "1M", "--bc", "x", "-m", "21", "-s", "1M", "a.fa"], cwd=d, capture_output=True)
    assert r.returncode == 1 and b"conflict" in r.stderr


def _tricky_fastq(path, rng, n):
    """FASTQ whose quality lines often start with '@' and whose sequences have 'N's: the record-boundary test must not be
    fooled by a quality line."""
    with open(path, "wb") as f:
        for r in range(n):
            L = rng.choice([40, 75, 151])
            seq = "".join(rng.choice("ACGTN" if rng.random() < 0.1 else "ACGT") for _ in range(L))
            qual = "".join(rng.choice("@+IIIIHHGG#5") for _ in range(L))
            if r % 3 == 0:
                qual = "@" + qual[1:]
            f.write(("@r%d\n%s\n+\n%s\n" % (r, seq, qual)).encode())


def test_file_parts_cover_the_file_exactly_once(cli, tmp_path):
    """What the ranks of `count --gpus N` read: part r of N of every file, cut at record boundaries found independently
    (device_sequence_parser::parse_file_part).  JFGPU_TEST_PARTS=N makes one process read the N parts one after the other:
    the output must be the plain run's, for multi-line FASTA (records of very different lengths: some parts are empty),
    FASTQ with '@' quality lines, pinned and mapped feeds."""
    import random
    rng = random.Random(5)
    fa = tmp_path / "multi.fa"
    with open(fa, "wb") as f:
        for r in range(120):
            seq = "".join(rng.choice("ACGT") for _ in range(rng.choice([30, 500, 30000])))
            f.write((">s%d\n" % r).encode())
            for i in range(0, len(seq), 70):
                f.write(seq[i:i + 70].encode() + b"\n")
    fq = tmp_path / "tricky.fq"
    _tricky_fastq(fq, rng, 4000)
    for inp in (str(fa), str(fq)):
        ref = str(tmp_path / "ref.jf")
        subprocess.check_call([cli, "count", "-m", "22", "-C", "-s", "4M", "-o", ref, inp])
        want = _body(ref)                     # (headers differ by the command line / time; bodies must not)
        for parts, pinned in ((2, "0"), (3, "1"), (8, "0"), (64, "1")):
            o = str(tmp_path / ("p%d.jf" % parts))
            subprocess.check_call([cli, "count", "-m", "22", "-C", "-s", "4M", "-o", o, inp],
                                  env=dict(os.environ, JFGPU_TEST_PARTS=str(parts), JFGPU_FEED_PINNED=pinned, JFGPU_PARSE_CHUNK="100000"))
            assert _body(o) == want and len(want) > 0, (inp, parts)


@pytest.mark.parametrize("self_rccl", ["0", "1"])
def test_count_gpus_1_goes_through_the_ranks_machinery(cli, tmp_path, self_rccl):
    """`count --gpus 1`: the command starts one rank process (rendezvous directory, RCCL id, communicator of world 1), the
    rank routes every k-mer through the exchange (JFGPU_COMM_SELF_RCCL=1: through ncclSend / ncclRecv to itself), agrees on
    the number of steps, and writes its records through the sharded writer.  File body and digest equal the plain run's."""
    case = next(c for c in MANIFEST["cases"] if c["name"] == "reads150_k21C")
    inp = os.path.join(GOLD, case["input"])
    ref, out = str(tmp_path / "ref.jf"), str(tmp_path / "g1.jf")
    dg0, dg1 = str(tmp_path / "d0.txt"), str(tmp_path / "d1.txt")
    subprocess.check_call([cli, "count", "-m", "21", "-C", "-s", case["size"], "-o", ref, "--digest", dg0, inp])
    subprocess.check_call([cli, "count", "-m", "21", "-C", "-s", case["size"], "-o", out, "--digest", dg1, "--gpus", "1", "--timing", str(tmp_path / "t"), inp],
                          env=dict(os.environ, JFGPU_COMM_SELF_RCCL=self_rccl, JFGPU_PARSE_CHUNK="200000"), timeout=600)
    assert open(dg0).read() == open(dg1).read()
    assert _body(out) == _body(ref)
    assert subprocess.check_output([cli, "stats", out]) == subprocess.check_output([cli, "stats", ref])
    assert open(tmp_path / "t").read().split()[0::2] == ["Init", "Counting", "Writing"]
    for bad in (["--gpus", "3"], ["--gpus", "2", "--disk"], ["--gpus", "2", "--bf-size", "1M"]):      # (round 6: --text, -g and --host-parse are taken with --gpus)
        r = subprocess.run([cli, "count", "-m", "21", "-s", "1M", "-o", out] + bad + [inp], capture_output=True)
        assert r.returncode != 0 and b"--gpus" in r.stderr


@pytest.mark.parametrize("world,items,k", [(2, "2", 21), (4, "2", 21), (2, "0", 21), (2, "1", 63), (4, "1", 40)])
def test_count_gpus_n_as_rank_processes_on_one_device(cli, tmp_path, world, items, k):
    """`count --gpus 2 / 4` as REAL rank processes (the command forks them; rendezvous directory; every rank reads its part
    of the file, routes by hash prefix, exchanges, writes its records at its offset of the common file) -- on this box's
    single GPU through the inter-process transport (JFGPU_COMM_TRANSPORT=ipc: hipIpc* copies between the ranks' device
    buffers, host-level collectives in shared memory).  Item path (JFGPU_COMM_ITEMS=2) and key path (=0); two-word keys
    (k = 40, 63: shards of 128-bit slots, two words per routed k-mer -- round 4).  File body, digest and stats equal the
    single-process run's."""
    import random
    rng = random.Random(17 + world)
    fa = tmp_path / "reads.fa"
    with open(fa, "wb") as f:
        for r in range(6000):
            f.write((">r%d\n%s\n" % (r, "".join(rng.choice("ACGT") for _ in range(150)))).encode())
    ref, out = str(tmp_path / "ref.jf"), str(tmp_path / "gN.jf")
    dg0, dg1 = str(tmp_path / "d0.txt"), str(tmp_path / "d1.txt")
    size = "64M" if k <= 32 else "1G"                         # (k = 63 needs 2^29 slots; every rank's shard a share of them)
    subprocess.check_call([cli, "count", "-m", str(k), "-C", "-s", size, "-o", ref, "--digest", dg0, str(fa)])
    env = dict(os.environ, JFGPU_COMM_TRANSPORT="ipc", JFGPU_COMM_ITEMS=items, JFGPU_PARSE_CHUNK="150000", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    subprocess.check_call([cli, "count", "-m", str(k), "-C", "-s", size, "-o", out, "--digest", dg1, "--gpus", str(world), str(fa)], env=env, timeout=900)
    assert open(dg0).read() == open(dg1).read()
    assert _body(out) == _body(ref) and len(_body(ref)) > 0
    assert subprocess.check_output([cli, "stats", out]) == subprocess.check_output([cli, "stats", ref])


@pytest.mark.parametrize("world,k", [(2, 21), (4, 21), (2, 40)])
def test_count_gpus_n_with_a_size_hint_far_too_small(cli, tmp_path, world, k):
    """`-s` is a hint with --gpus too (doc/Readme.md:67-72; round-3 review, missing #1: `count --gpus 8 -s <too small>` was
    "Hash full"): rank processes whose shards start at 1 k slots double them together, as often as it takes, and the file
    they write holds the single-process run's counts, in (pos, key) order under the matrix its header names (the
    reference's reader checks the order).  k = 40: shards of two-word keys grow the same way (round 4)."""
    import random
    rng = random.Random(23 + world)
    fa = tmp_path / "reads.fa"
    with open(fa, "wb") as f:
        for r in range(3000):
            f.write((">r%d\n%s\n" % (r, "".join(rng.choice("ACGT") for _ in range(150)))).encode())
    ref, out = str(tmp_path / "ref.jf"), str(tmp_path / "gN.jf")
    subprocess.check_call([cli, "count", "-m", str(k), "-C", "-s", "1k", "-o", ref, str(fa)])
    env = dict(os.environ, JFGPU_COMM_TRANSPORT="ipc", JFGPU_PARSE_CHUNK="100000", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    subprocess.check_call([cli, "count", "-m", str(k), "-C", "-s", "1k", "-o", out, "--gpus", str(world), str(fa)], env=env, timeout=900)
    want = sorted(subprocess.check_output([cli, "dump", "-c", ref]).decode().splitlines())
    got = subprocess.check_output([cli, "dump", "-c", out]).decode().splitlines()
    assert sorted(got) == want and len(want) > 300000
    assert subprocess.check_output([cli, "stats", out]) == subprocess.check_output([cli, "stats", ref])
    if O.have_ref():
        assert subprocess.check_output([O.REF_JF, "dump", "--check-order", out]).decode().startswith("ORDER OK %d" % len(want))


@pytest.mark.parametrize("k", [21, 31, 40])
def test_count_gpus_n_with_a_bloom_counter_file(cli, tmp_path, k):
    """`count --bc file --gpus 2` (count_main.cc:109-119, 191-206 with hash-prefix shards; round-3 review, missing #1): every
    rank process loads the counter file and asks it before routing; the file the ranks write equals the single-process
    `count --bc` file.  k = 21 takes the item path, k = 31 the key path, k = 40 (round 6) the key path of two-word keys:
    route_count / route_scatter_kernel<WideTable, BLOOM> ask the counter on the sending side."""
    import random
    rng = random.Random(101 + k)
    twice = ["".join(rng.choice("ACGT") for _ in range(150)) for _ in range(1500)]
    fa = tmp_path / "reads.fa"
    with open(fa, "wb") as f:
        for r in range(4000):
            seq = twice[r % 1500] if r < 3000 else "".join(rng.choice("ACGT") for _ in range(150))
            f.write((">r%d\n%s\n" % (r, seq)).encode())
    bc, ref, out = str(tmp_path / "reads.bc"), str(tmp_path / "ref.jf"), str(tmp_path / "g2.jf")
    subprocess.check_call([cli, "bc", "-m", str(k), "-C", "-s", "1M", "-f", "0.01", "-o", bc, str(fa)])
    subprocess.check_call([cli, "count", "-m", str(k), "-C", "-s", "4M", "--bc", bc, "-o", ref, str(fa)])
    env = dict(os.environ, JFGPU_COMM_TRANSPORT="ipc", JFGPU_PARSE_CHUNK="100000", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    subprocess.check_call([cli, "count", "-m", str(k), "-C", "-s", "4M", "--bc", bc, "-o", out, "--gpus", "2", str(fa)], env=env, timeout=900)
    want = subprocess.check_output([cli, "dump", "-c", ref]).decode().splitlines()
    got = subprocess.check_output([cli, "dump", "-c", out]).decode().splitlines()
    assert sorted(got) == sorted(want) and 100000 < len(want) < 400000      # (the once-seen reads' k-mers are not admitted)
    assert subprocess.check_output([cli, "stats", out]) == subprocess.check_output([cli, "stats", ref])


@pytest.mark.parametrize("k", [21, 40])
def test_count_gpus_n_with_if_files(cli, tmp_path, k):
    """`count --if wanted.fa --gpus 2` (count_main.cc:289-295 with hash-prefix shards; round-3 review, missing #1): the rank
    processes prime their shards with the --if k-mers (each reads its part of the file, every k-mer travels to its owner),
    then count only those; the file equals the single-process one.  k = 40 (round 6): shards of two-word keys -- the PRIME
    pass adds with value 0, the UPDATE pass goes through update_keys_kernel<WideTable> on arrival."""
    import random
    rng = random.Random(77)
    wanted = ["".join(rng.choice("ACGT") for _ in range(200)) for _ in range(600)]
    iff, fa = tmp_path / "wanted.fa", tmp_path / "reads.fa"
    with open(iff, "wb") as f:
        for i, w in enumerate(wanted):
            f.write((">w%d\n%s\n" % (i, w)).encode())
    with open(fa, "wb") as f:
        for r in range(3000):
            seq = wanted[r % 600][20:170] if r % 3 else "".join(rng.choice("ACGT") for _ in range(150))
            f.write((">r%d\n%s\n" % (r, seq)).encode())
    ref, out = str(tmp_path / "ref.jf"), str(tmp_path / "g2.jf")
    subprocess.check_call([cli, "count", "-m", str(k), "-C", "-s", "1M", "--if", str(iff), "-o", ref, str(fa)])
    env = dict(os.environ, JFGPU_COMM_TRANSPORT="ipc", JFGPU_PARSE_CHUNK="100000", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    subprocess.check_call([cli, "count", "-m", str(k), "-C", "-s", "1M", "--if", str(iff), "-o", out, "--gpus", "2", str(fa)], env=env, timeout=900)
    want = subprocess.check_output([cli, "dump", "-c", ref]).decode().splitlines()
    got = subprocess.check_output([cli, "dump", "-c", out]).decode().splitlines()
    assert sorted(got) == sorted(want) and len(want) > 90000
    assert any(l.endswith(" 0") for l in want) and any(not l.endswith(" 0") for l in want)     # primed and never seen / counted
    assert subprocess.check_output([cli, "stats", out]) == subprocess.check_output([cli, "stats", ref])


@pytest.mark.parametrize("world,k", [(2, 21), (4, 21), (2, 40)])
def test_count_gpus_n_text_output(cli, tmp_path, world, k):
    """`count --text --gpus N` (text_dumper.hpp:18-20 over hash-prefix shards; round 6): a text record has no fixed width, so
    every rank writes its lines to a part beside the output and rank 0 appends them in rank order -- the body is, line for
    line and in the same order, the single-process `--text` file's, and no part file is left behind."""
    import glob
    import random
    rng = random.Random(31 + world + k)
    fa = tmp_path / "reads.fa"
    with open(fa, "wb") as f:
        for r in range(3000):
            f.write((">r%d\n%s\n" % (r, "".join(rng.choice("ACGT") for _ in range(150)))).encode())
    ref, out = str(tmp_path / "ref.txt"), str(tmp_path / "gN.txt")
    subprocess.check_call([cli, "count", "-m", str(k), "-C", "-s", "4M", "--text", "-o", ref, str(fa)])
    env = dict(os.environ, JFGPU_COMM_TRANSPORT="ipc", JFGPU_PARSE_CHUNK="100000", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    subprocess.check_call([cli, "count", "-m", str(k), "-C", "-s", "4M", "--text", "-o", out, "--gpus", str(world), str(fa)], env=env, timeout=900)
    assert _body(out) == _body(ref) and len(_body(ref)) > 1_000_000
    assert not glob.glob(out + ".rank*")
    assert subprocess.check_output([cli, "histo", out]) == subprocess.check_output([cli, "histo", ref])


@pytest.mark.parametrize("how", ["generators", "host-parse", "generators+files"])
def test_count_gpus_n_with_generators_and_the_host_reader(cli, tmp_path, how):
    """`count --gpus 2 -g cmds` and `--host-parse` (round 6): input that no rank can cut into parts -- streams of generator
    commands (lib/generator_manager.cc), files read by the host reader -- is dealt out whole: command j to rank j mod N,
    file i to rank i mod N.  Ranks end up with different numbers of steps (the facade keeps stepping with nothing until
    nobody has input); the file equals the single-process one.  Three commands / files for two ranks: an uneven deal."""
    import gzip
    import random
    rng = random.Random(len(how))
    fas = []
    for i in range(3):
        fa = tmp_path / ("part%d.fa" % i)
        with open(fa, "wb") as f:
            for r in range(800 + 700 * i):
                f.write((">r%d_%d\n%s\n" % (i, r, "".join(rng.choice("ACGT") for _ in range(150)))).encode())
        fas.append(str(fa))
    gz = str(tmp_path / "part0.fa.gz")
    with open(fas[0], "rb") as f, gzip.open(gz, "wb") as g:
        g.write(f.read())
    gen = tmp_path / "generators"
    gen.write_text("gzip -dc %s\n# a comment\ncat %s\n\ncat %s\n" % (gz, fas[1], fas[2]))
    ref, out = str(tmp_path / "ref.jf"), str(tmp_path / "g2.jf")
    subprocess.check_call([cli, "count", "-m", "21", "-C", "-s", "4M", "-o", ref] + fas)
    env = dict(os.environ, JFGPU_COMM_TRANSPORT="ipc", JFGPU_PARSE_CHUNK="100000", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    if how == "generators":
        args = ["-g", str(gen)]
    elif how == "host-parse":
        args = ["--host-parse"] + fas
    else:
        gen.write_text("gzip -dc %s\ncat %s\n" % (gz, fas[1]))
        args = ["-g", str(gen), fas[2]]
    subprocess.check_call([cli, "count", "-m", "21", "-C", "-s", "4M", "-o", out, "--gpus", "2"] + args, env=env, timeout=900)
    want = subprocess.check_output([cli, "dump", "-c", ref])
    assert subprocess.check_output([cli, "dump", "-c", out]) == want and len(want) > 1_000_000


def test_a_failing_rank_ends_the_others(cli, tmp_path):
    """One rank of `count --gpus 2` cannot read its input (the file disappears for rank 1 only: JFGPU_TEST_FAIL_RANK): the
    command must come back with an error instead of leaving the other rank waiting in a collective."""
    fa = tmp_path / "reads.fa"
    fa.write_bytes(b">r\n" + b"ACGT" * 5000 + b"\n")
    env = dict(os.environ, JFGPU_COMM_TRANSPORT="ipc", JFGPU_TEST_FAIL_RANK="1")
    r = subprocess.run([cli, "count", "-m", "21", "-C", "-s", "64M", "-o", str(tmp_path / "x.jf"), "--gpus", "2", str(fa)], env=env, capture_output=True, timeout=300)
    assert r.returncode != 0


def test_pipes_are_read_in_pieces_of_whole_records(cli, tmp_path):
    """Input that cannot be mapped (a pipe: `zcat reads.fa.gz |`, generator commands) used to be read whole into memory
    before anything was parsed; it is now handed over in pieces that end where a record starts.  With pieces of 700 bytes
    (JFGPU_STREAM_PIECE) against records of up to 30 kb, multi-line FASTA and FASTQ with '@' quality lines through a FIFO
    and through -g give the same file body as the plain files."""
    import random
    rng = random.Random(8)
    fa = tmp_path / "multi.fa"
    with open(fa, "wb") as f:
        for r in range(60):
            seq = "".join(rng.choice("ACGT") for _ in range(rng.choice([30, 500, 30000])))
            f.write((">s%d\n" % r).encode())
            for i in range(0, len(seq), 70):
                f.write(seq[i:i + 70].encode() + b"\n")
    fq = tmp_path / "tricky.fq"
    _tricky_fastq(fq, rng, 1500)
    for inp in (str(fa), str(fq)):
        ref, out, outg = str(tmp_path / "ref.jf"), str(tmp_path / "pipe.jf"), str(tmp_path / "gen.jf")
        subprocess.check_call([cli, "count", "-m", "22", "-C", "-s", "4M", "-o", ref, inp])
        env = dict(os.environ, JFGPU_STREAM_PIECE="700")
        subprocess.check_call("cat %s | %s count -m 22 -C -s 4M -o %s /dev/stdin" % (inp, cli, out), shell=True, env=env)
        assert _body(out) == _body(ref) and len(_body(ref)) > 0
        gen = tmp_path / "gen.txt"
        gen.write_text("cat %s\n" % inp)
        subprocess.check_call([cli, "count", "-m", "22", "-C", "-s", "4M", "-o", outg, "-g", str(gen)], env=env)
        assert _body(outg) == _body(ref)
