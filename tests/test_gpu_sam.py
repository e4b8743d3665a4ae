"""`count --sam`: BGZF inflated and BAM records decoded on the device (kernels_bgzf.hip.hpp, abi_sam.inl,
jellyfish_amd/include/jellyfish_amd/sam_parser.hpp).  -m gpu only; tests/test_sam_emu.py runs a selection of these on
the host emulation.

  * the device inflate equals zlib byte for byte for every deflate variant; a bad CRC32 / ISIZE, a truncated or damaged
    member is an error (JFGPU_E_CORRUPT), never a fault or a wrong output
  * the record decode finds every record start whatever the guesses meet (fake headers in names and aux data, a read
    over many members, members that end on record boundaries, empty reads, a header of many megabytes, small chunks)
  * `count --sam` on BAM, BGZF SAM and SAM text writes the file `count` writes for the same reads as FASTQ / FASTA
"""
import os
import random
import struct
import subprocess
import gzip

import pytest

import oracle_lib as O
import sam_fixtures as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.environ.get("JFGPU_CLI") or os.path.join(ROOT, "bin", "jellyfish-amd")


@pytest.fixture(scope="module")
def cli(gpu):
    if not os.environ.get("JFGPU_CLI"):
        subprocess.check_call(["make", "-s", "cli"], cwd=ROOT)
    return CLI


@pytest.fixture()
def tools(gpu):
    t = gpu.Table(k=21, size=1 << 12)      # only used for raw device copies
    p = gpu.Parser(21)
    yield gpu, p, t
    p.close(); t.close()


def payloads():
    rng = random.Random(7)
    return {
        "random": bytes(rng.getrandbits(8) for _ in range(140000)),
        "repetitive": (b"ACGTTGCA" * 4000 + b"N" * 9000 + b"GA" * 7000) * 3,
        "bam": F.bam_stream(F.random_records(400, 3)),
    }


@pytest.mark.parametrize("variant", sorted(F.VARIANTS))
def test_inflate_equals_zlib(tools, variant):
    capi, p, t = tools
    for name, data in payloads().items():
        z = F.bgzf(data, block_size=60000 if variant == "stored" else 65280, variants=(variant,), empty_at=(1, 2))
        n = p.inflate(z)
        assert n == len(data)
        assert p.stream_read(0, n) == data, (name, variant)
        p.stream_consume(n)
    # every variant in one file, members of odd sizes
    data = payloads()["bam"]
    z = F.bgzf(data, block_size=7777, variants=tuple(sorted(F.VARIANTS)))
    n = p.inflate(z)
    assert p.stream_read(0, n) == data


def test_damaged_members_are_errors_not_faults(tools):
    capi, p, t = tools
    data = payloads()["bam"]
    good = F.bgzf(data, block_size=20000, eof=False)
    blocks, used = capi.bgzf_scan(good)
    assert used == len(good) and len(blocks) == (len(data) + 19999) // 20000

    def expect_corrupt(z, table=None):
        with pytest.raises(capi.JfgpuError) as e:
            p.inflate(z) if table is None else p.inflate_table(z, table)
        assert e.value.code == capi.E_CORRUPT, e.value.msg
        return e.value.msg

    b1 = blocks[1]
    crc_at = b1.c_off + b1.c_len
    bad = bytearray(good); bad[crc_at] ^= 1
    assert "CRC32" in expect_corrupt(bytes(bad))
    bad = bytearray(good); bad[crc_at + 4] ^= 1                  # ISIZE one more / one less
    assert "ISIZE" in expect_corrupt(bytes(bad))
    # a member cut short: its deflate data ends early (the table says so)
    table = capi.bgzf_scan(good)[0]
    table[2].c_len = table[2].c_len // 2
    expect_corrupt(good, table)
    # damaged deflate bytes: an error, whatever the damage hits
    rng = random.Random(5)
    for _ in range(12):
        bad = bytearray(good)
        at = b1.c_off + rng.randrange(b1.c_len - 1)              # (not the last byte: it may end in padding bits)
        bad[at] ^= 1 << rng.randrange(8)
        expect_corrupt(bytes(bad))
    # truncated file: the member is not complete, the scan leaves it out
    bl, u = capi.bgzf_scan(good[:len(good) - 100])
    assert len(bl) == len(blocks) - 1
    # plain gzip is not BGZF
    with pytest.raises(capi.JfgpuError) as e:
        capi.bgzf_scan(gzip.compress(data[:1000]))
    assert e.value.code == capi.E_CORRUPT and "BGZF" in e.value.msg
    # the parser still works
    n = p.inflate(good)
    assert p.stream_read(0, n) == data


def decode_via_api(capi, p, t, z, chunk_members):
    """What sam_parser does: chunks of whole members, the header read back on the host, records decoded on the device."""
    blocks, used = capi.bgzf_scan(z)
    starts = [b.c_off - 18 for b in blocks] + [used]
    out, hdr, n_ref, skip_done, records = b"", b"", None, False, 0
    for i in range(0, len(blocks), chunk_members):
        a, b = starts[i], starts[min(i + chunk_members, len(blocks))]
        n = p.inflate(z[a:b], which=(i // chunk_members) % 2)
        skip = 0
        if not skip_done:
            before = len(hdr)
            hdr += p.stream_read(0, n)
            H = header_length(hdr)
            if H is None:
                p.stream_consume(n)
                continue
            H, n_ref = H
            skip, skip_done = H - before, True
        ptr, n_out, recs, left = p.bam_decode(skip, n_ref)
        records += recs
        if n_out:
            out += bytes(t.d2h(ptr, n_out))
    return out, records, left


def header_length(h):
    if len(h) < 12:
        return None
    l_text = struct.unpack_from("<i", h, 4)[0]
    at = 8 + l_text
    if len(h) < at + 4:
        return None
    n_ref = struct.unpack_from("<i", h, at)[0]
    at += 4
    for _ in range(n_ref):
        if len(h) < at + 4:
            return None
        at += 8 + struct.unpack_from("<i", h, at)[0]
        if len(h) < at:
            return None
    return at, n_ref


def fake_record_aux(n_ref):
    """Aux data (a 'B' uint8 array) whose bytes look like a complete, plausible record."""
    name = b"fake\0"
    body = struct.pack("<iiBBHHHiiii", 0, 100, len(name), 0, 4680, 0, 0, 4, -1, -1, 0) + name + b"\x12\x48" + b"\x1e" * 4
    fake = struct.pack("<i", len(body)) + body
    return b"ZBBC" + struct.pack("<i", len(fake)) + fake


def defeating_records():
    rng = random.Random(11)
    recs = []
    for i in range(300):
        L = rng.choice([0, 0, 1, 20, 150, 151, 600])
        seq = "".join(rng.choice("ACGTNacgt=RY") for _ in range(L))
        qual = None if rng.random() < 0.1 else [rng.randint(0, 60) for _ in range(L)]
        aux = fake_record_aux(2) * rng.randint(0, 3)
        name = "r%d_%s" % (i, "!" * rng.randint(0, 40))
        recs.append(F.Record(name, seq, qual, flag=rng.choice([0, 4, 256, 2048]), ref=rng.choice([-1, 0, 1]),
                             pos=rng.randint(-1, 1000), cigar=[(L, 0)] if L and rng.random() < 0.5 else [], aux=aux))
    return recs


CASES = ["fake_headers", "long_read", "aligned_members", "empty_reads", "big_header"]


def case_file(case):
    refs = (("chr1", 100000), ("chr2", 5000))
    if case == "fake_headers":
        recs = defeating_records()
        return recs, refs, F.bgzf(F.bam_stream(recs, refs), block_size=3000, variants=("default", "fixed", "stored"))
    if case == "long_read":
        rng = random.Random(2)
        recs = F.random_records(30, 4) + [F.Record("long", "".join(rng.choice("ACGT") for _ in range(300000)),
                                                   [rng.randint(0, 40) for _ in range(300000)])] + F.random_records(30, 5, name_prefix="s")
        return recs, refs, F.bgzf(F.bam_stream(recs, refs), block_size=65280)
    if case == "aligned_members":
        recs = F.random_records(200, 6, length=(0, 300))
        offs = F.record_offsets(recs, refs)
        return recs, refs, F.bgzf(F.bam_stream(recs, refs), cuts=offs[::3], empty_at=(4, 9))
    if case == "empty_reads":
        recs = [F.Record("e%d" % i, "" if i % 2 else "ACGTA" * (i % 7), None if i % 3 == 0 else [30] * (5 * (i % 7) * (i % 2 == 0)))
                for i in range(500)]
        return recs, refs, F.bgzf(F.bam_stream(recs, refs), block_size=1000)
    if case == "big_header":
        refs = tuple(("contig_%06d_with_a_long_name" % i, 1000 + i) for i in range(50000))
        text = b"".join(b"@SQ\tSN:contig_%06d_with_a_long_name\tLN:%d\n" % (i, 1000 + i) for i in range(50000))
        recs = F.random_records(300, 8)
        for i, r in enumerate(recs):
            r.ref, r.pos = i % 50000, i
        return recs, refs, F.bgzf(F.bam_stream(recs, refs, text=text), block_size=65280)
    raise KeyError(case)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("chunk_members", [1, 3, 1000])
def test_record_starts_equal_the_serial_walk(tools, case, chunk_members):
    capi, p, t = tools
    recs, refs, z = case_file(case)
    out, n, left = decode_via_api(capi, p, t, z, chunk_members)
    assert left == 0
    assert n == len(recs)
    assert out == F.contract(recs)
    p.set_min_quality(ord("+"))
    out, n, left = decode_via_api(capi, p, t, z, chunk_members)
    assert out == F.contract(recs, ord("+"))


def test_truncated_and_corrupt_bam_are_refused(cli, tmp_path):
    recs = F.random_records(50, 9)
    data = F.bam_stream(recs)
    z = F.bgzf(data[:-40], block_size=4000)                    # the last record is cut
    (tmp_path / "t.bam").write_bytes(z)
    r = subprocess.run([cli, "count", "-m", "21", "-s", "1M", "-o", str(tmp_path / "o.jf"), "--sam", str(tmp_path / "t.bam")], capture_output=True)
    assert r.returncode != 0 and b"t.bam" in r.stderr and b"truncated" in r.stderr
    bad = bytearray(data); bad[len(F.bam_header((("chr1", 1000000),))) + 20] = 0xFF   # l_seq of the first record
    (tmp_path / "c.bam").write_bytes(F.bgzf(bytes(bad), block_size=4000))
    r = subprocess.run([cli, "count", "-m", "21", "-s", "1M", "-o", str(tmp_path / "o.jf"), "--sam", str(tmp_path / "c.bam")], capture_output=True)
    assert r.returncode != 0 and b"c.bam" in r.stderr
    z = bytearray(F.bgzf(data, block_size=4000)); z[100] ^= 0x10
    (tmp_path / "d.bam").write_bytes(bytes(z))
    r = subprocess.run([cli, "count", "-m", "21", "-s", "1M", "-o", str(tmp_path / "o.jf"), "--sam", str(tmp_path / "d.bam")], capture_output=True)
    assert r.returncode != 0 and b"d.bam" in r.stderr


def test_bgzf_with_another_extra_subfield_before_bc(cli, tmp_path):
    """The BGZF spec lets the 'BC' subfield sit anywhere in the gzip extra field."""
    recs = F.random_records(60, 71)
    p = write_inputs(tmp_path, recs)
    (tmp_path / "x.bam").write_bytes(F.bgzf(F.bam_stream(recs), block_size=5000, extra_first=b"XY\x03\x00abc"))
    want = dump(cli, count(cli, tmp_path, "fq", ["-m", "21", "-C", p["fq"]]))
    assert want and dump(cli, count(cli, tmp_path, "x", ["-m", "21", "-C", "--sam", str(tmp_path / "x.bam")])) == want


def test_cram_and_plain_gzip_are_refused_by_name(cli, tmp_path):
    import gzip
    (tmp_path / "x.cram").write_bytes(b"CRAM\x03\x00" + b"\0" * 100)
    (tmp_path / "x.sam.gz").write_bytes(gzip.compress(F.sam_text(F.random_records(5, 1))))
    for f, word in (("x.cram", b"CRAM"), ("x.sam.gz", b"gzip")):
        r = subprocess.run([cli, "count", "-m", "21", "-s", "1M", "-o", str(tmp_path / "o.jf"), "--sam", str(tmp_path / f)], capture_output=True)
        assert r.returncode != 0 and word in r.stderr and f.encode() in r.stderr, r.stderr


def write_inputs(tmp_path, recs, refs=(("chr1", 1000000),), block_size=20000):
    paths = {}
    for name, data in (("bam", F.bgzf(F.bam_stream(recs, refs), block_size=block_size)),
                       ("sam.bgz", F.bgzf(F.sam_text(recs, refs), block_size=block_size)),
                       ("sam", F.sam_text(recs, refs)),
                       ("fq", F.fastq(recs))):
        paths[name] = str(tmp_path / ("in." + name))
        open(paths[name], "wb").write(data)
    return paths


def dump(cli, jf):
    return subprocess.check_output([cli, "dump", "-c", jf]).decode().splitlines()


def count(cli, tmp_path, tag, args, env=None):
    out = str(tmp_path / (tag + ".jf"))
    subprocess.check_call([cli, "count", "-s", "1M", "-o", out] + args, env=env, timeout=900)
    return out


@pytest.mark.parametrize("k,canon", [(15, False), (21, True), (31, True), (40, True), (100, True)])
def test_count_sam_equals_count_of_the_same_reads_as_fastq(cli, tmp_path, k, canon):
    recs = F.random_records(300, 20 + k, length=(0, 400))
    paths = write_inputs(tmp_path, recs)
    base = ["-m", str(k)] + (["-C"] if canon else [])
    want = dump(cli, count(cli, tmp_path, "fq", base + [paths["fq"]]))
    assert want
    for kind in ("bam", "sam.bgz", "sam"):
        got = dump(cli, count(cli, tmp_path, kind, base + ["--sam", paths[kind]]))
        assert got == want, kind
    # the file itself: --sam writes, byte for byte, the body `count` writes for the FASTQ ...
    mine = count(cli, tmp_path, "bam2", base + ["--matrix", "reference", "--sam", paths["bam"]])
    assert body(mine) == body(count(cli, tmp_path, "fq2", base + ["--matrix", "reference", paths["fq"]]))
    if O.have_ref() and k <= 21:
        # ... and the reference's own count of the FASTQ (the key widths whose bodies the engine matches, test_cli_gpu.py)
        ref = str(tmp_path / "ref.jf")
        subprocess.check_call([O.REF_JF, "count", "-m", str(k), "-s", "1M", "-t", "2", "-o", ref] + (["-C"] if canon else []) + [paths["fq"]])
        assert body(mine) == body(ref)


def body(jf):
    """The records of a binary .jf: what follows the length-prefixed JSON header."""
    d = open(jf, "rb").read()
    return d[9 + int(d[:9]):]


@pytest.mark.parametrize("k", [21, 40])
def test_count_sam_against_the_oracle_counts(cli, tmp_path, k):
    """Independently of the engine: every (k-mer, count) of `count --sam` is the oracle's count of the FASTQ."""
    recs = F.random_records(200, 31, length=(20, 300))
    paths = write_inputs(tmp_path, recs)
    jf = count(cli, tmp_path, "bam", ["-m", str(k), "-C", "--sam", paths["bam"]])
    got = sorted(dump(cli, jf))
    keys, cnt = O.count(O.parse_file(open(paths["fq"], "rb").read()), k, True)
    want = sorted("%s %d" % (O.to_str(keys[i], k), int(cnt[i])) for i in range(len(keys)))
    assert want and got == want


@pytest.mark.parametrize("qopt", [["-Q", "+"], ["--min-quality", "10", "--quality-start", "33"]])
def test_quality_mask_missing_qualities_and_odd_bases(cli, tmp_path, qopt):
    rng = random.Random(3)
    recs = []
    for i in range(300):
        L = rng.choice([0, 30, 150, 151])
        seq = "".join(rng.choice("ACGTacgt" * 12 + "=NRYKM") for _ in range(L))
        qual = None if i % 7 == 0 else [30 if rng.random() < 0.9 else rng.choice([0, 5, 9, 10, 11, 93, 94, 95, 120, 200, 254]) for _ in range(L)]
        recs.append(F.Record("q%d" % i, seq, qual))
    mq = ord("+") if qopt[0] == "-Q" else 33 + 10
    paths = write_inputs(tmp_path, recs)
    fa = str(tmp_path / "masked.fa")
    open(fa, "wb").write(F.fasta(recs, mq))
    want = dump(cli, count(cli, tmp_path, "fa", ["-m", "21", "-C", fa]))
    assert want
    for kind in ("bam", "sam.bgz", "sam"):
        if kind != "bam" and any(q is not None and max(q, default=0) > 93 for q in (r.qual for r in recs)):
            continue                                              # SAM text cannot carry qualities above '~'
        got = dump(cli, count(cli, tmp_path, kind, ["-m", "21", "-C"] + qopt + ["--sam", paths[kind]]))
        assert got == want, kind
    # SAM text with printable qualities only
    recs2 = [F.Record(r.name, r.seq, None if r.qual is None else [min(q, 93) for q in r.qual]) for r in recs]
    paths = write_inputs(tmp_path, recs2)
    open(fa, "wb").write(F.fasta(recs2, mq))
    want = dump(cli, count(cli, tmp_path, "fa2", ["-m", "21", "-C", fa]))
    for kind in ("bam", "sam.bgz", "sam"):
        assert dump(cli, count(cli, tmp_path, kind + "2", ["-m", "21", "-C"] + qopt + ["--sam", paths[kind]])) == want, kind


def test_count_sam_with_other_options(cli, tmp_path):
    recs = F.random_records(400, 41, length=(50, 200))
    paths = write_inputs(tmp_path, recs)
    fq = paths["fq"]
    # --text, -L / -U, small chunks, several --sam files after a positional file
    env = dict(os.environ, JFGPU_PARSE_CHUNK="5000")
    a = count(cli, tmp_path, "a", ["-m", "21", "-C", "--text", "-L", "2", "-U", "5", fq, "--sam", paths["bam"], "--sam", paths["sam"]], env=env)
    b = count(cli, tmp_path, "b", ["-m", "21", "-C", "--text", "-L", "2", "-U", "5", fq, fq, fq])
    assert sorted(body(a).splitlines()) == sorted(body(b).splitlines()) != []
    # --bf-size (one-pass Bloom filter), --digest, --timing
    a = count(cli, tmp_path, "c", ["-m", "21", "-C", "--bf-size", "1M", "--digest", str(tmp_path / "d1"), "--timing", str(tmp_path / "t"), "--sam", paths["bam"]])
    b = count(cli, tmp_path, "d", ["-m", "21", "-C", "--bf-size", "1M", "--digest", str(tmp_path / "d2"), fq])
    assert dump(cli, a) == dump(cli, b)
    assert open(tmp_path / "d1").read() == open(tmp_path / "d2").read()
    assert open(tmp_path / "t").read().split()[0::2] == ["Init", "Counting", "Writing"]


def test_count_sam_on_two_ranks(cli, tmp_path):
    recs = F.random_records(300, 51)
    recs2 = F.random_records(200, 52, name_prefix="t")
    p1 = write_inputs(tmp_path, recs)
    d = tmp_path / "two"; d.mkdir()
    p2 = write_inputs(d, recs2)
    env = dict(os.environ, JFGPU_COMM_TRANSPORT="ipc", JFGPU_PARSE_CHUNK="20000", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    out = str(tmp_path / "g2.jf")
    subprocess.check_call([cli, "count", "-m", "21", "-C", "-s", "1M", "-o", out, "--gpus", "2", "--sam", p1["bam"], "--sam", p2["bam"]], env=env, timeout=900)
    want = count(cli, tmp_path, "one", ["-m", "21", "-C", p1["fq"], p2["fq"]])
    assert dump(cli, out) == dump(cli, want)


def test_sam_alone_is_enough_input_and_listed_in_help(cli, tmp_path):
    h = subprocess.check_output([cli, "count", "-h"]).decode()
    assert "--sam" in h
    recs = F.random_records(20, 61)
    p = write_inputs(tmp_path, recs)
    out = count(cli, tmp_path, "x", ["-m", "25", "--sam", p["bam"]])
    assert dump(cli, out) == dump(cli, count(cli, tmp_path, "y", ["-m", "25", p["fq"]]))
