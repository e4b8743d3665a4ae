"""`count` and `bc` on bgzip-compressed FASTA / FASTQ files (device_parser.hpp: parse_bgzf), through bin/jellyfish-amd
or JFGPU_CLI.  -m gpu only; tests/test_bgzf_seq_emu.py runs this module on the host emulation.

  1  the .jf body and the dump of `count x.fq.gz` are those of `count x.fq` (many chunks, empty members, an EOF marker in
     the middle, none at the end, no final newline), with no byte through the host parser
  2  the same with -Q, --if, bc, file parts, two ranks, and next to plain and --sam inputs
  3  what the device parser refuses goes through the general reader, with its counts and its error
  4  plain gzip, truncated and corrupt members and an incomplete last record are refused by name
"""
import gzip
import os
import re
import subprocess

import pytest

import sam_fixtures as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.environ.get("JFGPU_CLI") or os.path.join(ROOT, "bin", "jellyfish-amd")
SMALL = dict(JFGPU_PARSE_CHUNK="5000", JFGPU_FEED_TRACE="1")      # with 20000-byte members: many chunks, carried tails


@pytest.fixture(scope="module")
def cli(gpu):
    if not os.environ.get("JFGPU_CLI"):
        subprocess.check_call(["make", "-s", "cli"], cwd=ROOT)
    return CLI


def body(path):
    """The records of a binary .jf / .bc: what follows the length-prefixed JSON header."""
    d = open(path, "rb").read()
    return d[9 + int(d[:9]):]


def dump(cli, jf):
    return subprocess.check_output([cli, "dump", "-c", jf]).decode().splitlines()


def run(cli, tmp_path, tag, args, env=None, cmd="count", size="1M"):
    """-> (output path, stderr)"""
    out = str(tmp_path / (tag + (".jf" if cmd == "count" else ".bc")))
    e = dict(os.environ, **(env or {}))
    r = subprocess.run([cli, cmd, "-s", size, "-o", out] + args, env=e, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    return out, r.stderr


def trace(stderr):
    """The [feed] bgzf lines of a run as dicts."""
    return [dict((k, float(v)) for k, v in re.findall(r"(\w+)=([0-9.]+)", l)) for l in stderr.splitlines() if l.startswith("[feed] bgzf")]


def write(tmp_path, name, data):
    p = str(tmp_path / name)
    open(p, "wb").write(data)
    return p


def reads(n, seed, length=(30, 250)):
    return F.random_records(n, seed, length=length, qual_lo=0, qual_hi=41)


def fasta_wrapped(recs, width=70):
    out = bytearray()
    for r in recs:
        out += b">%s\n" % r.name.encode()
        b = r.bases().encode()
        for i in range(0, len(b), width):
            out += b[i:i + width] + b"\n"
    return bytes(out)


@pytest.mark.parametrize("fmt", ["fq", "fa"])
@pytest.mark.parametrize("k", [21, 100])
def test_compressed_equals_plain(cli, tmp_path, k, fmt):
    recs = reads(1000, 100 + k)
    text = F.fastq(recs) if fmt == "fq" else fasta_wrapped(recs)
    plain = write(tmp_path, "x." + fmt, text)
    base = ["-m", str(k), "-C"]
    want_jf, _ = run(cli, tmp_path, "plain", base + [plain])
    want, want_dump = body(want_jf), dump(cli, want_jf)
    assert want_dump
    half = text.index(b"\n", len(text) // 2) + 1
    variants = {
        "members": F.bgzf(text, block_size=20000),
        "empty_members": F.bgzf(text, block_size=20000, empty_at=(1, 2, 5)),
        "two_files": F.bgzf(text[:half], block_size=20000) + F.bgzf(text[half:], block_size=20000),   # an EOF marker inside
        "no_eof": F.bgzf(text, block_size=20000, eof=False),
        "no_newline": F.bgzf(text[:-1], block_size=20000),
    }
    for name, z in variants.items():
        gz = write(tmp_path, "%s.%s.gz" % (name, fmt), z)
        got, err = run(cli, tmp_path, name, base + [gz], env=SMALL)
        assert body(got) == want, name
        assert dump(cli, got) == want_dump, name
        tr = trace(err)
        assert len(tr) == 1 and tr[0]["fallback_bytes"] == 0 and tr[0]["compressed"] == len(z), (name, err)
        assert tr[0]["chunks"] >= 3 and tr[0]["inflated"] == len(text) - (name == "no_newline"), (name, err)
    # with the default chunk size too (one chunk)
    got, err = run(cli, tmp_path, "one_chunk", base + [str(tmp_path / ("members.%s.gz" % fmt))], env=dict(JFGPU_FEED_TRACE="1"))
    assert body(got) == want and trace(err)[0]["fallback_bytes"] == 0


def test_same_input_other_options(cli, tmp_path):
    recs, recs2 = reads(500, 7), reads(300, 8)
    fq, fq2 = F.fastq(recs), F.fastq(recs2)
    p1, p2 = write(tmp_path, "a.fq", fq), write(tmp_path, "b.fq", fq2)
    z1, z2 = write(tmp_path, "a.fq.gz", F.bgzf(fq, block_size=20000)), write(tmp_path, "b.fq.gz", F.bgzf(fq2, block_size=20000))
    base = ["-m", "21", "-C"]

    def same(tag, plain_args, gz_args, env=None, cmd="count", size="1M"):
        a, _ = run(cli, tmp_path, tag + "_plain", plain_args, cmd=cmd, size=size)
        b, err = run(cli, tmp_path, tag + "_gz", gz_args, env=dict(SMALL, **(env or {})), cmd=cmd, size=size)
        assert body(a) == body(b) and len(body(a)) > 0, tag
        assert all(t["fallback_bytes"] == 0 for t in trace(err)) and trace(err), tag
        return a, b

    same("Q", base + ["-Q", "$", p1], base + ["-Q", "$", z1])
    a, b = same("if", base + ["--if", p2, p1, p2], base + ["--if", z2, z1, p2])
    assert dump(cli, a) == dump(cli, b) != []
    same("bc", base + [p1, p2], base + [z1, z2], cmd="bc")
    # file parts: the j-th compressed file is read whole by part j mod 3, the plain file is cut in three
    same("parts", base + [p1, p2, p1], base + [z1, p2, z2.replace("b.fq.gz", "a.fq.gz")], env=dict(JFGPU_TEST_PARTS="3"))
    same("parts2", base + [p1, p2], base + [z1, z2], env=dict(JFGPU_TEST_PARTS="3"))
    # plain, compressed and --sam inputs in one command
    bam = write(tmp_path, "c.bam", F.bgzf(F.bam_stream(recs2), block_size=20000))
    same("mixed", base + [p1, p1, p2], base + [p1, z1, "--sam", bam])


def test_compressed_files_on_two_ranks(cli, tmp_path):
    recs, recs2 = reads(400, 17), reads(300, 18)
    fq, fq2 = F.fastq(recs), F.fastq(recs2)
    p1, p2 = write(tmp_path, "a.fq", fq), write(tmp_path, "b.fq", fq2)
    z1, z2 = write(tmp_path, "a.fq.gz", F.bgzf(fq, block_size=20000)), write(tmp_path, "b.fq.gz", F.bgzf(fq2, block_size=20000))
    env = dict(JFGPU_COMM_TRANSPORT="ipc", JFGPU_PARSE_CHUNK="20000", HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    got, _ = run(cli, tmp_path, "g2", ["-m", "21", "-C", "--gpus", "2", z1, p1, z2], env=env)
    want, _ = run(cli, tmp_path, "one", ["-m", "21", "-C", p1, p1, p2])
    assert dump(cli, got) == dump(cli, want) != []


def wrapped_fastq(recs, width=60):
    out = bytearray()
    for r in recs:
        b = r.bases().encode()
        q = "".join(chr(min(x, 93) + 33) for x in r.qual).encode()
        out += b"@%s\n" % r.name.encode()
        for i in range(0, len(b), width):
            out += b[i:i + width] + b"\n"
        out += b"+\n"
        for i in range(0, len(q), width):
            out += q[i:i + width] + b"\n"
    return bytes(out)


def test_fallback_to_the_general_reader(cli, tmp_path):
    recs = reads(400, 27, length=(100, 250))
    base = ["-m", "21", "-C"]
    # strict records first, wrapped ones after: the device parser takes the chunks it can, the rest is read back
    for name, text in (("wrapped", wrapped_fastq(recs)), ("late", F.fastq(recs[:300]) + wrapped_fastq(recs[300:]))):
        plain = write(tmp_path, name + ".fq", text)
        gz = write(tmp_path, name + ".fq.gz", F.bgzf(text, block_size=20000))
        a, _ = run(cli, tmp_path, name + "_plain", base + [plain])
        b, err = run(cli, tmp_path, name + "_gz", base + [gz], env=dict(SMALL, JFGPU_STREAM_PIECE="30000"))
        assert body(a) == body(b) and dump(cli, a) == dump(cli, b) != [], name
        tr = trace(err)
        assert 0 < tr[0]["fallback_bytes"] <= len(text), err
        if name == "late":
            assert tr[0]["fallback_bytes"] < len(text) // 2, err
    # a quality string of the wrong length: the message of the plain file
    text = F.fastq(recs[:50])
    at = text.index(b"\n+\n", len(text) // 2) + 3
    bad = text[:at] + text[at + 2:]
    msgs = []
    for name, data in (("bad.fq", bad), ("bad.fq.gz", F.bgzf(bad, block_size=5000))):
        out = str(tmp_path / "bad.jf")
        r = subprocess.run([cli, "count", "-s", "1M", "-o", out] + base + [write(tmp_path, name, data)], capture_output=True, text=True)
        assert r.returncode != 0 and "Invalid fastq sequence" in r.stderr, r.stderr
        msgs.append(r.stderr.strip().splitlines()[-1])
    assert msgs[0] in msgs[1] and "bad.fq.gz" in msgs[1]


def test_refusals(cli, tmp_path):
    recs = reads(200, 37)
    text = F.fastq(recs)
    z = F.bgzf(text, block_size=20000)
    blocks_at = [0]                                                         # where the members start
    for a in range(0, len(text), 20000):
        blocks_at.append(blocks_at[-1] + len(F.bgzf_member(text[a:a + 20000])))
    assert blocks_at[-1] + len(F.EOF_MARKER) == len(z)
    crc = bytearray(z); crc[blocks_at[2] - 8] ^= 0x01                       # the CRC32 of the second member
    last = text.rindex(b"\n@")
    cases = {
        "plain.fq.gz": (gzip.compress(text), ["gzip", "BGZF", "bgzip"]),
        "cut.fq.gz": (z[:blocks_at[2] + 500], ["truncated", "byte %d" % blocks_at[2]]),
        "crc.fq.gz": (bytes(crc), ["CRC32", "byte"]),
        "header_only.fq.gz": (F.bgzf(text[:last + 8], block_size=20000), ["incomplete", "byte"]),
        "no_plus.fq.gz": (F.bgzf(text[:last + 40], block_size=20000), ["incomplete", "byte"]),
        "short_quality.fq.gz": (F.bgzf(text[:-20], block_size=20000), ["Invalid fastq sequence"]),
    }
    for cmd, ext in (("count", ".jf"), ("bc", ".bc")):
        for name, (data, words) in cases.items():
            if cmd == "bc" and name not in ("plain.fq.gz", "crc.fq.gz", "no_plus.fq.gz"):
                continue                                              # (the feed is the same: a selection)
            out = str(tmp_path / ("refused" + ext))
            if os.path.exists(out):
                os.remove(out)
            r = subprocess.run([cli, cmd, "-m", "21", "-s", "1M", "-o", out, write(tmp_path, name, data)], capture_output=True, text=True,
                               env=dict(os.environ, JFGPU_PARSE_CHUNK="5000"))
            assert r.returncode != 0, (cmd, name)
            assert name in r.stderr and all(w in r.stderr for w in words), (cmd, name, r.stderr)
            # no output file that looks complete: none at all, or a header with no records behind it
            assert not os.path.exists(out) or os.path.getsize(out) == 0 or len(body(out)) == 0, (cmd, name)


def test_help_says_what_is_read(cli):
    for cmd in ("count", "bc"):
        h = subprocess.check_output([cli, cmd, "-h"]).decode()
        assert "bgzip" in h and "plain gzip" in h
