"""Device-side FASTA / FASTQ parse (jfgpu_parser_*, kernels_parse.hip.hpp) on the hand-built corpus of
tests/parse_fixtures.py, judged by its serial models: every mechanism of the five parse kernels at the lane (16 bytes), the
tile (4096 bytes) and the scan (1024 tiles) seams, runs of '\\r' of any length, the quality mask at the entry point, the
seam carry at several k, the line-count hand-over at its boundary and the two-buffer promise.  -m gpu only;
tests/test_parse_conformance_emu.py runs the same module on the host emulation in the CPU suite."""
import numpy as np
import pytest

import parse_fixtures as F

pytestmark = pytest.mark.gpu

CASES = F.cases()
GOOD_FQ = b"@r\nACGT\n+\nIIII\n"


@pytest.fixture(scope="module")
def tools(gpu):
    t = gpu.Table(k=21, size=1 << 12)      # only used for raw device copies
    p = gpu.Parser(21)
    yield gpu, p, t
    p.close(); t.close()


def flag(capi, fmt):
    return capi.PARSE_FASTA if fmt == "fa" else capi.PARSE_FASTQ


def fetch(t, ptr, n):
    return bytes(t.d2h(ptr, n)) if n else b""


def dev_parse(p, t, data, flags):
    ptr, n = p.parse(data, flags)
    return fetch(t, ptr, n)


def expected(fmt, data, min_qual=0):
    if fmt == "fa":
        return F.fasta_model(data)
    return F.model_fastq(data, min_qual), F.fastq_records(data)


def check_refused(capi, p, t, data):
    with pytest.raises(capi.JfgpuError) as e:
        p.parse(data, capi.PARSE_FASTQ)
    assert e.value.code == capi.E_FORMAT
    assert dev_parse(p, t, GOOD_FQ, capi.PARSE_FASTQ) == b"NACGT" and p.records == 1     # the handle is still good


# ---- the corpus ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_corpus(tools, case):
    capi, p, t = tools
    cid, fmt, data, expect = case
    want, records = expected(fmt, data)
    if expect == "refuse":
        assert want is F.REFUSE
        check_refused(capi, p, t, data)
        return
    may_refuse = expect == "short_lines" and data.count(b"\n") > F.short_lines_limit(data)
    try:
        got = dev_parse(p, t, data, flag(capi, fmt))
    except capi.JfgpuError as e:
        assert may_refuse and e.code == capi.E_FORMAT, "refused a chunk inside the contract: %s" % e
        assert dev_parse(p, t, GOOD_FQ, capi.PARSE_FASTQ) == b"NACGT"
        return
    assert len(got) == len(want)
    assert got == want
    assert p.records == records


# ---- minimum quality at the entry point ------------------------------------------------------------------------------
def qual_file(eol, final):
    """Records of 0, 1, 63, 64, 65 and 5000 bases; every quality byte from '!' to '~' is present."""
    every = bytes(range(ord("!"), ord("~") + 1))
    recs = []
    for i, ln in enumerate((0, 1, 63, 64, 65, 5000)):
        q = F.quals(ln, 50 + i)
        if ln == 5000:
            q = every + q[len(every):-len(every)] + every[::-1]
        recs.append(F.fq(F.bases(ln, 60 + i), q, eol, name=b"q%d" % i, plus=b"+" if i & 1 else b"+q%d" % i))
    data = b"".join(recs)
    assert set(every) <= set(data)
    return data if final else data[:-len(eol)]


@pytest.mark.parametrize("final", [True, False], ids=["final", "nofinal"])
@pytest.mark.parametrize("eol", [b"\n", b"\r\n"], ids=["n", "rn"])
@pytest.mark.parametrize("threshold", [ord("I") - 1, ord("I"), ord("I") + 1, ord("!"), 126])
def test_min_quality(gpu, threshold, eol, final):
    t = gpu.Table(k=21, size=1 << 12)
    p = gpu.Parser(21)
    try:
        data = qual_file(eol, final)
        given = bytes(bytearray(data))                 # the object handed to parse; `data` is the untouched copy
        plain = F.model_fastq(data)
        masked = F.model_fastq(data, threshold)
        assert (masked != plain) == (threshold > ord("!")) and len(masked) == len(plain)
        assert dev_parse(p, t, given, gpu.PARSE_FASTQ) == plain and p.records == 6
        p.set_min_quality(threshold)
        assert dev_parse(p, t, given, gpu.PARSE_FASTQ) == masked
        assert p.records == 6                          # records are unchanged by masking
        assert dev_parse(p, t, given, gpu.PARSE_FASTQ) == masked      # ... and so is a second pass over the same bytes
        assert given == data                           # the caller's host bytes are not edited
        p.set_min_quality(0)
        assert dev_parse(p, t, given, gpu.PARSE_FASTQ) == plain and p.records == 6
    finally:
        p.close(); t.close()


# ---- the seam carry --------------------------------------------------------------------------------------------------
def carry_file():
    lines = []
    for r in range(10):
        lines.append(b">r%d some > text\n" % r)
        for i, ln in enumerate((60, 60, 0, 1, 7, 33)[: 3 + r % 4]):
            lines.append(F.bases(ln, 10 * r + i) + (b"\r\n" if r == 5 else b"\n"))
        if r % 3 == 0:
            lines.append(b"\n")
    lines.append(b">last\n")
    lines.append(b"ACGTTGCA")                      # no final newline
    return lines


@pytest.mark.parametrize("k", [1, 2, 21, 64, 127])
def test_seam_carry(gpu, k):
    """One line a chunk: chunks that yield no character (blank lines) and fewer than k - 1 (every line, at k = 127)."""
    t = gpu.Table(k=21, size=1 << 12)
    p = gpu.Parser(k)
    try:
        lines = carry_file()
        assert 50 <= len(lines) <= 70 and b"\n" in lines
        whole = dev_parse(p, t, b"".join(lines), gpu.PARSE_FASTA)
        assert whole == F.model_fasta(b"".join(lines))
        stream = b""
        for i, line in enumerate(lines):
            got = dev_parse(p, t, line, gpu.PARSE_FASTA | (gpu.PARSE_CONTINUE if i else 0))
            seam = min(k - 1, len(stream))
            assert got[:seam] == stream[len(stream) - seam:], i
            assert got[seam:] == F.model_fasta(line), i
            stream += got[seam:]
            if i % 7 == 3:                           # an empty chunk in between keeps the carry
                assert p.parse(b"", gpu.PARSE_FASTA | gpu.PARSE_CONTINUE) == (0, 0)
        assert stream == whole
        # a chunk without PARSE_CONTINUE starts fresh ...
        assert dev_parse(p, t, b"GATTACA\n", gpu.PARSE_FASTA) == b"GATTACA"
        # ... FASTQ never takes a carry and leaves none
        assert dev_parse(p, t, b"TTTT\n", gpu.PARSE_FASTA | gpu.PARSE_CONTINUE) == b"GATTACA"[7 - min(k - 1, 7):] + b"TTTT"
        assert dev_parse(p, t, GOOD_FQ, gpu.PARSE_FASTQ | gpu.PARSE_CONTINUE) == b"NACGT"
        assert dev_parse(p, t, b"CCCC\n", gpu.PARSE_FASTA | gpu.PARSE_CONTINUE) == b"CCCC"
    finally:
        p.close(); t.close()


# ---- the two output buffers ------------------------------------------------------------------------------------------
def test_output_of_a_call_outlives_the_next_call_and_a_refusal(gpu):
    t = gpu.Table(k=21, size=1 << 12)
    p = gpu.Parser(21)
    try:
        inputs = [("fa", b">a\n" + F.bases(9000, 1) + b"\n>b\nGG\n"),
                  ("fq", F.fq(F.bases(300, 2)) + F.fq(b"GG")),
                  ("fa", b">c\n" + F.bases(60000, 3) + b"\r\n"),          # larger than anything before: the buffer grows
                  ("fq", F.fq(F.bases(5000, 4), eol=b"\r\n")),
                  ("fa", b">d\nAC\n")]
        bad = b"@r\nACGT\n+\nIII\n" + F.fq(F.bases(20000, 5))
        prev = None
        for i, (fmt, data) in enumerate(inputs):
            ptr, n = p.parse(data, flag(gpu, fmt))
            want = expected(fmt, data)[0]
            assert fetch(t, ptr, n) == want, i
            if prev is not None:
                assert fetch(t, prev[0], prev[1]) == prev[2], i         # call i - 1 is intact after call i
            with pytest.raises(gpu.JfgpuError) as e:
                p.parse(bad, gpu.PARSE_FASTQ)
            assert e.value.code == gpu.E_FORMAT
            assert fetch(t, ptr, n) == want, i                          # ... and call i after a refused call
            prev = (ptr, n, want)
    finally:
        p.close(); t.close()


@pytest.mark.parametrize("off", [1, 7, 15, 17])
@pytest.mark.parametrize("fmt", ["fa", "fq"])
def test_parse_dev_at_unaligned_pointers(tools, fmt, off):
    capi, p, t = tools
    if fmt == "fa":
        data = b"".join(b">r%d x\r\n" % r + F.bases(61 * r, r) + b"\r\n" for r in range(20)) + b">e\nAC\rGT\r"
    else:
        data = b"".join(F.fq(F.bases(37 * r, r), eol=b"\r\n", name=b"r%d" % r) for r in range(20)) + F.fq(b"GG", final=False)
    assert len(data) > 2 * F.TILE
    d = t.malloc(len(data) + off + 64)
    try:
        t.h2d(d + off, np.frombuffer(data, dtype=np.uint8))
        ptr, n = p.parse_dev(d + off, len(data), flag(capi, fmt))
        want, records = expected(fmt, data)
        assert fetch(t, ptr, n) == want and p.records == records
        assert fetch(t, d + off, len(data)) == data                    # no minimum quality set: the input is only read
    finally:
        t.free(d)
