"""Serial models of the device parser's contract and a corpus of hand-built FASTA / FASTQ chunks -- TEST INFRASTRUCTURE.

The models restate, with unbounded loops, the per-byte rules in the header of jellyfish_amd/csrc/kernels_parse.hip.hpp
and the strict FASTQ layout of jellyfish_amd/csrc/abi_parser.inl.  The corpus puts every mechanism of the five parse
kernels at the seams where they carry state: the lane (16 bytes a thread), the tile (4096 bytes a workgroup) and the scan
(above 1024 tiles one thread of the scan workgroup walks several tiles).  No file is read: everything is a literal or
comes from a seeded generator.

Used by tests/test_parse_fixtures.py (models against the oracle and the host reader, CPU) and
tests/test_gpu_parse_conformance.py (device against the models).

Outside the corpus on purpose: a FASTQ sequence or quality line that BEGINS with '\\r', and a '\\r' inside a quality
line.  The device drops leading '\\r's as the reference's skip_newlines does, while the record check and the quality
mask count raw line bytes; the strict layout gives such lines no meaning."""
import random
import re

LANE = 16
TILE = 4096
SCAN = 1024                      # tiles one pass of the scan workgroup covers with one tile a thread
SEAMS = (LANE, TILE, 2 * TILE)
REFUSE = "refuse"                # what model_fastq returns for a chunk outside the strict layout

NL, CR, GT = 10, 13, 62
_SPECIAL = re.compile(rb"[\n\r>]")


# ---- the models ------------------------------------------------------------------------------------------------------
def fasta_model(data: bytes):
    """-> (contract bytes, number of headers).  Per byte: a '>' that starts the chunk or follows a '\\n' (any number of
    '\\r' between) opens a header and emits one 'N'; the header ends at the next '\\n'; '\\n' is dropped; outside a header
    a '\\r' is dropped when its run of '\\r' reaches a '\\n' or the end of the chunk on the right, or a '\\n' or the start
    of the chunk on the left; every other byte is kept."""
    out = bytearray()
    n, i, records = len(data), 0, 0
    while i < n:
        m = _SPECIAL.search(data, i)            # bytes that are none of '\n' '\r' '>' are kept as they are
        if m is None:
            out += data[i:]
            break
        out += data[i:m.start()]
        i = m.start()
        c = data[i]
        if c == NL:
            i += 1
        elif c == GT:
            j = i - 1
            while j >= 0 and data[j] == CR:
                j -= 1
            if j < 0 or data[j] == NL:
                out.append(ord("N"))
                records += 1
                e = data.find(b"\n", i)
                i = n if e < 0 else e + 1         # the header, its '\n' included
            else:
                out.append(c)
                i += 1
        else:                                     # a whole run of '\r' at once: data[i - 1], if any, is not '\r'
            j = i
            while j < n and data[j] == CR:
                j += 1
            dropped = j >= n or data[j] == NL or i == 0 or data[i - 1] == NL
            if not dropped:
                out += data[i:j]
            i = j
    return bytes(out), records


def model_fasta(data: bytes) -> bytes:
    return fasta_model(data)[0]


def fastq_lines(data: bytes):
    """The lines of a chunk the way abi_parser.inl counts them: a last line without '\\n' counts, and so does an empty
    last quality line (newline count 4r + 3 at the end of the chunk)."""
    parts = data.split(b"\n")
    if parts[-1] == b"" and data.count(b"\n") % 4 != 3:
        parts.pop()
    return parts


def model_fastq(data: bytes, min_qual: int = 0):
    """Strict four-line records -> 'N' + the sequence line without its trailing '\\r's for every record, a base whose
    quality byte is < min_qual turned into 'N'; REFUSE for anything else."""
    if not data:
        return b""
    lines = fastq_lines(data)
    if len(lines) % 4:
        return REFUSE
    out = bytearray()
    for r in range(0, len(lines), 4):
        head, seq, plus, qual = lines[r:r + 4]
        if head[:1] != b"@" or plus[:1] != b"+":
            return REFUSE
        seq, qual = seq.rstrip(b"\r"), qual.rstrip(b"\r")
        if len(seq) != len(qual):
            return REFUSE
        out.append(ord("N"))
        if min_qual:
            seq = bytes(ord("N") if q < min_qual else s for s, q in zip(seq, qual))
        out += seq
    return bytes(out)


def fastq_records(data: bytes) -> int:
    return len(fastq_lines(data)) // 4 if data else 0


def short_lines_limit(data: bytes) -> int:
    """The device parses a FASTQ chunk with at most this many '\\n'; above it, it may hand the chunk to the host reader."""
    return len(data) // 8 + 16


def oracle_input(fmt: str, data: bytes) -> bytes:
    """The oracle restates a FILE reader: the first byte names the format.  A FASTA chunk from the middle of a file is
    given to it behind an empty header line: the '\\n' in front stands for the start of the chunk, which the rules above
    treat alike, and the extra record adds nothing but a leading 'N', which every comparison strips."""
    if fmt == "fa" and data[:1] != b">":
        return b">\n" + data
    return data


# ---- seeded material -------------------------------------------------------------------------------------------------
def _pool(seed, alphabet, n=1 << 16):
    rng = random.Random(seed)
    return bytes(rng.choice(alphabet) for _ in range(n))


_BASES = _pool(11, b"ACGTACGTACGTacgtNnR")
_PLAIN = _pool(12, b"ACGT")
_QUALS = _pool(13, bytes(range(ord("!"), ord("~") + 1)))


def _take(pool, rng, n):
    a = rng.randrange(len(pool) - n)
    return pool[a:a + n]


def bases(n, seed=0):
    return bytes(_PLAIN[(seed * 7919 + i) % len(_PLAIN)] for i in range(n)) if n < 64 else _take(_PLAIN, random.Random(seed * 31 + n), n)


def quals(n, seed=0):
    return bytes(_QUALS[(seed * 104729 + i) % len(_QUALS)] for i in range(n)) if n < 64 else _take(_QUALS, random.Random(seed * 37 + n), n)


def fq(seq, qual=None, eol=b"\n", name=b"r", plus=b"+", final=True):
    qual = quals(len(seq), len(seq)) if qual is None else qual
    rec = b"@" + name + eol + seq + eol + plus + eol + qual
    return rec + eol if final else rec


def span_fasta(target, eol, final, seed):
    """Records of 0 to 400 bases in lines of width 1, 7, 60 or unwrapped; exactly `target` bytes."""
    rng = random.Random(seed)
    out, size, r = [], 0, 0
    while target - size > 2500:
        ln = rng.randrange(401)
        seq = _take(_BASES, rng, ln)
        w = rng.choice((1, 7, 60, 1 << 20))
        rec = b">r%d some > text" % r + eol + b"".join(seq[i:i + w] + eol for i in range(0, ln, w))
        if rng.random() < 0.05:
            rec += eol                                   # a blank line
        out.append(rec); size += len(rec); r += 1
    left = target - size                                 # the last record's header takes up the slack
    tail = len(eol) * (2 if final else 1)
    name = b"x" * (left - 1 - 200 - tail)
    out.append(b">" + name + eol + _take(_BASES, rng, 200) + (eol if final else b""))
    data = b"".join(out)
    assert len(data) == target
    return data


def span_fastq_records(target, eol, seed):
    rng = random.Random(seed)
    out, size, r = [], 0, 0
    while target - size > 1000:
        ln = rng.randrange(251)
        rec = fq(_take(_PLAIN, rng, ln), _take(_QUALS, rng, ln), eol, name=b"r%d" % r, plus=b"+" if r & 1 else b"+r%d" % r)
        out.append(rec); size += len(rec); r += 1
    return out, size


def span_fastq(target, eol, final, seed):
    """Records of 0 to 250 bases; exactly `target` bytes."""
    out, size = span_fastq_records(target, eol, seed)
    left = target - size
    name = b"x" * (left - 2 - 200 - len(eol) * (4 if final else 3))
    out.append(fq(bases(100, seed), quals(100, seed), eol, name=name, final=final))
    data = b"".join(out)
    assert len(data) == target
    return data


def span_fastq_bad(target, where, seed):
    """The same with one record whose quality line is one byte short: `where` is a byte offset the record lies behind."""
    out, _ = span_fastq_records(target, b"\n", seed)
    at, i = 0, 0
    while at < where or out[i].split(b"\n")[1] == b"":
        at += len(out[i]); i += 1
    head, seq, plus, qual = out[i].split(b"\n")[:4]
    out[i] = b"\n".join((head, seq, plus, qual[:-1])) + b"\n"
    return b"".join(out), at


# ---- the corpus ------------------------------------------------------------------------------------------------------
_cache = None


def cases():
    """[(id, fmt, data, expect)]: fmt 'fa' or 'fq'; expect 'accept', 'refuse' or 'short_lines'.  Built once."""
    global _cache
    if _cache is None:
        _cache = list(_build())
        ids = [c[0] for c in _cache]
        assert len(ids) == len(set(ids))
    return _cache


def family(case_id):
    return case_id.split("-")[0]


def _name(pattern):
    return "".join({"\n": "n", "\r": "r", ">": "gt"}.get(ch, ch) for ch in pattern.decode())


def _build():
    # -- seam: each byte of a pattern in turn is the first byte after a lane / tile boundary
    for pat in (b"\n>", b"\r\n>", b"\n\r>", b"\r\r\n", b"A\rC", b"A>C", b"\n\n"):
        for B in SEAMS:
            for j in range(len(pat)):
                head = b">s\n"
                data = head + bases(B - j - len(head), B + j) + pat + b"x y\nGATTACA\r\n>t\nCC\n"
                assert data[B] == pat[j]
                yield "seam-fa-%s-B%d-%d" % (_name(pat), B, j), "fa", data, "accept"
    # the same as FASTQ line ends: after the sequence line (then '+') and after the quality line (then '@'), and a
    # lone '\r' inside the sequence
    for eol in (b"\n", b"\r\n", b"\r\r\n"):
        for B in SEAMS:
            for j in range(len(eol) + 1):
                ln = B - j - 3                                              # "@q\n" + sequence, then eol at B - j
                data = fq(bases(ln, B), None, eol, name=b"q") [len(b"@q") + len(eol):]
                data = b"@q\n" + data + fq(b"GATTACA", None, eol, name=b"t")
                assert data[B - j:B - j + len(eol) + 1] == eol + b"+"
                yield "seam-fq-seq-%s-B%d-%d" % (_name(eol), B, j), "fq", data, "accept"
                ln = (B - j - 3 - 2 - 2 * len(eol)) // 2                    # "@q\n" seq eol "+" pad eol qual, then eol at B - j
                pad = B - j - 3 - 1 - 2 * len(eol) - 2 * ln
                data = b"@q\n" + bases(ln, B) + eol + b"+" + b"p" * pad + eol + quals(ln, B) + eol + fq(b"GATTACA", None, eol, name=b"t")
                assert data[B - j:B - j + len(eol) + 1] == eol + b"@"
                yield "seam-fq-qual-%s-B%d-%d" % (_name(eol), B, j), "fq", data, "accept"
    for B in SEAMS:
        for j in range(3):
            ln = B - j - 3
            seq = bases(ln, B) + b"A\rC" + bases(5, j)
            data = fq(seq, None, b"\n", name=b"q") + fq(b"GG", None, b"\n", name=b"t")
            assert data[B] == b"A\rC"[j]
            yield "seam-fq-ArC-B%d-%d" % (B, j), "fq", data, "accept"

    # -- header: a tile with no event that is entered inside a header keeps nothing
    text = b"ACGT>\r desc "
    for H in list(range(4090, 4101)) + [8192, 12289]:
        header = b">" + (text * (H // len(text) + 1))[:H - 1]
        yield "header-len%d" % H, "fa", b">a\nACGT\n" + header + b"\nGGCC\n>c\nTT\n", "accept"
    pre = b">a\n" + b"".join(bases(60, i) + b"\n" for i in range(80))
    pre = pre[:TILE - 1] + b"\n"
    yield "header-one-tile-aligned", "fa", pre + b">" + (text * 400)[:TILE - 2] + b"\nGGCC\n", "accept"
    yield "header-three-tiles-aligned", "fa", pre + b">" + (text * 1100)[:3 * TILE - 2] + b"\nGGCC\n", "accept"
    yield "header-last-line-no-newline", "fa", b">a\nACGT\n>tail without newline", "accept"
    yield "header-last-line-long-no-newline", "fa", b">a\nACGT\n>" + (text * 800)[:9000], "accept"
    yield "header-only-headers", "fa", b">a\n>b\n>c\n", "accept"
    yield "header-only-long-headers", "fa", b"".join(b">" + (text * 500)[:n] + b"\n" for n in (4095, 4096, 5000, 3)), "accept"
    yield "header-empty-records", "fa", b">a\n>b\n\n>c\nAC\n>d\n\r\n>e\r\nGT\n>f", "accept"

    # -- runs of '\r' of every length around the old bound of 64, at each place a run can stand, once near the start of
    #    the chunk and once across a tile boundary
    places = {
        "before-nl": (b">a\nACGT", b"\nGG\n"),
        "nl-to-gt": (b">a\nACGT\n", b">b\nGG\n"),
        "nl-to-seq": (b">a\nACGT\n", b"GG\n"),
        "chunk-end": (b">a\nACGT", b""),
        "chunk-start": (b"", b"ACGT\n>b\nGG\n"),
        "mid-line": (b">a\nACGT", b"GG\n"),
    }
    for R in (1, 2, 15, 16, 17, 63, 64, 65, 200, 5000):
        for place, (left, right) in places.items():
            yield "cr-%s-%d" % (place, R), "fa", left + b"\r" * R + right, "accept"
            if left:
                start = TILE - R // 2 if R < 2 * TILE else TILE // 2          # the run's first byte
                fill = start - len(left)
                data = left[:3] + bases(fill, R) + left[3:] + b"\r" * R + right
                assert data[start - 1] != CR and data[start] == CR and start <= TILE < start + max(R, 2) + 1
                yield "cr-%s-%d-tile" % (place, R), "fa", data, "accept"
    yield "cr-64k-after-header", "fa", b">a\n" + b"\r" * 65536, "accept"
    yield "cr-64k-mid-line", "fa", b">a\nAC" + b"\r" * 65536 + b"GT\n", "accept"
    for R in (2, 63, 64, 65, 200, 5000):
        eol = b"\r" * R + b"\n"
        yield "cr-fq-line-ends-%d" % R, "fq", fq(bases(3900, R), None, eol) + fq(b"GATTACA", None, eol), "accept"
        yield "cr-fq-chunk-end-%d" % R, "fq", fq(b"ACGT", b"IIII", b"\n", final=False) + b"\r" * R, "accept"

    # -- span: the scan walks several tiles a thread above 1024 tiles
    sizes = (("1024t", SCAN * TILE), ("1024t+1", SCAN * TILE + 1), ("2048t+", 2 * SCAN * TILE + 1234))
    for si, (label, target) in enumerate(sizes):
        for ei, eol in enumerate((b"\n", b"\r\n")):
            final = bool((si + ei) & 1)
            tag = "%s-%s-%s" % (label, _name(eol), "final" if final else "nofinal")
            yield "span-fa-" + tag, "fa", span_fasta(target, eol, final, 100 + 2 * si + ei), "accept"
            yield "span-fq-" + tag, "fq", span_fastq(target, eol, final, 200 + 2 * si + ei), "accept"
    data, at = span_fastq_bad(2 * SCAN * TILE + 1234, 1500 * TILE, 300)
    assert at >= 1500 * TILE
    yield "span-fq-bad-beyond-tile-1024", "fq", data, "refuse"
    data, at = span_fastq_bad(SCAN * TILE + 1, 0, 301)
    assert at < TILE
    yield "span-fq-bad-first-tile", "fq", data, "refuse"
    data, at = span_fastq_bad(SCAN * TILE + 1, SCAN * TILE - 2500, 302)
    assert len(data) - at < TILE
    yield "span-fq-bad-last-tile", "fq", data, "refuse"

    # -- fastq: the strict layout and its edges
    for ln in (0, 1, 15, 16, 17, 4095, 4096, 4097, 9000):
        for eol in (b"\n", b"\r\n"):
            yield "fastq-len%d-%s" % (ln, _name(eol)), "fq", fq(bases(ln, ln), None, eol) + fq(b"GATTACA", None, eol, name=b"t"), "accept"
    yield "fastq-qual-starts-with-at", "fq", fq(b"ACGT", b"@III") + fq(b"GG", b"@@"), "accept"
    yield "fastq-qual-starts-with-plus", "fq", fq(b"ACGT", b"+III") + fq(b"GG", b"++"), "accept"
    yield "fastq-plus-name", "fq", fq(b"ACGT", b"IIII", plus=b"+r extra") + fq(b"GG", b"II", plus=b"+t"), "accept"
    yield "fastq-crcrlf", "fq", fq(b"ACGT", b"IIII", b"\r\r\n") + fq(b"GG", b"II", b"\r\r\n"), "accept"
    yield "fastq-lone-cr-in-seq", "fq", fq(b"AC\rGT", b"IIIII") + fq(b"G\r\rG", b"IIII"), "accept"
    yield "fastq-lone-cr-in-seq-crlf", "fq", fq(b"AC\rGT", b"IIIII", b"\r\n") + fq(b"GG", b"II", b"\r\n"), "accept"
    yield "fastq-last-no-newline", "fq", fq(b"ACGT", b"IIII") + fq(b"GG", b"II", final=False), "accept"
    yield "fastq-last-no-newline-crlf", "fq", fq(b"ACGT", b"IIII", b"\r\n") + fq(b"GG", b"II", b"\r\n", final=False), "accept"
    yield "fastq-last-bare-cr", "fq", fq(b"ACGT", b"IIII", b"\r\n") + fq(b"GG", b"II", b"\r\n", final=False) + b"\r", "accept"
    yield "fastq-last-empty-quality-no-newline", "fq", fq(b"ACGT", b"IIII") + b"@e\n\n+\n", "accept"
    yield "fastq-only-empty-quality-no-newline", "fq", b"@e\n\n+\n", "accept"
    for i, bad in enumerate((
            b"@r\nACGT\nACGT\n+\nIIII\nIIII\n",                 # wrapped sequence
            b"@r\nACGT\n+\nIII\n",                               # short quality
            b"@r\nACGT\n+\nIIII\n\n@s\nAC\n+\nII\n",             # blank line between records
            b"@r\nACGT\n+\nIIII\n@s\nAC\n",                      # truncated last record
            b"@r\nACGT\n-\nIIII\n")):                            # no '+' line
        yield "fastq-refused-%d" % i, "fq", bad, "refuse"
    yield "fastq-quality-one-longer", "fq", fq(b"ACGT", b"IIIII") + fq(b"GG", b"II"), "refuse"
    yield "fastq-quality-one-longer-last", "fq", fq(b"GG", b"II") + fq(b"ACGT", b"IIIII", final=False), "refuse"
    yield "fastq-second-record-no-at", "fq", fq(b"ACGT", b"IIII") + b"r\nGG\n+\nII\n", "refuse"
    yield "fastq-4n+1-lines", "fq", fq(b"ACGT", b"IIII") + b"@x\n", "refuse"
    yield "fastq-4n+1-lines-no-newline", "fq", fq(b"ACGT", b"IIII") + b"@x", "refuse"
    yield "fastq-4n+2-lines", "fq", fq(b"ACGT", b"IIII") + b"@x\nAC\n", "refuse"
    yield "fastq-4n+3-lines", "fq", fq(b"ACGT", b"IIII") + b"@x\nAC\n+", "refuse"
    yield "fastq-4n+3-lines-newline", "fq", fq(b"ACGT", b"IIII") + b"@x\nAC\n+\n", "refuse"   # counts as an empty quality line

    # -- short_lines: the hand-over to the host reader at its boundary.  Four lines of L bytes a record; the first
    #    header is padded until the number of '\n' is limit - 1, limit, limit + 1.
    for L in range(1, 10):
        def chunk(R, pad):
            recs = [b"@" + b"h" * (L - 1 + (pad if r == 0 else 0)) + b"\n" + bases(L, r) + b"\n+" + b"p" * (L - 1) + b"\n" + quals(L, r) + b"\n"
                    for r in range(R)]
            return b"".join(recs)
        over = lambda d: d.count(b"\n") - short_lines_limit(d)
        if 4 * (L + 1) >= 32:                                # eight bytes a line or more: never above the limit
            yield "short_lines-L%d-below" % L, "fq", chunk(40, 0), "short_lines"
            continue
        R = 1
        while over(chunk(R, 0)) < 1:
            R += 1
        for d in (1, 0, -1):
            pad = 0
            while over(chunk(R, pad)) > d:
                pad += 1
            data = chunk(R, pad)
            assert over(data) == d
            yield "short_lines-L%d-limit%+d" % (L, d), "fq", data, "short_lines"
