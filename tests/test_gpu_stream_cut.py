"""stream_cut_kernel (kernels_stream.hip.hpp) through jfgpu_parser_stream_cut: where the inflated text of a bgzip-compressed
FASTA / FASTQ file may be cut into chunks for the parse kernels.  -m gpu only; tests/test_bgzf_seq_emu.py runs this module
on the host emulation.

Every text is compressed (tests/sam_fixtures.py: bgzf), uploaded, inflated on the device, and the cut the kernel reports is
compared with `serial_cut`, the rule of the issue restated in a few lines of Python:

  FASTA  1 + the position of the last '\\n'
  FASTQ  the largest s with 0 < s < len, S[s-1] == '\\n', S[s] == '@' and, e1 the first '\\n' at or after s, e2 the first
         one after e1: e2 + 1 < len and S[e2+1] == '+'
  0 when there is no such place.

Each text is also cut short, before compressing, at lengths inside its last two records (every length where they are short,
40 evenly spread ones and every line end - 1, + 0, + 1 where they are long: at most 90 prefixes a text) and at the kernel's
tile size - 1, + 0, + 1, and runs at member sizes of 1 byte for the first 64 bytes, of 4096 and of 65280.
"""
import random

import pytest

import sam_fixtures as F

pytestmark = pytest.mark.gpu


def serial_cut(S, fastq):
    if not fastq:
        return S.rfind(b"\n") + 1
    s = len(S)
    while True:
        q = S.rfind(b"\n", 0, s - 1) if s > 1 else -1           # the last '\n' before position s - 1 ... s becomes q + 1 < s
        if q < 0:
            return 0
        s = q + 1
        if s < len(S) and S[s:s + 1] == b"@":
            e1 = S.find(b"\n", s)
            e2 = S.find(b"\n", e1 + 1) if e1 >= 0 else -1
            if e2 >= 0 and e2 + 1 < len(S) and S[e2 + 1:e2 + 2] == b"+":
                return s


def tricky_fastq(eol=b"\n", n=40, length=150, seed=1):
    rng = random.Random(seed)
    out = bytearray()
    for r in range(n):
        seq = bytes(rng.choice(b"ACGT") for _ in range(length))
        first = (b"@", b"+", b"I")[r % 3]                         # quality lines starting with '@' and with '+'
        qual = first + bytes(rng.choice(b"@+IIIIFFF#5") for _ in range(length - 1))
        name = b"r%d+x@y +@" % r                                  # headers containing '+' and '@'
        plus = b"+" + name if r % 2 else b"+"                     # '+' lines that repeat the name
        out += b"@" + name + eol + seq + eol + plus + eol + qual + eol
    return bytes(out)


def long_record():
    rng = random.Random(2)
    seq = bytes(rng.choice(b"ACGT") for _ in range(300000))      # spans members and many tiles of the kernel
    return tricky_fastq(n=3, seed=5) + b"@long\n" + seq + b"\n+\n" + b"@" * 300000 + b"\n@short\nACGT\n+\n@@@@\n"


def wrapped_fasta():
    rng = random.Random(3)
    out = bytearray()
    for r in range(30):
        out += b">seq%d > @ +\n" % r
        seq = bytes(rng.choice(b"ACGTN") for _ in range(rng.choice([0, 59, 60, 61, 500])))
        for i in range(0, len(seq), 60):
            out += seq[i:i + 60] + b"\n"
    return bytes(out)


TEXTS = {
    "fastq": (tricky_fastq(), True),
    "fastq_crlf": (tricky_fastq(eol=b"\r\n"), True),
    "long_record": (long_record(), True),
    "fasta_wrapped": (wrapped_fasta(), False),
    "no_newline": (b"@" + b"ACGT@+" * 1500, True),
    "no_newline_fasta": (b">" + b"ACGT" * 2000, False),
    "one_header": (b"@only a header +\n", True),
}


def prefixes(text, tile):
    """The lengths a text is cut short at: inside its last two records, around the kernel's tile size, and whole."""
    lines = [i + 1 for i, c in enumerate(text) if c == 10]
    lens = {len(text)}
    if len(lines) > 8:
        a = lines[-9]                                             # start of the second-last record (4 lines a record)
        step = max(1, (len(text) - a) // 40)
        lens.update(range(a, len(text), step))
        lens.update(l + d for l in lines[-9:] for d in (-1, 0, 1))
    lens.update(n for n in (tile - 1, tile, tile + 1, 2 * tile, 2 * tile + 1) if n <= len(text))
    return sorted(n for n in lens if 0 < n <= len(text))


def member_cuts(n, size):
    """Member boundaries: 1-byte members for the first 64 bytes, then members of `size`."""
    return list(range(0, min(n, 64))) + list(range(64, n, size))


@pytest.fixture(scope="module")
def parser(gpu):
    p = gpu.Parser(21)
    yield p
    p.close()


@pytest.mark.parametrize("size", [4096, 65280])
@pytest.mark.parametrize("name", sorted(TEXTS))
def test_cut_equals_the_serial_rule(gpu, parser, name, size):
    text, fastq = TEXTS[name]
    fmt = gpu.PARSE_FASTQ if fastq else gpu.PARSE_FASTA
    lens = prefixes(text, gpu.STREAM_CUT_TILE)
    assert len(lens) <= 90
    seen = set()
    for n in lens:
        S = text[:n]
        z = F.bgzf(S, cuts=member_cuts(n, size), variants=("default", "stored"))
        assert parser.inflate(z) == n
        got, want = parser.stream_cut(fmt), serial_cut(S, fastq)
        assert got == want, (name, n, got, want)
        assert want == 0 or S[want - 1:want] == b"\n"
        seen.add(want)
        parser.stream_consume(n)
    if name in ("no_newline", "no_newline_fasta", "one_header"):
        assert seen == {0}
    else:
        assert len(seen) > 2 and max(seen) > 0


def test_cut_of_a_carried_tail_and_of_an_empty_stream(gpu, parser):
    """The stream after a consume (the tail moved to the other buffer) is cut like a fresh one; an empty stream has no cut."""
    assert parser.stream_cut(gpu.PARSE_FASTQ) == 0
    text = tricky_fastq(n=60, seed=9)
    n = parser.inflate(F.bgzf(text, block_size=5000))
    cut = parser.stream_cut(gpu.PARSE_FASTQ)
    assert cut == serial_cut(text, True) and 0 < cut < n
    drop = serial_cut(text[:7000], True)
    parser.stream_consume(drop)
    assert parser.stream_cut(gpu.PARSE_FASTQ) == cut - drop
    assert parser.stream_cut(gpu.PARSE_FASTA) == n - drop                  # the text ends with '\n'
    parser.stream_consume(n - drop)
    with pytest.raises(gpu.JfgpuError) as e:
        parser.stream_cut(3)
    assert e.value.code == gpu.E_INVALID
