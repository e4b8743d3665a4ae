"""SAM / BGZF SAM / BAM fixtures for the `count --sam` tests, with the standard library only (zlib, struct).

A Record is what htslib's bam1_t holds for the counting: name, bases, qualities (None = missing, BAM 0xFF / SAM '*'),
and the fields the decoder must step over (flag, positions, CIGAR, aux).  The writers produce the same records as SAM
text, BAM, BGZF-compressed SAM, and the FASTQ / FASTA that `count` should see the same k-mers in:

  * bam_stream(records, refs)          uncompressed BAM (magic, header text, references, records)
  * sam_text(records, refs)            SAM text (@HD / @SQ header lines, 11 columns + aux)
  * bgzf(data, block_size, variants)   BGZF members of at most block_size input bytes each, the deflate variant of
                                       member i is variants[i % len(variants)] (VARIANTS), optional empty members
                                       at given member indices, the EOF marker at the end
  * fastq(records) / fasta(records, min_qual)   the equivalent sequence files (fasta applies the quality mask)
"""
import random
import struct
import zlib

NT16 = "=ACMGRSVTWYHKDBN"                       # htslib's 4-bit codes
# deflate variants: (level, strategy)
VARIANTS = {
    "stored": (0, zlib.Z_DEFAULT_STRATEGY),
    "fixed": (6, zlib.Z_FIXED),
    "huffman": (6, zlib.Z_HUFFMAN_ONLY),
    "rle": (6, zlib.Z_RLE),
    "default": (6, zlib.Z_DEFAULT_STRATEGY),
    "best": (9, zlib.Z_DEFAULT_STRATEGY),
}
EOF_MARKER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


class Record:
    def __init__(self, name, seq, qual=None, flag=4, ref=-1, pos=-1, mapq=0, cigar=(), next_ref=-1, next_pos=-1, tlen=0, aux=b""):
        self.name, self.seq, self.qual, self.flag = name, seq, qual, flag
        self.ref, self.pos, self.mapq, self.cigar = ref, pos, mapq, list(cigar)
        self.next_ref, self.next_pos, self.tlen, self.aux = next_ref, next_pos, tlen, aux

    def codes(self):
        return [NT16.find(c.upper()) if c.upper() in NT16 else 15 for c in self.seq]

    def bases(self):
        """What the decoder gives: 1 A, 2 C, 4 G, 8 T, anything else N."""
        m = {1: "A", 2: "C", 4: "G", 8: "T"}
        return "".join(m.get(c, "N") for c in self.codes())

    def masked(self, min_qual):
        """bases() with the quality mask of count -Q: (char)(q + '!') compared as a signed char."""
        b = self.bases()
        if not min_qual:
            return b
        qs = self.qual if self.qual is not None else [0xFF] * len(b)
        out = []
        for base, q in zip(b, qs):
            c = (q + 33) & 0xFF
            c = c - 256 if c > 127 else c
            out.append(base if c >= min_qual else "N")
        return "".join(out)


def random_records(n, seed, length=150, name_prefix="r", qual_lo=2, qual_hi=41):
    rng = random.Random(seed)
    recs = []
    for i in range(n):
        L = length if isinstance(length, int) else rng.randint(*length)
        seq = "".join(rng.choice("ACGT") for _ in range(L))
        qual = [rng.randint(qual_lo, qual_hi) for _ in range(L)]
        recs.append(Record("%s%d" % (name_prefix, i), seq, qual, flag=rng.choice([0, 4, 16, 256, 1024, 2048])))
    return recs


def _record_bytes(r):
    name = r.name.encode() + b"\0"
    codes = r.codes()
    seq = bytearray((len(codes) + 1) // 2)
    for i, c in enumerate(codes):
        seq[i // 2] |= c << (4 if i % 2 == 0 else 0)
    qual = bytes(r.qual) if r.qual is not None else b"\xff" * len(codes)
    cigar = b"".join(struct.pack("<I", (n << 4) | op) for n, op in r.cigar)
    fixed = struct.pack("<iiBBHHHiiii", r.ref, r.pos, len(name), r.mapq, 4680, len(r.cigar), r.flag, len(codes), r.next_ref, r.next_pos, r.tlen)
    block = fixed + name + cigar + bytes(seq) + qual + r.aux
    return struct.pack("<i", len(block)) + block


def bam_header(refs, text=b"@HD\tVN:1.6\tSO:unsorted\n"):
    h = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, length in refs:
        nb = name.encode() + b"\0"
        h += struct.pack("<i", len(nb)) + nb + struct.pack("<i", length)
    return h


def bam_stream(records, refs=(("chr1", 1000000),), text=None):
    hdr = bam_header(refs) if text is None else bam_header(refs, text)
    return hdr + b"".join(_record_bytes(r) for r in records)


def sam_text(records, refs=(("chr1", 1000000),)):
    lines = ["@HD\tVN:1.6\tSO:unsorted"] + ["@SQ\tSN:%s\tLN:%d" % (n, l) for n, l in refs]
    for r in records:
        seq = r.seq if r.seq else "*"
        qual = "".join(chr(q + 33) for q in r.qual) if (r.qual is not None and r.seq) else "*"
        rname = refs[r.ref][0] if r.ref >= 0 else "*"
        cig = "".join("%d%s" % (n, "MIDNSHP=X"[op]) for n, op in r.cigar) or "*"
        lines.append("\t".join([r.name, str(r.flag), rname, str(r.pos + 1), str(r.mapq), cig, "*", "0", "0", seq, qual]))
    return ("\n".join(lines) + "\n").encode()


def deflate(data, variant):
    level, strategy = VARIANTS[variant]
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(data) + c.flush()


def bgzf_member(data, variant="default", extra_first=b"", cdata=None, crc32=None, isize=None, oversize=False):
    """One BGZF member; extra_first: gzip extra subfields (SI1 SI2 LEN data) placed before the 'BC' one.

    cdata: ready-made deflate bytes to wrap instead of compressing data (data may then be None when crc32 and isize are
    given); crc32 / isize: the trailer's fields when they are not to be those of data; oversize: let the member be longer
    than BSIZE can say (the field wraps: such a member is only reachable through a caller's own block table)."""
    if cdata is None:
        assert len(data) <= 65536
        cdata = deflate(data, variant)
    if crc32 is None:
        crc32 = zlib.crc32(data) & 0xFFFFFFFF
    if isize is None:
        isize = len(data)
    bsize = 18 + len(extra_first) + len(cdata) + 8
    assert oversize or bsize <= 65536, "member does not fit BGZF: use a smaller block size with this variant"
    head = b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", 6 + len(extra_first)) + extra_first + b"BC" + struct.pack("<HH", 2, (bsize - 1) & 0xFFFF)
    return head + cdata + struct.pack("<II", crc32 & 0xFFFFFFFF, isize & 0xFFFFFFFF)


def bgzf(data, block_size=65280, variants=("default",), empty_at=(), eof=True, cuts=None, extra_first=b""):
    """BGZF of data: members of block_size input bytes (or cut exactly at the offsets `cuts`)."""
    bounds = sorted(set([0, len(data)] + list(cuts))) if cuts is not None else list(range(0, len(data), block_size)) + [len(data)]
    pieces = [data[a:b] for a, b in zip(bounds, bounds[1:]) if b > a]
    out, empty_at = [], set(empty_at)
    for i, p in enumerate(pieces):
        if i in empty_at:
            out.append(bgzf_member(b"", "default"))
        out.append(bgzf_member(p, variants[i % len(variants)], extra_first))
    if eof:
        out.append(EOF_MARKER)
    return b"".join(out)


def record_offsets(records, refs=(("chr1", 1000000),)):
    """Offsets of the records in bam_stream(records, refs) (the serial walk)."""
    off, res = len(bam_header(refs)), []
    for r in records:
        res.append(off)
        off += len(_record_bytes(r))
    return res


def fastq(records):
    out = []
    for r in records:
        b = r.bases()
        q = "".join(chr(min(q, 93) + 33) for q in r.qual) if r.qual is not None else "!" * len(b)
        out.append("@%s\n%s\n+\n%s\n" % (r.name, b, q))
    return "".join(out).encode()


def fasta(records, min_qual=0):
    return "".join(">%s\n%s\n" % (r.name, r.masked(min_qual)) for r in records).encode()


def contract(records, min_qual=0):
    """The contract buffer the device decode emits: every record's bases, then 'N'."""
    return "".join(r.masked(min_qual) + "N" for r in records).encode()
