"""bgzip-compressed FASTA / FASTQ at library level: members fed in groups to jfgpu_parser_inflate_uploaded ->
_stream_cut -> _stream_parse, the pieces counted, against the uncompressed text parsed whole and the oracle's counts
(tests/oracle_lib.py).  -m gpu only; tests/test_bgzf_seq_emu.py runs this module on the host emulation.

Chunked input is judged as tests/test_gpu_parse.py::test_fasta_chunks_with_seam judges it: piece i+1 of a FASTA starts with
the last k-1 characters of the output so far, and the pieces minus those seams are the one-shot output."""
import random

import numpy as np
import pytest

import oracle_lib as O
import sam_fixtures as F

pytestmark = pytest.mark.gpu


def fasta_text():
    rng = random.Random(21)
    out = bytearray()
    for r in range(120):
        out += b">read_%d > x\n" % r
        seq = bytes(rng.choice(b"ACGTACGTACGTacgtN") for _ in range(rng.choice([0, 1, 99, 100, 150, 700])))
        w = rng.choice([60, 10 ** 9])
        for i in range(0, len(seq), w):
            out += seq[i:i + w] + b"\n"
    return bytes(out)[:-1]                                        # the file need not end in a newline


def fastq_text(min_qual=0):
    recs = F.random_records(260, 33, length=(0, 260), qual_lo=20, qual_hi=41)
    rng = random.Random(34)
    for r in recs:                                                # a few bases below any threshold: k-mers of 100 survive
        for _ in range(len(r.qual) // 120):
            r.qual[rng.randrange(len(r.qual))] = rng.choice([0, 5, 19])
    return F.fastq(recs), F.fasta(recs, min_qual)


def groups(z, capi, n_members):
    """The file as consecutive groups of n_members whole BGZF members."""
    blocks, used = capi.bgzf_scan(z)
    assert used == len(z)
    starts = [b.c_off - 18 for b in blocks] + [used]
    return [z[starts[i]:starts[min(i + n_members, len(blocks))]] for i in range(0, len(blocks), n_members)]


def feed(capi, p, t, z, n_members, fmt, k):
    """What device_sequence_parser does with a BGZF file -> the pieces' contract buffers, the records."""
    pieces, records, first = [], 0, True
    gs = groups(z, capi, n_members)
    for i, g in enumerate(gs):
        n = p.inflate(g, which=i % 2)
        cut = n if i + 1 == len(gs) else p.stream_cut(fmt)
        if not cut:
            continue                                              # no boundary yet: inflate more
        ptr, n_out, recs, left = p.stream_parse(cut, fmt | (0 if first else capi.PARSE_CONTINUE))
        assert left == n - cut
        pieces.append(bytes(t.d2h(ptr, n_out)) if n_out else b"")
        records += recs
        first = False
    return pieces, records


def join(pieces, k, fasta):
    stream = b""
    for got in pieces:
        seam = min(len(stream), k - 1) if fasta else 0
        assert got[:seam] == stream[len(stream) - seam:]
        stream += got[seam:]
    return stream


def table_counts(capi, k, pieces):
    with capi.Table(k, 1 << 16, canonical=True) as t:
        for b in pieces:
            t.count_ascii(b)
        t.sync()
        keys, cnts = capi.decode_records(t.dump_records(chunk_records=1 << 16), k, t.info.out_counter_len)
    keys = np.asarray(keys, dtype=np.uint64).reshape(len(cnts), -1)
    return {tuple(r): int(c) for r, c in zip(keys.tolist(), np.asarray(cnts).tolist())}


def oracle_counts(contract, k):
    keys, cnt = O.count(contract, k, True)
    return {tuple(r): int(c) for r, c in zip(keys.reshape(len(cnt), -1).tolist(), cnt.tolist())}


@pytest.fixture(scope="module")
def holder(gpu):
    t = gpu.Table(k=21, size=1 << 12)                             # raw device copies only
    yield t
    t.close()


@pytest.mark.parametrize("n_members", [1, 3, 1000])
@pytest.mark.parametrize("k", [21, 100])
@pytest.mark.parametrize("kind", ["fasta", "fastq", "fastq_Q"])
def test_compressed_pieces_equal_the_text_parsed_whole(gpu, holder, kind, k, n_members):
    capi = gpu
    min_qual = ord("5") if kind == "fastq_Q" else 0
    if kind == "fasta":
        text, fmt = fasta_text(), capi.PARSE_FASTA
        plain = text
    else:
        (text, plain), fmt = fastq_text(min_qual), capi.PARSE_FASTQ
    z = F.bgzf(text, block_size=3000, variants=("default", "fixed", "stored"), empty_at=(2, 3))
    p = capi.Parser(k)
    try:
        if min_qual:
            p.set_min_quality(min_qual)
        ptr, n = p.parse(text, fmt)
        whole, whole_records = bytes(holder.d2h(ptr, n)), p.records
        pieces, records = feed(capi, p, holder, z, n_members, fmt, k)
        assert len(pieces) > (1 if n_members < 1000 else 0)
        stream = join(pieces, k, kind == "fasta")
        assert stream == whole and records == whole_records
    finally:
        p.close()
    # the k-mers: the pieces counted == the oracle's count of the text (for -Q: of the masked reads as FASTA)
    want = oracle_counts(O.parse_file(plain), k)
    assert want and table_counts(capi, k, pieces) == want


def test_stream_parse_refusals_leave_the_stream(gpu, holder):
    capi = gpu
    p = capi.Parser(21)
    try:
        bad = b"@r\nACGT\nACGT\n+\nIIII\nIIII\n"                  # wrapped: the host parser's
        n = p.inflate(F.bgzf(bad))
        with pytest.raises(capi.JfgpuError) as e:
            p.stream_parse(n, capi.PARSE_FASTQ)
        assert e.value.code == capi.E_FORMAT
        assert p.stream_read(0, n) == bad                         # nothing consumed: the bytes can be read back
        with pytest.raises(capi.JfgpuError) as e:
            p.stream_parse(n + 1, capi.PARSE_FASTQ)
        assert e.value.code == capi.E_INVALID
        with pytest.raises(capi.JfgpuError) as e:
            p.stream_parse((1 << 31) + 1, capi.PARSE_FASTQ)
        assert e.value.code == capi.E_INVALID
        p.stream_consume(n)
        good = b"@r\nACGT\n+\nIIII\n@s\nGG\n+\nII"
        n = p.inflate(F.bgzf(good))
        cut = p.stream_cut(capi.PARSE_FASTQ)
        assert cut == 15
        ptr, n_out, recs, left = p.stream_parse(cut, capi.PARSE_FASTQ)
        assert bytes(holder.d2h(ptr, n_out)) == b"NACGT" and recs == 1 and left == n - cut
        assert p.stream_read(0, left) == b"@s\nGG\n+\nII"
    finally:
        p.close()
