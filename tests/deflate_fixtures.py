"""A deflate *writer* for the inflate conformance tests, with the standard library only.

The device inflate (bgzf_inflate_kernel) must give the verdict of the reference reader on every RFC 1951 stream, not
only on the streams zlib's compressor happens to write.  This module writes streams by hand, with every choice an
encoder has under the caller's control, and lets zlib's *decoder* judge them:

  * BitWriter                    Huffman codes MSB first, everything else LSB first (RFC 1951 3.1.1)
  * canonical(lens)              code assignment from code lengths (3.2.2), also for sets that are not complete
  * stored / fixed / dynamic / reserved    block descriptions; a dynamic block takes HLIT, HDIST, HCLEN, the
                                 code-length-code lengths, the header's token sequence (literal lengths and 16 / 17 / 18
                                 with their repeat counts) and the two length sets, each explicit or derived
  * lit / match / L / D / R      LZ77 tokens: by value, or as raw symbols with raw extra bits, or as raw bits
  * encode(blocks)               the stream; simulate(blocks) the payload the tokens mean (an LZ77 interpreter)
  * judge(cdata)                 zlib's verdict: the bytes when `zlib.decompressobj(-15)` reaches the end of the stream
                                 with at most 64 KiB of output (input left over is ignored, as htslib does), else None
  * Case / make_case / layout    a stream in a BGZF member (sam_fixtures.bgzf_member) with the CRC32 / ISIZE of zlib's
                                 output when zlib accepts and of the intended payload when it refuses, and the upload
                                 and block table of many members
  * DIRECTED                     the named edge cases, each built with the verdict it is meant to have: a case whose
                                 zlib verdict is another one fails as a fixture
  * generated_valid / generated_mutated    seeded random streams (Kraft-complete random codes up to 15 bits, random
                                 legal header tokenisations, tokens over the full length and distance ranges), and the
                                 same streams damaged in one place

A member is refused when zlib refuses its stream, and also when its trailer speaks of another payload than the stream
holds (ISIZE one more or one less): the BGZF reader checks the trailer against the inflated bytes.  The expected value
never comes from the engine.
"""
import bisect
import heapq
import random
import struct
import zlib

import sam_fixtures as F

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
         8193, 12289, 16385, 24577]
DEXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def rand_bytes(rng, n):
    return rng.getrandbits(8 * n).to_bytes(n, "little") if n else b""


# ---------------------------------------------------------------- bits and codes
class BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    @property
    def bitpos(self):
        return len(self.out) * 8 + self.n

    def bits(self, v, n):
        """n bits of v, least significant first."""
        assert 0 <= v < (1 << n) or (n == 0 and v == 0), (v, n)
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):
        """A Huffman code of n bits, most significant first."""
        self.bits(reverse(code, n), n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, b):
        assert self.n == 0
        self.out += b

    def getvalue(self):
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def reverse(code, n):
    r = 0
    for i in range(n):
        r |= ((code >> i) & 1) << (n - 1 - i)
    return r


def as_list(lens, n=0):
    """A length set given as {symbol: length} or as a list -> a list of at least n entries."""
    if isinstance(lens, dict):
        lens = [lens.get(s, 0) for s in range(max(lens, default=-1) + 1)]
    return list(lens) + [0] * (n - len(lens))


def canonical(lens):
    """Canonical codes (RFC 1951 3.2.2) of a list of lengths; None where the length is 0.  An over-subscribed set gets
    the codes the algorithm gives, cut to their lengths: such a set is only written to be refused."""
    maxl = max(lens, default=0)
    cnt = [0] * (maxl + 2)
    for l in lens:
        if l:
            cnt[l] += 1
    nxt, code = [0] * (maxl + 2), 0
    for l in range(1, maxl + 1):
        code = (code + cnt[l - 1]) << 1
        nxt[l] = code
    codes = [None] * len(lens)
    for s, l in enumerate(lens):
        if l:
            codes[s] = nxt[l] & ((1 << l) - 1)
            nxt[l] += 1
    return codes


def kraft(lens, maxlen=15):
    """Sum of 2^-l in units of 2^-maxlen: 1 << maxlen when the set is complete."""
    return sum(1 << (maxlen - l) for l in lens if l)


def huff_lengths(freq, maxlen):
    """Code lengths of a Huffman code of {symbol: frequency}, at most maxlen bits, complete (one symbol: length 1)."""
    syms = sorted(freq)
    assert syms
    if len(syms) == 1:
        return {syms[0]: 1}
    lens = dict.fromkeys(syms, 0)
    heap = [(freq[s], i, [s]) for i, s in enumerate(syms)]
    heapq.heapify(heap)
    tick = len(syms)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[2] + b[2]:
            lens[s] += 1
        heapq.heappush(heap, (a[0] + b[0], tick, a[2] + b[2]))
        tick += 1
    if max(lens.values()) > maxlen:
        for s in syms:
            lens[s] = min(lens[s], maxlen)
        cap, k = 1 << maxlen, kraft(lens.values(), maxlen)
        while k > cap:                                              # lengthen the longest codes that can still grow
            s = max((s for s in syms if lens[s] < maxlen), key=lambda s: (lens[s], -freq[s]))
            k -= 1 << (maxlen - lens[s] - 1)
            lens[s] += 1
        while k < cap:                                              # and give back what that took too much
            s = max((s for s in syms if lens[s] > 1 and (1 << (maxlen - lens[s])) <= cap - k), key=lambda s: (lens[s], freq[s]))
            k += 1 << (maxlen - lens[s])
            lens[s] -= 1
    assert kraft(lens.values(), maxlen) == 1 << maxlen
    return lens


def random_complete_lengths(rng, n, maxlen):
    """n code lengths of a random Kraft-complete set, none above maxlen (n >= 2): leaves of a random binary tree, half
    of the splits at the deepest leaf that may still split so that long codes are common."""
    assert 2 <= n <= 1 << maxlen
    leaves = [1, 1]
    while len(leaves) < n:
        open_ = [i for i, d in enumerate(leaves) if d < maxlen]
        i = max(open_, key=lambda i: leaves[i]) if rng.random() < 0.5 else rng.choice(open_)
        leaves[i] += 1
        leaves.append(leaves[i])
    rng.shuffle(leaves)
    assert kraft(leaves, maxlen) == 1 << maxlen
    return leaves


# ---------------------------------------------------------------- tokens
def L(sym, extra=0):
    """A literal / length symbol with its extra bits given raw."""
    return ("L", sym, extra)


def D(sym, extra=0):
    return ("D", sym, extra)


def R(value, nbits):
    """Raw bits in the token stream (an unassigned code, say)."""
    return ("R", value, nbits)


def lit(b):
    return [("L", b, 0)]


def lits(data):
    return [("L", b, 0) for b in data]


def len_sym(length):
    for i in range(28, -1, -1):
        if LBASE[i] <= length < LBASE[i] + (1 << LEXTRA[i]) and (i < 28 or length == 258):
            return 257 + i
    raise ValueError(length)


def dist_sym(dist):
    for i in range(29, -1, -1):
        if DBASE[i] <= dist < DBASE[i] + (1 << DEXTRA[i]):
            return i
    raise ValueError(dist)


def match(length, dist, lsym=None, dsym=None):
    """A length / distance pair by value; lsym: the length symbol to use where two can say it (258 = 284 + 31 = 285)."""
    ls = len_sym(length) if lsym is None else lsym
    ds = dist_sym(dist) if dsym is None else dsym
    return [("L", ls, length - LBASE[ls - 257]), ("D", ds, dist - DBASE[ds])]


class Invalid(Exception):
    pass


def simulate(blocks, strict=True):
    """The payload the blocks mean.  strict=False: what they give up to the first thing that has no meaning."""
    out = bytearray()
    try:
        for b in blocks:
            if b["type"] == "stored":
                if b.get("len") is not None or b.get("nlen") is not None:
                    raise Invalid("stored block with a false length")
                out += b["data"]
                continue
            if b["type"] == "reserved":
                raise Invalid("block type 3")
            toks = b["tokens"]
            i = 0
            while i < len(toks):
                kind, s, e = toks[i]
                i += 1
                if kind != "L":
                    raise Invalid("stray token")
                if s < 256:
                    out.append(s)
                elif s == 256:
                    break
                else:
                    if s > 285 or i >= len(toks) or toks[i][0] != "D" or toks[i][1] > 29:
                        raise Invalid("no such length or distance")
                    length, dist = LBASE[s - 257] + e, DBASE[toks[i][1]] + toks[i][2]
                    i += 1
                    if dist > len(out):
                        raise Invalid("distance too far back")
                    at = len(out) - dist
                    if dist >= length:
                        out += out[at:at + length]
                    else:
                        for j in range(length):
                            out.append(out[at + j])
            if not b.get("eob", True):
                raise Invalid("no end of block")
    except Invalid:
        if strict:
            raise
    return bytes(out)


# ---------------------------------------------------------------- blocks
def stored(data, final=None, len_=None, nlen=None):
    """len_ / nlen: the LEN and NLEN fields when they are not to be those of data."""
    return {"type": "stored", "data": bytes(data), "final": final, "len": len_, "nlen": nlen}


def fixed(tokens, final=None, eob=True):
    return {"type": "fixed", "tokens": list(tokens), "final": final, "eob": eob}


def dynamic(tokens, final=None, eob=True, lit_lens=None, dist_lens=None, hlit=None, hdist=None, hclen=None, cl_lens=None,
            header=None, rng=None):
    """lit_lens / dist_lens: {symbol: length} or lists (default: Huffman lengths of the tokens' own frequencies);
    hlit / hdist: the numbers of lengths sent (default: up to the last one that is not 0); header: the token sequence
    that sends them, literal lengths as ints and runs as (16 | 17 | 18, count) (default: tokenise(), at random with an
    rng); with a header and no length sets, the sets are what the header expands to; cl_lens: the code-length code
    (default: Huffman lengths of the header's frequencies, 7 bits at most); hclen: how many of them are sent."""
    return {"type": "dynamic", "tokens": list(tokens), "final": final, "eob": eob, "lit_lens": lit_lens, "dist_lens": dist_lens,
            "hlit": hlit, "hdist": hdist, "hclen": hclen, "cl_lens": cl_lens, "header": header, "rng": rng}


def reserved(final=None):
    return {"type": "reserved", "final": final}


def tokenise(seq, rng=None):
    """A legal header token sequence for the lengths seq: greedy (the longest run code wherever one applies), or with an
    rng a random choice among everything legal at each place -- 16 after a zero included."""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, run = seq[i], 1
        while i + run < n and seq[i + run] == v:
            run += 1
        opts = []
        if v == 0 and run >= 11:
            opts.append((18, 11, min(138, run)))
        if v == 0 and run >= 3:
            opts.append((17, 3, min(10, run)))
        if i > 0 and seq[i - 1] == v and run >= 3:
            opts.append((16, 3, min(6, run)))
        if rng is None:
            pick = opts[0] if opts else None
            rep = pick[2] if pick else 1
        else:
            pick = rng.choice(opts + opts + [None]) if opts else None
            rep = 1 if pick is None else (pick[2] if rng.random() < 0.5 else rng.randint(pick[1], pick[2]))
        out.append(v if pick is None else (pick[0], rep))
        i += rep
    return out


def expand(header):
    """The lengths a header token sequence means: 16 repeats the last length written, whichever token wrote it."""
    seq = []
    for t in header:
        if isinstance(t, int):
            seq.append(t)
        elif t[0] == 16:
            seq += [seq[-1] if seq else 0] * t[1]
        else:
            seq += [0] * t[1]
    return seq


def _with_dummy(freq, universe):
    """A second symbol for a set of one, so that the default sets are complete."""
    if len(freq) == 1:
        freq[next(s for s in universe if s not in freq)] = 1
    return freq


def _dyn_params(b):
    toks, header, hlit, hdist = b["tokens"], b["header"], b["hlit"], b["hdist"]
    lit_lens, dist_lens = b["lit_lens"], b["dist_lens"]
    if header is not None and (lit_lens is None or dist_lens is None):
        assert hlit is not None and hdist is not None
        seq = expand(header)[:hlit + hdist]
        seq += [0] * (hlit + hdist - len(seq))
        lit_lens = seq[:hlit] if lit_lens is None else lit_lens
        dist_lens = seq[hlit:] if dist_lens is None else dist_lens
    if lit_lens is None:
        freq = {}
        for k, s, _ in toks:
            if k == "L":
                freq[s] = freq.get(s, 0) + 1
        if b["eob"]:
            freq[256] = freq.get(256, 0) + 1
        lit_lens = huff_lengths(_with_dummy(freq, range(286)), 15)
    if dist_lens is None:
        freq = {}
        for k, s, _ in toks:
            if k == "D":
                freq[s] = freq.get(s, 0) + 1
        dist_lens = huff_lengths(_with_dummy(freq, range(30)), 15) if freq else [0]
    lit_lens, dist_lens = as_list(lit_lens), as_list(dist_lens)
    if hlit is None:
        hlit = max(257, max((s + 1 for s, l in enumerate(lit_lens) if l), default=0))
    if hdist is None:
        hdist = max(1, max((s + 1 for s, l in enumerate(dist_lens) if l), default=0))
    lit_lens, dist_lens = as_list(lit_lens, hlit), as_list(dist_lens, hdist)
    if header is None:
        header = tokenise(lit_lens[:hlit] + dist_lens[:hdist], b["rng"])
    cl_lens = b["cl_lens"]
    if cl_lens is None:
        freq = {}
        for t in header:
            s = t if isinstance(t, int) else t[0]
            freq[s] = freq.get(s, 0) + 1
        cl_lens = huff_lengths(_with_dummy(freq, range(19)), 7)
    cl_lens = as_list(cl_lens, 19)
    hclen = b["hclen"]
    if hclen is None:
        hclen = max(4, max(i + 1 for i in range(19) if cl_lens[CL_ORDER[i]]))
    return lit_lens, dist_lens, hlit, hdist, header, cl_lens, hclen


def _emit_tokens(w, toks, lit_lens, dist_lens, eob):
    lc, dc = canonical(lit_lens), canonical(dist_lens)
    ltab = [(reverse(c, l), l) if l else None for c, l in zip(lc, lit_lens)]
    dtab = [(reverse(c, l), l) if l else None for c, l in zip(dc, dist_lens)]
    for kind, s, e in list(toks) + ([("L", 256, 0)] if eob else []):
        if kind == "R":
            w.bits(s, e)
        elif kind == "L":
            assert s < len(ltab) and ltab[s], "token with a literal / length symbol that has no code: %d" % s
            w.bits(*ltab[s])
            if 257 <= s <= 285:
                w.bits(e, LEXTRA[s - 257])
        else:
            assert s < len(dtab) and dtab[s], "token with a distance symbol that has no code: %d" % s
            w.bits(*dtab[s])
            if s < 30:
                w.bits(e, DEXTRA[s])


class Info:
    """Where things are in an encoded stream (bit offsets): block starts, and the spans of the dynamic headers."""
    def __init__(self):
        self.block_starts, self.header_spans = [], []


def encode(blocks):
    """-> (the deflate stream, Info).  The last block is final unless a block says otherwise."""
    w, info = BitWriter(), Info()
    for i, b in enumerate(blocks):
        final = b["final"] if b.get("final") is not None else i == len(blocks) - 1
        info.block_starts.append(w.bitpos)
        w.bits(int(final), 1)
        if b["type"] == "stored":
            w.bits(0, 2)
            w.align()
            n = len(b["data"]) if b["len"] is None else b["len"]
            w.bits(n, 16)
            w.bits((~n & 0xFFFF) if b["nlen"] is None else b["nlen"], 16)
            w.raw(b["data"])
        elif b["type"] == "fixed":
            w.bits(1, 2)
            _emit_tokens(w, b["tokens"], FIXED_LIT, FIXED_DIST, b["eob"])
        elif b["type"] == "reserved":
            w.bits(3, 2)
        else:
            lit_lens, dist_lens, hlit, hdist, header, cl_lens, hclen = _dyn_params(b)
            w.bits(2, 2)
            w.bits(hlit - 257, 5)
            w.bits(hdist - 1, 5)
            w.bits(hclen - 4, 4)
            for j in range(hclen):
                w.bits(cl_lens[CL_ORDER[j]], 3)
            cc = canonical(cl_lens)
            for t in header:
                s = t if isinstance(t, int) else t[0]
                assert cl_lens[s], "header token %d has no code in the code-length code" % s
                w.code(cc[s], cl_lens[s])
                if s == 16:
                    w.bits(t[1] - 3, 2)
                elif s == 17:
                    w.bits(t[1] - 3, 3)
                elif s == 18:
                    w.bits(t[1] - 11, 7)
            info.header_spans.append((info.block_starts[-1], w.bitpos))
            _emit_tokens(w, b["tokens"], lit_lens, dist_lens, b["eob"])
    return w.getvalue(), info


# ---------------------------------------------------------------- the judge, cases, members
def judge(cdata):
    """zlib's verdict on a raw deflate stream: its output, or None (refused)."""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(cdata)
    except zlib.error:
        return None
    if not d.eof or len(out) > 65536:
        return None
    return out


class Case:
    """One member: cdata and the trailer's fields; want = the bytes the engine must give, None = it must refuse."""
    def __init__(self, name, cdata, want, crc, isize, extra_first=b""):
        self.name, self.cdata, self.want, self.crc, self.isize, self.extra_first = name, cdata, want, crc, isize, extra_first

    @property
    def verdict(self):
        return "refuse" if self.want is None else "accept"

    def member(self):
        return F.bgzf_member(None, extra_first=self.extra_first, cdata=self.cdata, crc32=self.crc, isize=self.isize, oversize=True)

    def fits_bgzf(self):
        return 18 + len(self.extra_first) + len(self.cdata) + 8 <= 65536


def make_case(name, cdata, intended=None, expect=None, extra_first=b"", trailer=None):
    """intended: the payload the writer meant (checked against zlib when the case is meant to be accepted; the trailer's
    source when zlib refuses).  trailer: a payload other than the stream's for CRC32 / ISIZE: the member is refused.
    expect: the verdict the case is built for -- another one is an error of the fixture."""
    out = judge(cdata)
    if trailer is not None:
        assert out is not None and trailer != out, "%s: a false trailer needs a stream zlib accepts" % name
        src, want = trailer, None
    elif out is not None:
        src, want = out, out
    else:
        src, want = intended if intended is not None else b"", None
    c = Case(name, cdata, want, zlib.crc32(src) & 0xFFFFFFFF, len(src), extra_first)
    if expect is not None:
        assert c.verdict == expect, "%s: built to be a case of '%s', but the reference verdict is '%s'" % (name, expect, c.verdict)
        if expect == "accept" and intended is not None:
            assert out == intended, "%s: zlib's output is not the payload the writer meant" % name
    return c


def case_of_blocks(name, blocks, expect=None, **kw):
    cdata, _ = encode(blocks)
    intended = kw.pop("intended", None)
    if intended is None:
        intended = simulate(blocks, strict=expect == "accept")
    return make_case(name, cdata, intended, expect, **kw)


def layout(cases, eof=False):
    """The upload of the members one after the other, and their block table rows (c_off, u_off, c_len, isize, crc32)."""
    parts, rows, off, u = [], [], 0, 0
    for c in cases:
        m = c.member()
        rows.append((off + 18 + len(c.extra_first), u, len(c.cdata), c.isize, c.crc))
        parts.append(m)
        off += len(m)
        u += c.isize
    if eof:
        parts.append(F.EOF_MARKER)
    return b"".join(parts), rows


# ---------------------------------------------------------------- directed cases
DIRECTED = {}          # name -> (the verdict it is built for, builder -> Case)


def directed(name, expect):
    def deco(f):
        assert name not in DIRECTED, name
        DIRECTED[name] = (expect, f)
        return f
    return deco


def blocks_case(name, expect, build, **kw):
    """Registers a case given by a function -> blocks."""
    DIRECTED[name] = (expect, lambda: case_of_blocks(name, build(), expect, **kw))


def directed_case(name):
    c = DIRECTED[name][1]()
    assert c.verdict == DIRECTED[name][0], name
    return c


def directed_names(expect):
    return sorted(n for n, (e, _) in DIRECTED.items() if e == expect)


A0A = lits(b"a\0a")
A0A_LENS = {0: 2, 97: 2, 256: 1}


def a0a(header, hlit=257, hdist=1, **kw):
    return lambda: [dynamic(A0A, header=header, hlit=hlit, hdist=hdist, **kw)]


# --- header run-length codes.  The lengths of a\0a: 0 -> 2, 1..96 -> 0, 97 -> 2, 98..255 -> 0, 256 -> 1, distance 0 -> 0
blocks_case("hdr_zero_runs_end_in_literal_0", "accept", a0a([2, (18, 95), 0, 2, (18, 138), (18, 19), 0, 1, 0]))
blocks_case("hdr_16_after_18", "accept", a0a([2, (18, 90), (16, 6), 2, (18, 138), (18, 17), (16, 3), 1, 0]))
blocks_case("hdr_16_after_17", "accept", a0a([2, (18, 86), (17, 4), (16, 6), 2, (18, 138), (17, 10), (17, 7), (16, 3), 1, 0]))
blocks_case("hdr_16_after_literal_0", "accept", a0a([2, (18, 92), 0, (16, 3), 2, (18, 138), (18, 16), 0, (16, 3), 1, 0]))
blocks_case("hdr_16_first", "refuse", a0a([(16, 3), (18, 94), 2, (18, 138), (18, 20), 1, 0], lit_lens=A0A_LENS, dist_lens=[0]))
blocks_case("hdr_run_overshoots_hlit_hdist", "refuse", a0a([2, (18, 96), 2, (18, 138), (18, 20), 1, (17, 3)]))
# 254 -> 3, then 16 x 6 and 16 x 5 over 255, 256, 257 and the eight distance lengths
blocks_case("hdr_16_run_crosses_into_distances", "accept", lambda: [dynamic(
    lits([97, 254, 255] * 2) + match(3, 2) + match(3, 4) + lits([97]) + match(3, 13),
    header=[(18, 97), 1, (18, 138), (18, 18), 3, (16, 6), (16, 5)], hlit=258, hdist=8)])
# 260 -> 2, then 17 x 6 over 261..263 and distances 0..2, distance 3 -> 1
blocks_case("hdr_17_run_crosses_into_distances", "accept", lambda: [dynamic(
    lits([97] * 4) + match(6, 4), header=[(18, 97), 1, (18, 138), (18, 20), 2, (17, 3), 2, (17, 6), 1], hlit=264, hdist=4)])
# 260 -> 2, then 18 x 13 over 261..269 and distances 0..3, distance 4 -> 1
blocks_case("hdr_18_run_crosses_into_distances", "accept", lambda: [dynamic(
    lits([97] * 6) + match(6, 6), header=[(18, 97), 1, (18, 138), (18, 20), 2, (17, 3), 2, (18, 13), 1], hlit=270, hdist=5)])

# --- header counts
# HCLEN 4 sends lengths for 16, 17, 18 and 0 only: no length but 0 can be said, so there is no end-of-block code and the
# reference refuses every such block.  HCLEN 5 adds the code for length 8: the smallest count that can be accepted.
blocks_case("hclen_4", "refuse", lambda: [dynamic([], eob=False, header=[(18, 138), (18, 120)], hlit=257, hdist=1, hclen=4,
                                                   cl_lens={18: 1, 0: 1})])
blocks_case("hclen_5", "accept", lambda: [dynamic(lits(b"HCLEN 5: every code has 8 bits"), header=[8] * 255 + [0, 8, 0], hlit=257, hdist=1,
                                                   hclen=5, cl_lens={0: 1, 8: 1})])
LADDER = list(range(1, 16)) + [15]                       # lengths 1 .. 15 and a second 15: complete


def ladder_blocks():
    """Both alphabets with every length from 1 to 15, and every code used: the 11- to 15-bit ones are beyond the
    decoder's first-level table.  Frequencies fall with the length, as they would in a Fibonacci-like source."""
    lsyms = [65 + i for i in range(11)] + [257, 270, 285, 90, 256]        # lengths 1 .. 11 on literals, 12 13 14 15 15
    lit_lens = dict(zip(lsyms, LADDER))
    dist_lens = dict(zip(range(16), LADDER))
    rng = random.Random(15)
    toks = []
    for i in range(11):
        toks += lits([65 + i] * max(2, 200 >> i))
    toks += lits([90, 90])
    rng.shuffle(toks)
    for ds in range(16):
        for e, ln in ((0, 3), ((1 << DEXTRA[ds]) - 1, 258), (0, 23), ((1 << DEXTRA[ds]) - 1, 26)):
            toks += match(ln, DBASE[ds] + e) + lits([90, 65 + ds % 11])
    return [dynamic(toks, lit_lens=lit_lens, dist_lens=dist_lens)]


def _ladder_hclen19():
    b = ladder_blocks()
    assert _dyn_params(b[0])[6] == 19                    # length 15 is the last of the code-length order
    return b


blocks_case("huffman_lengths_1_to_15_all_used_hclen_19", "accept", _ladder_hclen19)
blocks_case("code_length_code_of_7_bits", "accept", lambda: [dynamic(
    lits(b"abcdefabcabaaaaaabbbcc"), lit_lens={97: 1, 98: 2, 99: 3, 100: 4, 101: 5, 102: 6, 256: 6}, dist_lens=[0],
    cl_lens={18: 1, 6: 2, 0: 3, 1: 4, 2: 5, 3: 6, 4: 7, 5: 7})])
blocks_case("hlit_257", "accept", a0a([2, (18, 96), 2, (18, 138), (18, 20), 1, 0]))


def _hlit(n):
    lens = huff_lengths({s: 1 + (s % 3) for s in range(n)}, 15)
    return lambda: [dynamic(lits(b"all the symbols") + match(258, 1) + lits([255]), lit_lens=lens, hlit=n)]


blocks_case("hlit_286", "accept", _hlit(286))
blocks_case("hlit_287", "refuse", _hlit(287))
blocks_case("hlit_288", "refuse", _hlit(288))
blocks_case("hdist_1_of_length_0_literals_only", "accept", lambda: [dynamic(lits(b"literals only"), dist_lens=[0], hdist=1)])


def _hdist(n):
    lens = huff_lengths({s: 1 + (s % 3) for s in range(n)}, 15)
    return lambda: [stored(rand_bytes(random.Random(n), 24600)), dynamic(lits(b"xy") + match(3, 24577) + match(5, 1), dist_lens=lens, hdist=n)]


blocks_case("hdist_30", "accept", _hdist(30))
blocks_case("hdist_31", "refuse", _hdist(31))
blocks_case("hdist_32", "refuse", _hdist(32))
blocks_case("no_end_of_block_code", "refuse", lambda: [dynamic(lits(b"abab"), eob=False, lit_lens={97: 1, 98: 1})])

# --- Huffman sets
blocks_case("one_distance_code_of_length_1_used", "accept", lambda: [dynamic(lits(b"abcde") + match(5, 4), dist_lens={3: 1})])
blocks_case("one_distance_code_its_sibling_used", "refuse",
            lambda: [dynamic(lits(b"abcde") + [L(259), R(1, 1)], lit_lens=huff_lengths({s: 1 for s in (97, 98, 99, 100, 101, 256, 259)}, 15),
                             dist_lens={3: 1})])
blocks_case("no_distance_code_and_a_match", "refuse",
            lambda: [dynamic(lits(b"abcde") + [L(259), R(0, 1)], lit_lens=huff_lengths({s: 1 for s in (97, 98, 99, 100, 101, 256, 259)}, 15),
                             dist_lens=[0])])
blocks_case("oversubscribed_code_length_code", "refuse",
            lambda: [dynamic(lits(b"aa"), lit_lens={97: 1, 256: 1}, dist_lens=[0], header=[(18, 97), 1, (18, 138), (18, 20), 1, 0],
                             cl_lens={18: 1, 1: 1, 0: 1})])
blocks_case("oversubscribed_literal_set", "refuse", lambda: [dynamic(A0A, lit_lens={0: 1, 97: 1, 256: 1}, dist_lens=[0])])
blocks_case("oversubscribed_distance_set", "refuse", lambda: [dynamic(lits(b"abc") + match(3, 1), dist_lens=[1, 1, 1])])
blocks_case("incomplete_code_length_code", "refuse",
            lambda: [dynamic(lits(b"aa"), lit_lens={97: 1, 256: 1}, dist_lens=[0], header=[(18, 97), 1, (18, 138), (18, 20), 1, 0],
                             cl_lens={18: 2, 1: 2, 0: 2})])
blocks_case("incomplete_code_length_code_of_one_code", "refuse",
            lambda: [dynamic(lits(b"aa"), lit_lens=[8] * 257, dist_lens=[8], header=[8] * 258, cl_lens={8: 1})])
blocks_case("incomplete_literal_set", "refuse", lambda: [dynamic(lits(b"a"), lit_lens={97: 2, 256: 1}, dist_lens=[0])])
blocks_case("incomplete_literal_set_unused_long_code", "refuse", lambda: [dynamic(lits(b"ab"), lit_lens={97: 1, 98: 2, 256: 3}, dist_lens=[0])])
# zlib lets a set be incomplete when it is one code of one bit: here only the end-of-block code
blocks_case("literal_set_of_one_code_of_length_1", "accept", lambda: [dynamic([], lit_lens={256: 1}, dist_lens=[0])])
blocks_case("literal_set_of_one_code_its_sibling_used", "refuse", lambda: [dynamic([R(1, 1)], lit_lens={256: 1}, dist_lens=[0])])
blocks_case("literal_set_of_one_code_of_length_2", "refuse", lambda: [dynamic([], lit_lens={256: 2}, dist_lens=[0])])
blocks_case("incomplete_distance_set_used", "refuse", lambda: [dynamic(lits(b"abc") + match(3, 1), dist_lens=[2, 2])])
blocks_case("incomplete_distance_set_unused", "refuse", lambda: [dynamic(lits(b"abc"), dist_lens=[2, 2, 2])])
blocks_case("distance_set_of_one_code_of_length_2", "refuse", lambda: [dynamic(lits(b"abc") + match(3, 1), dist_lens=[2])])
blocks_case("distance_set_of_one_code_unused", "accept", lambda: [dynamic(lits(b"abc"), dist_lens={7: 1})])


# --- matches
def _both(toks, before=()):
    """The same tokens in a fixed and in a dynamic block (the second one's matches reach into the first)."""
    return list(before) + [fixed(toks), dynamic(toks)]


for _s in range(257, 286):
    _hi = (1 << LEXTRA[_s - 257]) - 1
    blocks_case("length_symbol_%d_both_ends" % _s, "accept", lambda s=_s, hi=_hi: _both(
        lits(b"wxyz") + [L(s, 0), D(0, 0)] + lits(b"q") + [L(s, hi), D(2, 0)] + lits(b"r") + [L(s, hi), D(3, 0)]))
for _d in range(30):
    _hi = (1 << DEXTRA[_d]) - 1
    blocks_case("distance_symbol_%d_both_ends" % _d, "accept", lambda d=_d, hi=_hi: _both(
        [L(257, 0), D(d, 0), L(260, 0), D(d, hi)] + lits(b"k") + [L(285, 0), D(d, hi)],
        before=[stored(rand_bytes(random.Random(d), DBASE[d] + hi))]))
blocks_case("length_258_as_symbol_284_with_extra_31", "accept", lambda: _both(lits(b"ab") + match(258, 2, lsym=284) + match(258, 1)))
blocks_case("distance_32768_with_a_full_window_length_258", "accept",
            lambda: _both(match(258, 32768) + match(3, 32768), before=[stored(rand_bytes(random.Random(1), 32768))]))


def _dist1():
    toks = []
    for n in range(3, 259):
        toks += lit(n & 255) + match(n, 1)
    return toks


blocks_case("distance_1_lengths_3_to_258_fixed", "accept", lambda: [fixed(_dist1())])
blocks_case("distance_1_lengths_3_to_258_dynamic", "accept", lambda: [dynamic(_dist1())])
for _d in (2, 3, 5, 7, 63, 64, 65, 127, 257):
    blocks_case("overlapping_copy_distance_%d" % _d, "accept", lambda d=_d: _both(
        lits(rand_bytes(random.Random(d), d)) + match(d + 1, d) + match(min(258, 2 * d + 3), d) + lits(b"!") + match(258, d)))
blocks_case("distance_equal_to_position", "accept", lambda: [fixed(lits(b"0123456") + match(10, 7)), dynamic(match(30, 17))])
blocks_case("distance_of_position_plus_1_fixed", "refuse", lambda: [fixed(lits(b"0123456") + match(10, 8))])
blocks_case("distance_of_position_plus_1_dynamic", "refuse", lambda: [stored(b"0123456"), dynamic(lits(b"7") + match(10, 9))])
blocks_case("match_at_position_0", "refuse", lambda: [fixed(match(3, 1))])
PREV = {"stored": lambda d: stored(d), "fixed": lambda d: fixed(lits(d)), "dynamic": lambda d: dynamic(lits(d))}
for _p in PREV:
    for _c, _mk in (("fixed", fixed), ("dynamic", dynamic)):
        blocks_case("match_source_in_previous_%s_block_from_%s" % (_p, _c), "accept", lambda p=_p, mk=_mk: [
            PREV[p](b"twenty bytes of text"), mk(match(10, 20) + lits(b"+") + match(258, 31))])


def _to_65536(last=()):
    """32768 stored bytes, then matches up to byte 65536 exactly; last: what follows in the same block."""
    toks = []
    for _ in range(126):
        toks += match(258, 32768)
    toks += match(257, 32768) + match(3, 5)
    return [stored(rand_bytes(random.Random(3), 32768)), fixed(toks + list(last))]


blocks_case("match_ends_exactly_at_65536", "accept", _to_65536)
blocks_case("literal_past_65536", "refuse", lambda: _to_65536(lits(b"x")))
blocks_case("match_past_65536", "refuse", lambda: _to_65536()[:1] + [fixed(_to_65536()[1]["tokens"][:-2] + match(4, 5))])
blocks_case("stored_block_past_65536", "refuse", lambda: [dict(b, final=False) for b in _to_65536()] + [stored(b"x")])


def _isize_case(name, build, delta):
    def f():
        cdata, _ = encode(build())
        out = simulate(build())
        return make_case(name, cdata, out, "refuse", trailer=out[:-1] if delta > 0 else out + b"\0")
    DIRECTED[name] = ("refuse", f)


_SMALL = lits(b"some bytes, then the last one")
_isize_case("one_byte_more_than_isize_by_a_literal", lambda: [dynamic(_SMALL)], 1)
_isize_case("one_byte_more_than_isize_by_a_match", lambda: [dynamic(_SMALL + match(3, 7))], 1)
_isize_case("one_byte_more_than_isize_by_a_stored_block", lambda: [fixed(_SMALL, final=False), stored(b"z")], 1)
_isize_case("one_byte_more_than_isize_by_a_long_stored_block", lambda: [fixed(_SMALL, final=False), stored(b"z" * 300)], 1)
_isize_case("one_byte_less_than_isize", lambda: [dynamic(_SMALL + match(3, 7))], -1)
_isize_case("one_byte_less_than_isize_empty_stream", lambda: [fixed([])], -1)

# --- fixed blocks: the fixed code has codes for symbols that do not exist
blocks_case("fixed_length_symbol_286", "refuse", lambda: [fixed(lits(b"abc") + [L(286), D(0)])])
blocks_case("fixed_length_symbol_287", "refuse", lambda: [fixed(lits(b"abc") + [L(287), D(0)])])
blocks_case("fixed_distance_symbol_30", "refuse", lambda: [fixed(lits(b"abc") + [L(257), D(30)])])
blocks_case("fixed_distance_symbol_31", "refuse", lambda: [fixed(lits(b"abc") + [L(257), D(31)])])


@directed("fixed_empty_final_block_of_2_bytes", "accept")
def _empty_fixed():
    cdata, _ = encode([fixed([])])
    assert cdata == b"\x03\x00"
    return make_case("fixed_empty_final_block_of_2_bytes", cdata, b"", "accept")


# --- stored blocks
blocks_case("stored_len_0_between_huffman_blocks", "accept",
            lambda: [fixed(lits(b"before ")), stored(b""), dynamic(lits(b"after ") + match(6, 13)), stored(b""), fixed(match(4, 4))])


def _phase(p):
    def f():
        blocks = [fixed(lits([200] * ((p - 2) % 8))), stored(b"stored bytes at a bit phase"), fixed(lits(b"tail") + match(5, 9))]
        _, info = encode(blocks)
        assert info.block_starts[1] % 8 == p
        return blocks
    return f


for _p in range(8):
    blocks_case("stored_block_entered_at_bit_phase_%d" % _p, "accept", _phase(_p))
blocks_case("stored_len_65535", "accept", lambda: [stored(rand_bytes(random.Random(4), 65535)), fixed(lits(b"e"))])
blocks_case("stored_len_nlen_mismatch", "refuse", lambda: [stored(b"abcdef", nlen=(~6 & 0xFFFF) ^ 0x100)])
blocks_case("stored_len_runs_past_the_member", "refuse", lambda: [stored(b"x" * 50, len_=100)])


@directed("stored_header_cut_short", "refuse")
def _stored_cut():
    cdata, _ = encode([fixed(lits(b"ab")), stored(b"")])
    return make_case("stored_header_cut_short", cdata[:-2], b"ab", "refuse")


# --- block type and block count
blocks_case("block_type_3", "refuse", lambda: [fixed(lits(b"ab")), reserved()])
blocks_case("block_type_3_first", "refuse", lambda: [reserved()])


def _tiny_blocks():
    rng = random.Random(300)
    blocks, pos = [], 0
    for i in range(300):
        data = rand_bytes(rng, rng.randint(0, 5))
        toks = lits(data)
        if pos >= 4 and rng.random() < 0.5:
            toks += match(rng.randint(3, 12), rng.randint(1, min(pos, 300)))
        kind = rng.choice(("stored", "fixed", "dynamic"))
        blocks.append(stored(data) if kind == "stored" else fixed(toks) if kind == "fixed" else dynamic(toks, rng=rng))
        pos = len(simulate(blocks))
    return blocks


blocks_case("three_hundred_tiny_blocks_of_mixed_type", "accept", _tiny_blocks)
blocks_case("only_empty_blocks", "accept", lambda: [stored(b""), fixed([]), dynamic([]), stored(b""), dynamic([], lit_lens={256: 1}, dist_lens=[0]), fixed([])])

# --- framing: where the deflate data starts and ends relative to the 4-byte words the bit reader loads
for _k in range(4):
    blocks_case("data_starts_after_an_extra_subfield_of_%d_bytes" % _k, "accept",
                lambda: [dynamic(lits(b"framing framing framing") + match(20, 8))], extra_first=b"XY" + struct.pack("<H", _k) + b"z" * _k)
    blocks_case("data_ends_at_byte_alignment_%d" % _k, "accept", lambda k=_k: [fixed(lits(b"end")), stored(b"0123456789"[:6 + k])])


@directed("last_byte_cut_and_first_crc_byte_equal_to_it", "refuse")
def _cut_last():
    """The stream lacks its last byte, and the CRC32 field behind it begins with exactly that byte: a decoder that reads
    on into the trailer sees a complete stream."""
    rng = random.Random(8)
    for _ in range(20000):
        payload = rand_bytes(rng, 9)
        cdata, _ = encode([dynamic(lits(payload))])
        if judge(cdata[:-1]) is None and (zlib.crc32(payload) & 0xFF) == cdata[-1]:
            c = make_case("last_byte_cut_and_first_crc_byte_equal_to_it", cdata[:-1], payload, "refuse")
            assert judge(c.member()[18:18 + len(cdata)]) == payload           # with one byte of the trailer it is whole
            return c
    raise AssertionError("no payload found whose CRC32 begins with the cut byte")


# ---------------------------------------------------------------- CRC lane split
CRC_SIZES = list(range(0, 201)) + [4095, 4096, 4097] + list(range(65472, 65537))
CRC_KINDS = ("stored", "fixed", "dynamic")


def compressible_tokens(rng, size):
    """Tokens of exactly size bytes: a few literals, then mostly long matches (few tokens for a large payload)."""
    toks, pos = [], 0
    while pos < size:
        if pos < 40 or size - pos < 3 or rng.random() < 0.2:
            toks += lit(rng.getrandbits(8))
            pos += 1
        else:
            n = min(size - pos, rng.choice((258, 258, rng.randint(3, 258))))
            toks += match(n, rng.randint(1, min(pos, 32768)))
            pos += n
    return toks


def crc_case(size, kind):
    rng = random.Random(size * 3 + CRC_KINDS.index(kind))
    if kind == "stored":
        data = rand_bytes(rng, size)
        blocks = [stored(data)] if size < 65536 else [stored(data[:40000]), stored(data[40000:])]
    else:
        toks = compressible_tokens(rng, size)
        blocks = [fixed(toks)] if kind == "fixed" else [dynamic(toks)]
    c = case_of_blocks("crc_%s_%d" % (kind, size), blocks, "accept")
    assert len(c.want) == size
    return c


# ---------------------------------------------------------------- generated streams
def _pick_size(rng):
    r = rng.random()
    if r < 0.08:
        return rng.randint(0, 10)
    if r < 0.75:
        return int(2 ** rng.uniform(0, 12))
    if r < 0.93:
        return rng.randint(4097, 65536)
    return 65536 - rng.choice((0, 0, 0, 1, 2, 3))


def _gen_tokens(rng, pos, share, literals, lsyms, dsyms):
    """Random tokens of exactly share bytes from the given symbols; pos: bytes before them."""
    toks, end = [], pos + share
    lsyms, dsyms = sorted(lsyms), sorted(dsyms)                    # (bases grow with the symbols)
    lbase, dbase = [LBASE[s - 257] for s in lsyms], [DBASE[d] for d in dsyms]
    while pos < end:
        rem = end - pos
        nl, nd = bisect.bisect_right(lbase, rem), bisect.bisect_right(dbase, pos)
        if nl and nd and rng.random() < 0.7:
            s, d = lsyms[rng.randrange(nl)], dsyms[rng.randrange(nd)]
            le = rng.randint(0, min((1 << LEXTRA[s - 257]) - 1, rem - LBASE[s - 257]))
            de = rng.randint(0, min((1 << DEXTRA[d]) - 1, pos - DBASE[d]))
            toks += [L(s, le), D(d, de)]
            pos += LBASE[s - 257] + le
        else:
            toks.append(L(rng.choice(literals), 0))
            pos += 1
    return toks


def _gen_dynamic(rng, pos, share):
    k = rng.choice((1, 2, 3, rng.randint(1, 40), rng.randint(1, 256)))
    literals = sorted(rng.sample(range(256), k))
    lsyms = sorted(rng.sample(range(257, 286), rng.choice((0, 1, rng.randint(0, 29), 29))))
    dsyms = sorted(rng.sample(range(30), rng.choice((0, 1, 2, rng.randint(0, 30), 30))))
    syms = literals + [256] + lsyms
    lit_lens = dict(zip(syms, random_complete_lengths(rng, len(syms), 15)))
    if len(dsyms) == 0:
        dist_lens = [0]
    elif len(dsyms) == 1:
        dist_lens = {dsyms[0]: 1}
    else:
        dist_lens = dict(zip(dsyms, random_complete_lengths(rng, len(dsyms), 15)))
    hlit = rng.randint(max(257, syms[-1] + 1), 286)
    hdist = rng.randint(max(1, dsyms[-1] + 1 if dsyms else 1), 30)
    header = tokenise(as_list(lit_lens, hlit) + as_list(dist_lens, hdist), rng)
    used = sorted({t if isinstance(t, int) else t[0] for t in header})
    spare = [s for s in range(19) if s not in used]
    rng.shuffle(spare)
    used += spare[:max(2 - len(used), rng.choice((0, 0, 1, 3, len(spare))))]
    cl_lens = dict(zip(used, random_complete_lengths(rng, len(used), 7)))
    need = max(4, max(i + 1 for i in range(19) if CL_ORDER[i] in cl_lens))
    toks = _gen_tokens(rng, pos, share, literals, lsyms, dsyms)
    return dynamic(toks, lit_lens=lit_lens, dist_lens=dist_lens, hlit=hlit, hdist=hdist, header=header, cl_lens=cl_lens,
                   hclen=rng.randint(need, 19))


def gen_blocks(rng, need_dynamic=False):
    """A valid stream: 1 to 12 blocks of random type, a payload of 0 to 65536 bytes."""
    target, n = _pick_size(rng), rng.randint(1, 12)
    blocks, pos = [], 0
    for i in range(n):
        rem = target - pos
        share = rem if i == n - 1 else rng.choice((0, rng.randint(0, rem), rng.randint(0, rem) // 4))
        kind = "dynamic" if need_dynamic and i == 0 else rng.choice(("stored", "fixed", "dynamic", "dynamic"))
        if kind == "stored":
            share = min(share, 65535)
            blocks.append(stored(rand_bytes(rng, share)))
        elif kind == "fixed":
            blocks.append(fixed(_gen_tokens(rng, pos, share, range(256), range(257, 286), range(30))))
        else:
            blocks.append(_gen_dynamic(rng, pos, share))
        pos += share
    return blocks


def generated_valid(seed, count):
    """count valid streams.  Every one must be accepted by zlib with the payload its tokens mean: nothing is filtered."""
    rng = random.Random(seed)
    cases = []
    for i in range(count):
        blocks = gen_blocks(rng)
        c = case_of_blocks("valid_%d_%d" % (seed, i), blocks, "accept")
        assert c.isize <= 65536
        cases.append(c)
    return cases


MUTATIONS = ("header_bits", "token", "truncate", "isize")
# what the tests run: sized so that the whole CPU module takes less time than tests/test_sam_emu.py
VALID_SEED, VALID_COUNT = 20240, 300
MUTATED_SEED, MUTATED_COUNT = 20241, 160


def _mutate_token(rng, blocks):
    cand = [i for i, b in enumerate(blocks) if b["type"] in ("fixed", "dynamic") and b["tokens"]]
    if not cand:
        return None
    bi = rng.choice(cand)
    b = dict(blocks[bi])
    toks = list(b["tokens"])
    if b["type"] == "fixed":
        lset, dset = list(range(286)), list(range(30))
    else:
        lset = [s for s, l in enumerate(as_list(b["lit_lens"])) if l and s != 256]
        dset = [s for s, l in enumerate(as_list(b["dist_lens"])) if l]
    ti = rng.randrange(len(toks))
    kind, s, e = toks[ti]
    if kind == "D":
        s2 = rng.choice(dset)
        toks[ti] = D(s2, rng.randrange(1 << DEXTRA[s2]))
    else:
        s2 = rng.choice([x for x in lset if (x < 256) == (s < 256)])
        toks[ti] = L(s2, rng.randrange(1 << LEXTRA[s2 - 257]) if s2 > 256 else 0)
    b["tokens"] = toks
    return blocks[:bi] + [b] + blocks[bi + 1:]


def generated_mutated(seed, count):
    """count streams of the valid generator, each damaged in one place; the verdict is zlib's (or the trailer rule)."""
    rng = random.Random(seed)
    cases = []
    for i in range(count):
        kind = MUTATIONS[i % len(MUTATIONS)]
        blocks = gen_blocks(rng, need_dynamic=kind == "header_bits")
        payload = simulate(blocks)
        cdata, info = encode(blocks)
        assert judge(cdata) == payload
        name = "mutated_%d_%d_%s" % (seed, i, kind)
        if kind == "header_bits":
            a, b = rng.choice(info.header_spans)
            z = bytearray(cdata)
            for _ in range(rng.choice((1, 1, 2))):
                at = rng.randrange(a, b)
                z[at >> 3] ^= 1 << (at & 7)
            c = make_case(name, bytes(z), payload)
        elif kind == "token":
            mb = _mutate_token(rng, blocks)
            c = make_case(name, encode(mb)[0] if mb else cdata[:-1], payload)
        elif kind == "truncate":
            c = make_case(name, cdata[:max(0, len(cdata) - rng.randint(1, 16))], payload)
        else:
            c = make_case(name, cdata, payload, "refuse", trailer=payload + b"\0" if (rng.random() < 0.5 or not payload) else payload[:-1])
        cases.append(c)
    return cases
