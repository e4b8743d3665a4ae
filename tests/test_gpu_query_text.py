"""jfgpu_qtext_*, jfgpu_query_text and jfgpu_bc_query_text on the GPU (-m gpu, over capi.QueryText): the lines of `query -s`
built on the device (jellyfish_amd/csrc/kernels_qtext.hip.hpp, abi_qtext.inl) against a formatter written here in plain
Python -- slices, upper(), a translate table and str(count), no engine code.  Output bytes are compared whole.

Shapes: mer lengths at which the key view, the number of whole dwords of a k-mer and its remainder change (1, 2, 21, 32, 33,
64, 65, 128), counts of every number of digits and at every value where the conversion path changes, lengths around one and
three tiles of 256 positions, sequence and text pointers at every offset class mod 4 and mod 16, guard bytes round the text,
format_dev at and one byte under the needed capacity, host pieces of one window, of less and more than a tile and the
default, a piece without any k-mer, a sink that stops the run."""
import ctypes as C
import random

import numpy as np
import pytest

from test_gpu_bloom_query import expected_of
from test_gpu_query import FOUND, MER, REVCOMP, end_positions, revcomp, rnd_seq

pytestmark = pytest.mark.gpu

U64 = 2 ** 64 - 1
TILE = 256                                                   # kTextBlock: positions of a tile of the formatter
# one value of every digit count, and every value at which the digits or the conversion path (32-bit / 64-bit) change
VALUES = sorted({0, 9, 10, 2 ** 32 - 1, 2 ** 32, 10 ** 19, U64} | {10 ** j - 1 for j in range(1, 20)} | {10 ** j for j in range(1, 20)})
assert {len(str(v)) for v in VALUES} == set(range(1, 21))


def py_lines(seq, vals, flags, k):
    """The reference of these tests: the loop of query_main restated.  Returns (text, lines)."""
    out = []
    for p in np.nonzero(flags & MER)[0].tolist():
        if p < k - 1:
            continue
        w = seq[p - k + 1:p + 1].upper()
        out.append((revcomp(w) if flags[p] & REVCOMP else w) + b" " + str(int(vals[p])).encode() + b"\n")
    return b"".join(out), len(out)


def check(got, want):
    if got != want:
        i = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
        raise AssertionError("%d bytes, expected %d; first difference at byte %d: %r, expected %r"
                             % (len(got), len(want), i, got[max(0, i - 60):i + 60], want[max(0, i - 60):i + 60]))


def synthetic(rng, k, n):
    """n bytes of sequence with N, lower case and a window whose first base is the first byte of the second tile; flags with
    JFGPU_Q_MER exactly at the window ends and JFGPU_Q_REVCOMP at random; vals that go round VALUES."""
    s = bytearray(rnd_seq(rng, n, "ACGTacgt"))
    for at in (TILE - 1, 2 * TILE + 40):
        if at < n:
            s[at] = ord("N")
    seq = bytes(s)
    ends = end_positions(seq, k)
    flags = np.zeros(n, dtype=np.uint8)
    vals = np.zeros(n, dtype=np.uint64)
    flags[ends] = MER
    for i, p in enumerate(ends.tolist()):
        vals[p] = VALUES[i % len(VALUES)] if i < 2 * len(VALUES) else rng.getrandbits(64) >> rng.randrange(64)
        if rng.random() < 0.5:
            flags[p] |= REVCOMP
        if vals[p]:
            flags[p] |= FOUND
    return seq, vals, flags


class DevBuffers:
    """Sequence, answer and text on the device, each with room to shift the pointer and guard bytes round the text."""

    GUARD = 64

    def __init__(self, mem, n_max, text_max):
        self.mem = mem
        self.d_seq, self.d_vals, self.d_flags = mem.malloc(n_max + 64), mem.malloc(8 * n_max + 64), mem.malloc(n_max + 64)
        self.text_max = text_max
        self.d_text = mem.malloc(text_max + 2 * self.GUARD + 16)

    def free(self):
        for p in (self.d_seq, self.d_vals, self.d_flags, self.d_text):
            self.mem.free(p)

    def format(self, x, seq, vals, flags, shift_in=0, shift_out=0, capacity=None):
        """format_dev with the sequence and the flags shifted by shift_in and the text by shift_out; bases in front of and
        behind the sequence (a kernel reading outside [0, n) would print them).  Returns (text, bytes, lines) after checking
        the guards; raises what format_dev raises, after checking that nothing at all was written."""
        n, G = len(seq), self.GUARD
        self.mem.h2d(self.d_seq, np.frombuffer(b"T" * shift_in + seq + b"ACGT" * 8, dtype=np.uint8))
        self.mem.h2d(self.d_vals, np.concatenate([vals, np.full(2, 77, dtype=np.uint64)]))
        self.mem.h2d(self.d_flags, np.concatenate([np.full(shift_in, MER, dtype=np.uint8), flags, np.full(16, MER | REVCOMP, dtype=np.uint8)]))
        total = self.text_max + 2 * G + 16
        self.mem.h2d(self.d_text, np.full(total, 0xA5, dtype=np.uint8))
        cap = self.text_max if capacity is None else capacity
        try:
            nb, nl = x.format_dev(self.d_seq + shift_in, n, self.d_vals, self.d_flags + shift_in, self.d_text + G + shift_out, cap)
        except Exception:
            assert self.mem.d2h(self.d_text, total).tobytes() == b"\xA5" * total, "written although the capacity is short"
            raise
        out = self.mem.d2h(self.d_text, total).tobytes()
        at = G + shift_out
        assert out[:at] == b"\xA5" * at and out[at + nb:] == b"\xA5" * (total - at - nb), "written outside [0, n_bytes)"
        return out[at:at + nb], nb, nl


@pytest.fixture(scope="module")
def mem(gpu):
    with gpu.Table(21, 1 << 12) as t:                         # (device memory for the tests: malloc, h2d, d2h)
        yield t


# ---- format_dev with synthetic answers ------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 21, 32, 33, 64, 65, 128])
def test_format_dev(gpu, mem, k):
    rng = random.Random(k)
    n_max = 3 * TILE + 7
    seq, vals, flags = synthetic(rng, k, n_max)
    assert flags[TILE + k - 1] & MER and not flags[TILE + k - 2] & MER if k > 1 else True     # a window that starts with the second tile
    with gpu.QueryText(k) as x:
        assert x.line_max == k + 22
        bufs = DevBuffers(mem, n_max, n_max * x.line_max)
        try:
            shifts = [(a, b) for a in (0, 1, 3, 15) for b in (0, 1, 3, 15)]
            for i, n in enumerate((0, 1, k - 1, k, TILE - 1, TILE, TILE + 1, n_max)):
                s, v, f = seq[:n], vals[:n].copy(), flags[:n].copy()
                want, lines = py_lines(s, v, f, k)
                for a, b in (shifts if n == n_max else [(0, 0), shifts[(3 * i + 5) % 16]]):
                    got, nb, nl = bufs.format(x, s, v, f, a, b)
                    check(got, want)
                    assert (nb, nl) == (len(want), lines)
                if n >= k:
                    assert lines > 0
            # every digit count went through
            want, lines = py_lines(seq, vals, flags, k)
            assert {len(l.split(b" ")[1]) for l in want.splitlines()} == set(range(1, 21))
            # capacity: exactly the need, and one byte less (nothing written, the need reported)
            got, nb, nl = bufs.format(x, seq, vals, flags, 1, 3, capacity=len(want))
            check(got, want)
            with pytest.raises(gpu.JfgpuError) as e:
                bufs.format(x, seq, vals, flags, 1, 3, capacity=len(want) - 1)
            assert e.value.code == gpu.E_INVALID and e.value.needed == len(want)
            # a JFGPU_Q_MER below k - 1 makes no line; a buffer without any k-mer makes none at all
            f2 = flags.copy()
            f2[:k - 1] = MER
            check(bufs.format(x, seq, vals, f2)[0], want)
            none = b"N" * 300 + b"ACGT"[:min(k - 1, 4)] + b"N" * 300
            assert bufs.format(x, none, np.zeros(len(none), dtype=np.uint64), np.zeros(len(none), dtype=np.uint8), 3, 1) == (b"", 0, 0)
        finally:
            bufs.free()


# ---- the host forms -------------------------------------------------------------------------------------------------------
def host_query(rng, text, k, n):
    """A query of n bytes: parts of the counted text on both strands, random sequence, lower case, and a stretch of N longer
    than a piece of 1000 positions."""
    parts = [text[50:50 + n // 4], revcomp(text[300:300 + n // 5]), b"N" * (2200 if n > 3000 else 0), rnd_seq(rng, n // 5), text[:n // 6].lower(), b"n"]
    q = b"N".join(parts)
    return q + rnd_seq(rng, max(0, n - len(q)))


def run_and_check(x, run, answer, k, q, pieces):
    chunks = []
    got = run(q, sink=lambda data, n_lines: chunks.append((data, n_lines)) or 0)
    vals, flags = answer(q)
    want, lines = py_lines(q, vals, flags, k)
    check(got, want)
    assert b"".join(c[0] for c in chunks) == want
    assert all(c[0] and c[0].endswith(b"\n") and c[0].count(b"\n") == c[1] for c in chunks), "the sink gets whole lines only, and no empty piece"
    assert sum(c[1] for c in chunks) == lines
    assert x.counts() == (pieces, len(q), lines, len(want))
    assert len(chunks) <= pieces
    assert len(x.last_ms()) == 4 and all(t >= 0 for t in x.last_ms())
    return chunks, lines


def n_pieces(n, piece, k):
    return 0 if n == 0 else 1 if n <= piece else 1 + -(-(n - piece) // (piece - (k - 1)))


@pytest.mark.parametrize("piece", [-1, 1000, 4096, 0], ids=["k", "1000", "4096", "default"])
@pytest.mark.parametrize("k", [21, 40, 100])
def test_query_text_of_a_table(gpu, k, piece):
    rng = random.Random(10 * k + max(piece, 0))
    text = rnd_seq(rng, 4000)
    q = host_query(rng, text, k, 700 if piece < 0 else 9000)     # (a piece of k positions is one window: a short query)
    with gpu.Table(k, 1 << 14) as t, gpu.QueryText(k, piece_positions=k if piece < 0 else piece) as x:
        t.count_ascii(text)
        t.sync()
        p = k if piece < 0 else piece if piece else 1 << 21
        chunks, lines = run_and_check(x, lambda s, sink: x.run_table(t, s, sink), t.query_ascii, k, q, n_pieces(len(q), p, k))
        assert lines > 100
        if piece == 1000:
            assert len(chunks) < x.counts()[0], "a piece of only N must not reach the sink"
        # a sink that says stop ends the run with an error
        with pytest.raises(gpu.JfgpuError):
            x.run_table(t, q, sink=lambda data, n_lines: 1)
        assert x.run_table(t, b"") == b"" and x.counts() == (0, 0, 0, 0)
        run_and_check(x, lambda s, sink: x.run_table(t, s, sink), t.query_ascii, k, q[:k - 1], 1)      # no window at all
        assert t.stats().total == len(end_positions(text, k))     # (the table is as counted)


@pytest.mark.parametrize("piece", [-1, 1000, 4096, 0], ids=["k", "1000", "4096", "default"])
@pytest.mark.parametrize("k", [21, 65])
def test_query_text_of_a_bloom_counter(gpu, k, piece):
    rng = random.Random(20 * k + max(piece, 0))
    text = rnd_seq(rng, 4000)
    q = host_query(rng, text, k, 700 if piece < 0 else 9000)
    with gpu.Bloom(k, gpu.opt_m(0.001, 6000), gpu.opt_k(0.001), canonical=True, seed=4) as b, gpu.QueryText(k, piece_positions=k if piece < 0 else piece) as x:
        b.insert_ascii(text)
        b.insert_ascii(text[:150])
        data = b.read()
        p = k if piece < 0 else piece if piece else 1 << 21
        chunks, lines = run_and_check(x, lambda s, sink: x.run_bloom(b, s, sink), b.query_ascii, k, q, n_pieces(len(q), p, k))
        want = expected_of(b, q, True, data=data)                 # (and the answer it formats is the oracle's)
        got = b.query_ascii(q)
        assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
        assert set(want[0][want[1] & MER != 0].tolist()) == {0, 1, 2}
        if piece == 1000:
            assert len(chunks) < x.counts()[0]
        with pytest.raises(gpu.JfgpuError):
            x.run_bloom(b, q, sink=lambda data, n_lines: 1)


# ---- errors ---------------------------------------------------------------------------------------------------------------
def test_errors(gpu):
    lib = gpu.load()
    seq = np.frombuffer(b"ACGTACGTACGTACGTACGTACGTACGT", dtype=np.uint8)
    cb = gpu.TEXT_SINK(lambda user, text, n_bytes, n_lines: 0)
    null_sink = gpu.TEXT_SINK()
    with gpu.QueryText(21) as x, gpu.QueryText(22) as x22:
        with gpu.Table(21, 1 << 14) as t:
            assert lib.jfgpu_query_text(t._h, x._h, seq.ctypes.data, len(seq), cb, None) == gpu.OK
            assert lib.jfgpu_query_text(t._h, x._h, None, 0, cb, None) == gpu.OK
            assert lib.jfgpu_query_text(None, x._h, seq.ctypes.data, len(seq), cb, None) == gpu.E_INVALID
            assert lib.jfgpu_query_text(t._h, None, seq.ctypes.data, len(seq), cb, None) == gpu.E_INVALID
            assert lib.jfgpu_query_text(t._h, x._h, None, len(seq), cb, None) == gpu.E_INVALID
            assert lib.jfgpu_query_text(t._h, x._h, seq.ctypes.data, len(seq), null_sink, None) == gpu.E_INVALID
            assert lib.jfgpu_query_text(t._h, x22._h, seq.ctypes.data, len(seq), cb, None) == gpu.E_INVALID
            assert b"k (22)" in lib.jfgpu_last_error()
        with gpu.Table(21, 1 << 16, shard_bits=1, shard_id=1) as t:
            assert lib.jfgpu_query_text(t._h, x._h, seq.ctypes.data, len(seq), cb, None) == gpu.E_UNSUPPORTED
            assert b"shard" in lib.jfgpu_last_error()
        with gpu.Bloom(21, 10000, 3) as b:
            assert lib.jfgpu_bc_query_text(b._h, x._h, seq.ctypes.data, len(seq), cb, None) == gpu.OK
            assert lib.jfgpu_bc_query_text(None, x._h, seq.ctypes.data, len(seq), cb, None) == gpu.E_INVALID
            assert lib.jfgpu_bc_query_text(b._h, None, seq.ctypes.data, len(seq), cb, None) == gpu.E_INVALID
            assert lib.jfgpu_bc_query_text(b._h, x._h, None, len(seq), cb, None) == gpu.E_INVALID
            assert lib.jfgpu_bc_query_text(b._h, x._h, seq.ctypes.data, len(seq), null_sink, None) == gpu.E_INVALID
            assert lib.jfgpu_bc_query_text(b._h, x22._h, seq.ctypes.data, len(seq), cb, None) == gpu.E_INVALID
        with gpu.Bloom(21, 10000, 3, one_pass_filter=True) as b:
            assert lib.jfgpu_bc_query_text(b._h, x._h, seq.ctypes.data, len(seq), cb, None) == gpu.E_UNSUPPORTED
        if gpu.device_count() > 1:                           # a formatter on another device than the one that answers
            with gpu.QueryText(21, device=1) as other, gpu.Table(21, 1 << 14, device=0) as t, gpu.Bloom(21, 10000, 3, device=0) as b:
                assert lib.jfgpu_query_text(t._h, other._h, seq.ctypes.data, len(seq), cb, None) == gpu.E_INVALID
                assert b"another device" in lib.jfgpu_last_error()
                assert lib.jfgpu_bc_query_text(b._h, other._h, seq.ctypes.data, len(seq), cb, None) == gpu.E_INVALID
    out = C.c_uint32()
    assert lib.jfgpu_qtext_line_max(None, C.byref(out)) == gpu.E_INVALID
    h = C.c_void_p()
    for k, piece, code in ((0, 0, gpu.E_UNSUPPORTED), (129, 0, gpu.E_UNSUPPORTED), (21, 20, gpu.E_INVALID)):
        p = gpu.QTextParams(k=k, device=-1, piece_positions=piece)
        assert lib.jfgpu_qtext_create(C.byref(p), C.byref(h)) == code and not h.value
    assert lib.jfgpu_qtext_create(None, C.byref(h)) == gpu.E_INVALID
