"""jfgpu_sorted_* on the GPU (-m gpu, over capi.Sorted): look-ups in the packed records of a binary/sorted body as the file
has them (jellyfish_amd/csrc/kernels_sorted.hip.hpp, abi_sorted.inl) against an answer built without the engine.

The body is made here: keys and counts from tests/oracle_lib.py, pos = M * key with header_matrix::times restated in numpy
(bit j of the key XORs in columns[c - 1 - j]) under capi.reference_matrix, records sorted by (pos, key) with the key compared
from its most significant word, packed as kb key bytes and vb count bytes, little endian.  The expected vals and flags are
expected() of tests/test_gpu_query.py over a dict of what the body holds; they are compared exactly, entry by entry.

The shapes are a few thousand records and positions.  k = 63, 64 and 128, for which a table starts at tens of gigabytes, are
as small as the rest here and run under the host emulation too."""
import functools
import random

import numpy as np
import pytest

import oracle_lib as O
from test_gpu_query import FOUND, MER, REVCOMP, check, expected, palindrome, revcomp, rnd_seq
from test_gpu_query_text import check as check_text
from test_gpu_query_text import py_lines

pytestmark = pytest.mark.gpu

WIDTHS = [5, 21, 31, 32, 33, 40, 63, 64, 65, 96, 97, 100, 128]
U64 = np.uint64


def lsize_of(k):
    return 12 if k == 5 else 12 + k % 5


def matrix_of(k, lsize):
    """The header's matrix: the reference's for 2^lsize positions, the identity (None) where the key has no more bits."""
    from jellyfish_amd import capi
    return None if lsize >= 2 * k else capi.reference_matrix(lsize, 2 * k)


def positions(keys, k, lsize, matrix):
    """header_matrix::times restated, masked to lsize bits.  keys: (n, nw) uint64."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(len(keys), O.nb_words(k))
    mask = U64((1 << lsize) - 1)
    if matrix is None:
        return keys[:, 0] & mask
    c = 2 * k
    pos = np.zeros(len(keys), dtype=np.uint64)
    for j in range(c):
        bit = (keys[:, j // 64] >> U64(j % 64)) & U64(1)
        pos ^= bit * matrix[c - 1 - j]
    return pos & mask


def make_body(keys, counts, k, lsize, matrix, vb, top_ones=False):
    """(body uint8[n * rb], keys and counts in file order, pos in file order)."""
    nw, kb = O.nb_words(k), (2 * k + 7) // 8
    keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(len(keys), nw)
    counts = np.ascontiguousarray(counts, dtype=np.uint64)
    pos = positions(keys, k, lsize, matrix)
    order = np.lexsort(tuple(keys[:, w] for w in range(nw)) + (pos,))     # the last key is the primary one
    keys, counts, pos = keys[order], counts[order], pos[order]
    kbytes = np.ascontiguousarray(keys).view(np.uint8).reshape(len(keys), 8 * nw)[:, :kb].copy()
    if top_ones and (2 * k) % 8:
        kbytes[:, kb - 1] |= np.uint8((0xFF << ((2 * k) % 8)) & 0xFF)
    vbytes = counts.reshape(-1, 1).view(np.uint8).reshape(len(keys), 8)[:, :vb]
    return np.ascontiguousarray(np.concatenate([kbytes, vbytes], axis=1)).reshape(-1), keys, counts, pos


def table_of(keys, counts):
    return {keys[i].tobytes(): int(counts[i]) for i in range(len(keys))}


def longest_bucket(pos, lsize, bits):
    if not len(pos):
        return 0
    return int(np.bincount((pos >> U64(lsize - bits)).astype(np.int64)).max())


@functools.lru_cache(maxsize=None)
def scenario(k, canonical):
    """The sequences of tests/test_gpu_query.py: what was counted (a homopolymer run, lower case) and what is asked (found,
    other strand, novel, palindromes).  Returns (keys, counts, query, expected answer under counts as counted)."""
    rng = random.Random(1000 * k + canonical)
    a = rnd_seq(rng, 1200) + b"A" * (k + 20) + rnd_seq(rng, 600, "ACGTacgt")
    counted = a + b"N" + rnd_seq(rng, 700)
    parts = [a[100:1700], revcomp(a[300:1000 + k]), rnd_seq(rng, 1500 + k), b"n", a[:k + 3]]
    if k % 2 == 0:
        parts += [palindrome(rng, k), palindrome(rng, k)]
    query = b"N".join(parts)
    keys, counts = O.count(counted, k, canonical)
    want = expected(query, k, canonical, table_of(keys, counts))
    return keys, counts, query, want


def assert_not_degenerate(want, canonical=False):
    mers = int((want[1] & MER != 0).sum())
    found = int((want[1] & FOUND != 0).sum())
    assert mers > 3000 and 3 * found >= mers and 10 * (mers - found) >= mers, (mers, found)     # all-found and all-zero cannot pass
    if canonical:
        assert (want[1] & REVCOMP != 0).sum() > 500


@pytest.fixture(scope="module")
def mem(gpu):
    with gpu.Table(21, 1 << 12) as t:                         # (device memory for the tests: malloc, h2d, d2h)
        yield t


# ---- key widths and strands ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", [True, False], ids=["C", "fw"])
@pytest.mark.parametrize("k", WIDTHS)
def test_every_key_width_against_the_oracle(gpu, k, canonical):
    keys, counts, query, want = scenario(k, canonical)
    if k > 5:                                                 # (of the 1024 5-mers nearly all were counted)
        assert_not_degenerate(want, canonical)
    else:
        assert (want[1] & MER != 0).sum() > 3000 and (want[1] & FOUND != 0).sum() > 1000
    lsize = lsize_of(k)
    matrix = matrix_of(k, lsize)
    assert (matrix is None) == (k == 5)
    for top_ones in ([False, True] if (2 * k) % 8 else [False]):      # the unused bits of the last key byte are not looked at
        body, fkeys, fcounts, pos = make_body(keys, counts, k, lsize, matrix, 4, top_ones)
        with gpu.Sorted(k, 1 << lsize, matrix, 4, body, canonical=canonical) as s:
            assert s.n_records == len(keys)
            check(s.query_ascii(query), want, "k = %d, unused bits %d" % (k, top_ones))
            info = s.info()
            bits, nbytes = gpu.sorted_plan(len(keys), 1 << lsize, k, 4)
            assert info["n_records"] == len(keys) and info["bucket_bits"] == bits
            assert info["longest_bucket"] == longest_bucket(pos, lsize, bits)
            assert info["device_bytes"] == nbytes - (0 if matrix is not None else 2048 * ((2 * k + 7) // 8))


# ---- record shapes: odd record lengths, counts that use all their bytes --------------------------------------------------------
@pytest.mark.parametrize("vb", [1, 2, 4, 8])
@pytest.mark.parametrize("k", [21, 100])
def test_record_shapes(gpu, k, vb):
    keys, _, query, _ = scenario(k, True)
    rng = random.Random(31 * k + vb)
    top = 2 ** (8 * vb) - 1
    counts = np.array([top if i % 7 == 0 else rng.randrange(1, top + 1) for i in range(len(keys))], dtype=np.uint64)
    want = expected(query, k, True, table_of(keys, counts))
    assert_not_degenerate(want, True)
    assert (want[0] == top).sum() > 50
    lsize = lsize_of(k)
    matrix = matrix_of(k, lsize)
    body, _, _, _ = make_body(keys, counts, k, lsize, matrix, vb)
    assert len(body) == len(keys) * ((2 * k + 7) // 8 + vb)
    with gpu.Sorted(k, 1 << lsize, matrix, vb, body) as s:
        check(s.query_ascii(query), want, "k = %d, counter_len = %d" % (k, vb))


# ---- index seams -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", [1, 8, "n"])
@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 513])
def test_index_seams(gpu, n, per):
    k, lsize = 21, 13
    keys, counts, query, _ = scenario(k, True)
    matrix = matrix_of(k, lsize)
    pick = np.sort(np.random.RandomState(n).permutation(len(keys))[:n])
    body, fkeys, fcounts, pos = make_body(keys[pick], counts[pick], k, lsize, matrix, 4)
    want = expected(query, k, True, table_of(fkeys, fcounts))
    assert n < 200 or (want[1] & FOUND != 0).sum() > 100
    rpb = n if per == "n" else per
    with gpu.Sorted(k, 1 << lsize, matrix, 4, body, records_per_bucket=rpb) as s:
        info = s.info()
        bits = gpu.sorted_plan(n, 1 << lsize, k, 4, rpb)[0]
        assert info["bucket_bits"] == bits and (per != "n" or bits == 0)
        assert info["longest_bucket"] == longest_bucket(pos, lsize, bits)
        check(s.query_ascii(query), want, "%d records, %s a bucket" % (n, per))
        if n:                                                 # the first and the last record, by name
            v, f = s.lookup(fkeys[[0, n - 1]])
            assert f.all() and v.tolist() == [int(fcounts[0]), int(fcounts[n - 1])]


def test_three_records_in_a_large_file(gpu):
    k, lsize = 21, 20
    keys, counts, _, _ = scenario(k, True)
    matrix = matrix_of(k, lsize)
    body, fkeys, fcounts, pos = make_body(keys[[10, 700, 1500]], counts[[10, 700, 1500]], k, lsize, matrix, 4)
    with gpu.Sorted(k, 1 << lsize, matrix, 4, body, records_per_bucket=1) as s:
        v, f = s.lookup(fkeys)
        assert f.all() and (v == fcounts).all()
        v, f = s.lookup(keys[[11, 701, 1501, 0, len(keys) - 1]])
        assert not f.any() and not v.any()
        assert s.info()["bucket_bits"] == gpu.sorted_plan(3, 1 << lsize, k, 4, 1)[0]


def test_runs_of_empty_buckets(gpu):
    """Records in three far-apart clusters of positions under the identity matrix: with one record a bucket there are 2^12
    buckets, so the index kernel fills runs of about two thousand empty ones in front of, between and behind the clusters."""
    k, lsize, n_each = 21, 20, 1400
    rng = random.Random(8)
    keys = []
    for bucket in (7, 2000, 4000):                            # of 2^12: the top 12 bits of the position
        lows = rng.sample(range(256), 200)
        keys += [(rng.getrandbits(22) << 20) | (bucket << 8) | lows[i % 200] for i in range(n_each)]
    keys = np.array(sorted(set(keys)), dtype=np.uint64).reshape(-1, 1)
    counts = np.arange(1, len(keys) + 1, dtype=np.uint64)
    assert len(keys) > 4096
    body, fkeys, fcounts, pos = make_body(keys, counts, k, lsize, None, 4)
    with gpu.Sorted(k, 1 << lsize, None, 4, body, canonical=False, records_per_bucket=1) as s:
        info = s.info()
        assert info["bucket_bits"] == 12 and info["longest_bucket"] == longest_bucket(pos, lsize, 12) > 1000
        v, f = s.lookup(fkeys)
        assert f.all() and (v == fcounts).all()
        # keys of empty buckets: in front of the first cluster, between two and behind the last, and the neighbours of each
        absent = np.array([(5 << 20) | (b << 8) | 3 for b in (0, 6, 8, 1000, 1999, 2001, 3999, 4001, 4095)], dtype=np.uint64)
        v, f = s.lookup(absent)
        assert not f.any() and not v.any()


# ---- look-ups that must miss -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", [1, "n"], ids=["one_record", "one_bucket"])
@pytest.mark.parametrize("k", [21, 40, 100])
def test_near_misses(gpu, k, per):
    keys, counts, _, _ = scenario(k, False)
    lsize = lsize_of(k)
    matrix = matrix_of(k, lsize)
    have = {keys[i].tobytes() for i in range(len(keys))}
    body, fkeys, fcounts, pos = make_body(keys, counts, k, lsize, matrix, 4)
    nw = keys.shape[1]
    near = []
    for i in range(0, len(keys), 7):
        a = keys[i].copy()                                    # differs in the top two bits of the top key byte only
        a[(2 * k - 1) // 64] ^= U64(3) << U64((2 * k - 2) % 64)
        near.append(a)
        if nw > 1:                                            # equal in the first word only
            b = keys[i].copy()
            b[1] ^= U64(1)
            near.append(b)
    near = np.array([x for x in near if x.tobytes() not in have], dtype=np.uint64)
    assert len(near) > 100
    with gpu.Sorted(k, 1 << lsize, matrix, 4, body, canonical=False, records_per_bucket=len(keys) if per == "n" else per) as s:
        bits = s.info()["bucket_bits"]
        assert (bits == 0) == (per == "n")
        v, f = s.lookup(near)
        assert not f.any() and not v.any()
        v, f = s.lookup(keys)
        assert f.all() and (v == counts).all()
        # a key whose bucket holds no record
        rng = random.Random(k)
        full = set((pos >> U64(lsize - bits)).tolist())
        cand = np.array([O.from_str(rnd_seq(rng, k).decode(), k) for _ in range(300)], dtype=np.uint64).reshape(-1, nw)
        lonely = cand[[int(b) not in full for b in (positions(cand, k, lsize, matrix) >> U64(lsize - bits)).tolist()]]
        assert per == "n" or len(lonely) > 5
        if len(lonely):
            v, f = s.lookup(lonely)
            assert not f.any() and not v.any()


# ---- lookup(keys) against a dict, bits above 2k ignored ------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 21, 32, 40, 64, 65, 100, 128])
def test_lookup_equals_a_dict(gpu, k):
    keys, counts, _, _ = scenario(k, True)
    lsize = lsize_of(k)
    matrix = matrix_of(k, lsize)
    table = table_of(keys, counts)
    rng = random.Random(5 * k)
    nw = keys.shape[1]
    absent = np.array([O.from_str(rnd_seq(rng, k).decode(), k) for _ in range(400)], dtype=np.uint64).reshape(-1, nw)
    asked = np.concatenate([keys[::3], absent])
    want_v = np.array([table.get(a.tobytes(), 0) for a in asked], dtype=np.uint64)
    want_f = np.array([a.tobytes() in table for a in asked])
    assert want_f.sum() > 300 and (k == 5 or (~want_f).sum() > 300)
    dirty = asked.copy()
    if (2 * k) % 64:
        dirty[:, nw - 1] |= U64((~((1 << ((2 * k) % 64)) - 1)) & (2 ** 64 - 1))
    body, _, _, _ = make_body(keys, counts, k, lsize, matrix, 4)
    with gpu.Sorted(k, 1 << lsize, matrix, 4, body) as s:
        for what in (asked, dirty):
            v, f = s.lookup(what)
            assert (f == want_f).all() and (v == want_v).all()
        v, f = s.lookup(np.zeros((0, nw), dtype=np.uint64))
        assert len(v) == 0 and len(f) == 0


# ---- query_ascii_dev: unaligned sequence pointer, n no multiple of 16, guards behind the outputs ---------------------------------
@pytest.mark.parametrize("k", [21, 100])
def test_unaligned_device_buffers(gpu, mem, k):
    keys, counts, query, _ = scenario(k, True)
    query = query + b"N" + query[:2500]
    assert len(query) > 5300
    lsize = lsize_of(k)
    matrix = matrix_of(k, lsize)
    body, fkeys, _, _ = make_body(keys, counts, k, lsize, matrix, 4)
    table = table_of(keys, counts)
    pad = 32
    d_seq, d_vals, d_flags = mem.malloc(len(query) + 4 * pad), mem.malloc(8 * (len(query) + 2)), mem.malloc(len(query) + 32)
    try:
        with gpu.Sorted(k, 1 << lsize, matrix, 4, body) as s:
            for shift, n in ((0, 4096 + 48), (1, 5000), (7, 4096 + 9), (15, 4999), (0, 4993)):
                q = query[200:200 + n]
                mem.h2d(d_seq, np.frombuffer(b"ACGT" * (pad // 4) + query[200 - shift:200] + q + b"ACGT" * (pad // 2), dtype=np.uint8))
                exp = expected(q, k, True, table)
                for with_flags in (True, False):
                    mem.h2d(d_vals, np.full(n + 2, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64))
                    mem.h2d(d_flags, np.full(n + 32, 0xEE, dtype=np.uint8))
                    s.query_ascii_dev(d_seq + pad + shift, n, d_vals, d_flags if with_flags else None)
                    s.lookup(fkeys[:1])                       # (a host form of the same object: it ends behind the kernel)
                    gv = mem.d2h(d_vals, 8 * (n + 2)).view(np.uint64)
                    gf = mem.d2h(d_flags, n + 32)
                    assert (gv[n:] == 0xA5A5A5A5A5A5A5A5).all() and (gf[n:] == 0xEE).all(), "written beyond n"
                    if not with_flags:
                        assert (gf == 0xEE).all()
                        gf = exp[1]
                    check((gv[:n].copy(), gf[:n].copy()), exp, "pointer + %d, n = %d, flags %s" % (shift, n, with_flags))
    finally:
        mem.free(d_seq); mem.free(d_vals); mem.free(d_flags)


# ---- refusals: create fails with its code and text, and the next create succeeds -----------------------------------------------
def test_refusals(gpu):
    k, lsize = 21, 13
    keys, counts, query, _ = scenario(k, True)
    matrix = matrix_of(k, lsize)
    body, fkeys, fcounts, _ = make_body(keys, counts, k, lsize, matrix, 4)
    rb = (2 * k + 7) // 8 + 4
    recs = body.reshape(-1, rb)
    swapped = recs.copy()
    swapped[[300, 301]] = swapped[[301, 300]]
    doubled = np.concatenate([recs[:500], recs[499:]])
    want = expected(query, k, True, table_of(keys, counts))

    def good():
        with gpu.Sorted(k, 1 << lsize, matrix, 4, body) as s:
            check(s.query_ascii(query), want, "after a refusal")

    good()
    for what, code, text, make in (
            ("swapped", gpu.E_INVALID, "strictly increasing (pos, key) order", lambda: gpu.Sorted(k, 1 << lsize, matrix, 4, swapped.reshape(-1))),
            ("doubled", gpu.E_INVALID, "strictly increasing (pos, key) order", lambda: gpu.Sorted(k, 1 << lsize, matrix, 4, doubled.reshape(-1))),
            ("size", gpu.E_INVALID, "matrix_rows", lambda: gpu.Sorted(k, 1 << (lsize + 1), matrix, 4, body, matrix_rows=lsize)),
            ("size not a power", gpu.E_INVALID, "power of two", lambda: gpu.Sorted(k, (1 << lsize) + 1, matrix, 4, body)),
            ("counter_len 0", gpu.E_INVALID, "counter_len", lambda: gpu.Sorted(k, 1 << lsize, matrix, 0, body)),
            ("counter_len 9", gpu.E_UNSUPPORTED, "counter_len", lambda: gpu.Sorted(k, 1 << lsize, matrix, 9, body)),
            ("k = 129", gpu.E_UNSUPPORTED, "mer length", lambda: gpu.Sorted(129, 1 << lsize, None, 4, body))):
        with pytest.raises(gpu.JfgpuError) as e:
            make()
        assert e.value.code == code and text in e.value.msg, (what, e.value.code, e.value.msg)
        good()


# ---- QueryText.run_sorted: the text of query -s ---------------------------------------------------------------------------------
@pytest.mark.parametrize("piece", [0, 700])
@pytest.mark.parametrize("k", [21, 100])
def test_run_sorted_text(gpu, k, piece):
    keys, counts, query, want = scenario(k, True)
    lsize = lsize_of(k)
    matrix = matrix_of(k, lsize)
    body, _, _, _ = make_body(keys, counts, k, lsize, matrix, 4)
    text, lines = py_lines(query, want[0], want[1], k)
    assert lines > 3000
    with gpu.Sorted(k, 1 << lsize, matrix, 4, body) as s, gpu.QueryText(k, piece_positions=piece) as x:
        check_text(x.run_sorted(s, query), text)
        assert x.counts()[2] == lines and (piece == 0 or x.counts()[0] > 5)
        seen = []
        assert x.run_sorted(s, query, sink=lambda data, n: seen.append(n) or 0) == text and sum(seen) == lines
