"""The routing kernels (route_count_kernel / route_scatter_kernel, every key width) at the level of their own contract,
through jfgpu_partition_ascii_dev alone: no communicator, no exchange, no insert.  -m gpu; the same cases run on the host
emulation in the CPU suite (tests/test_emu_kernels.py).

The judge shares nothing with the engine: the k-mers are the oracle's (oracle/jf_oracle.c), the owner of a k-mer is the top
shard_bits bits of M * key over GF(2), computed here in numpy from the columns the table reports (matrix()).  For every
buffer: counts[s] is the number of oracle k-mers (with multiplicity) whose owner is s; region s of the output -- records
[sum(counts[:s]), +counts[s]) of key_words little-endian words -- holds exactly that multiset, in any order; the words
beyond 2k bits are zero; and nothing behind the last region was written (the buffer is filled with a sentinel first).

The tables are asked for 2^16 slots; the engine raises that to the slot format's minimum (2^30 for k = 32, 2^31 for
k = 64 and 128), and the routing reads nothing of a table but its matrix."""
import os
import random

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

TILE = 4096                                    # sequence positions a workgroup stages at a time (kTilePos)
SENT = np.uint64(0xA5A5A5A5A5A5A5A5)
TAIL = 64                                      # sentinel words kept behind the capacity that is declared
EMU = bool(os.environ.get("JFGPU_LIB"))        # the host emulation (or another experimental build) is loaded


def owners(t, keys, sb):
    """Top sb bits of M * key for each row of keys (n, key_words): column c - 1 - j of the table's matrix is the image of
    key bit j, so bit r of the position is the parity of key & (row r of M)."""
    c, lsize, nw = 2 * t.k, int(t.info.lsize), keys.shape[1]
    cols = [int(x) for x in t.matrix()]
    own = np.zeros(len(keys), dtype=np.int64)
    for r in range(lsize - 1, lsize - 1 - sb, -1):
        row = sum(((cols[c - 1 - j] >> r) & 1) << j for j in range(c))
        x = np.zeros(len(keys), dtype=np.uint64)
        for w in range(nw):
            x ^= keys[:, w] & np.uint64((row >> (64 * w)) & (2 ** 64 - 1))
        for s in (32, 16, 8, 4, 2, 1):
            x ^= x >> np.uint64(s)
        own = (own << 1) | (x & np.uint64(1)).astype(np.int64)
    return own


def sort_rows(rows):
    """The rows in one canonical order (whatever the order, the same for equal multisets)."""
    if len(rows) < 2:
        return rows
    r = rows[np.argsort(rows[:, 0], kind="stable")]
    if rows.shape[1] > 1 and (r[1:, 0] == r[:-1, 0]).any():
        r = rows[np.lexsort(rows.T)]
    return r


def route(t, seq, lo):
    """partition_ascii_dev on a buffer that starts lo bytes behind a 16-byte boundary -> (counts, the whole output buffer)."""
    n, kw = len(seq), t.key_words
    cap = max(n, 1)
    words = cap * kw + TAIL
    d_seq = t.malloc(n + lo + 32)
    d_out = t.malloc(8 * words)
    try:
        assert d_seq % 16 == 0
        if n:
            t.h2d(d_seq + lo, np.frombuffer(seq, dtype=np.uint8))
        t.h2d(d_out, np.full(words, SENT, dtype=np.uint64))
        counts = t.partition_ascii_dev(d_seq + lo, n, d_out, cap)
        out = t.d2h(d_out, 8 * words).view(np.uint64)
    finally:
        t.free(d_seq)
        t.free(d_out)
    return counts.astype(np.int64), out


def check(t, seq, canonical, lo, tag, expect=None):
    k, kw, sb = t.k, t.key_words, int(t.info.shard_bits)
    exp = np.ascontiguousarray(O.extract(seq, k, canonical)) if expect is None else expect
    own = owners(t, exp, sb)
    if len(exp):                               # the reading of matrix() above, against the oracle's own product
        pos = O.matrix_times(t.matrix(), int(t.info.lsize), 2 * k, exp[:32])
        assert ((pos >> np.uint64(int(t.info.lsize) - sb)).astype(np.int64) == own[:32]).all()
    want = np.bincount(own, minlength=1 << sb)
    counts, out = route(t, seq, lo)
    assert counts.tolist() == want.tolist(), tag
    total = int(want.sum())
    assert (out[total * kw:] == SENT).all(), tag + ": words behind the last region were written"
    got = out[:total * kw].reshape(-1, kw)
    if (2 * k) % 64:
        assert not (got[:, kw - 1] >> np.uint64((2 * k) % 64)).any(), tag + ": bits beyond 2k"
    off = 0
    for s in range(1 << sb):
        c = int(want[s])
        assert (sort_rows(got[off:off + c]) == sort_rows(exp[own == s])).all(), "%s: region %d" % (tag, s)
        off += c
    return total


def rnd(rng, n, alphabet="ACGT"):
    return bytearray("".join(rng.choice(alphabet) for _ in range(n)).encode())


def tiles_buffer(rng, k, lo, n_tiles=5, tail=777):
    """n_tiles tiles and a ragged tail, counted from the 16-byte boundary the kernels count their tiles from (the buffer
    starts lo bytes behind it), with an N on the last base of a tile, on the first base of a tile, and k - 1 bases before
    a tile boundary: the halo then carries an invalid base into the next tile's first lanes."""
    seq = rnd(rng, n_tiles * TILE + tail - lo)
    for at in (TILE - 1, 2 * TILE, 3 * TILE - (k - 1)):
        seq[at - lo] = ord("N")
    return bytes(seq)


def buffers(k):
    rng = random.Random(1000 + k)
    yield "5 tiles and a tail", tiles_buffer(rng, k, 0), 0
    yield "5 tiles and a tail, start not aligned", tiles_buffer(rng, k, 5), 5
    yield "length k - 1", bytes(rnd(rng, k - 1)), 0
    yield "length k", bytes(rnd(rng, k)), 0
    yield "length k + 1", bytes(rnd(rng, k + 1)), 13
    yield "homopolymer", b"C" * 3000, 0        # every lane of many waves routes one key to one owner
    yield "random ACGTN", bytes(rnd(rng, 9000, "ACGT" * 8 + "N")), 9


# every boundary of a trait member (key words 1 | 2 | 3 | 4), shard_bits 1 and 2 everywhere, both strands' forms for one k
# per width; 256 owners -- all of s_hist / s_base -- once per width
TABLES = [(k, True, sb) for k in (21, 32, 33, 40, 64, 65, 96, 97, 128) for sb in (1, 2)] + \
         [(k, False, sb) for k in (21, 40, 97) for sb in (1, 2)] + \
         [(32, True, 8), (64, True, 8), (128, True, 8)]


@pytest.mark.parametrize("k,canonical,sb", TABLES)
def test_routed_regions_hold_the_oracle_kmers_of_their_owner(gpu, k, canonical, sb):
    with gpu.Table(k, 1 << 16, canonical=canonical, shard_bits=sb, shard_id=(1 << sb) - 1) as t:
        assert t.key_words == (2 * k + 63) // 64 and t.info.shard_bits == sb
        for tag, seq, lo in buffers(k):
            total = check(t, seq, canonical, lo, tag)
            if tag.startswith("length"):
                assert total == max(0, len(seq) - k + 1)
            elif tag == "homopolymer":
                assert total == 3000 - k + 1


@pytest.mark.parametrize("k", [21, 40, 100])
def test_a_workgroup_that_takes_several_tiles(gpu, k):
    """The grid is clamped to eight workgroups per compute unit; one tile more than that (2049 on the 256 compute units of
    an MI355X, 17 on the emulation's two) is the smallest buffer on which a workgroup goes round its tile loop twice."""
    cus = int(os.environ.get("JFGPU_EMU_CUS", 2)) if EMU else 256
    rng = np.random.default_rng(k)
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(8 * cus + 1) * TILE + 300)].tobytes()
    with gpu.Table(k, 1 << 16, shard_bits=1, shard_id=0) as t:
        assert check(t, seq, True, 0, "clamped grid") == len(seq) - k + 1


@pytest.mark.parametrize("k", [21, 40])
def test_the_senders_bloom_counter_decides_what_is_routed(gpu, k):
    """count --bc over shards: a Bloom counter attached to the shard is asked by both passes.  Half the sequence was
    inserted twice; what is routed is what the ORACLE's check() > 1 says of the counter's bytes (jfo_bc_check, key by
    key: it reads the counter, not the routing kernels), with multiplicity."""
    rng = random.Random(k)
    seq = tiles_buffer(rng, k, 0, tail=500)
    half = seq[:len(seq) // 2]
    with gpu.Bloom(k, gpu.opt_m(0.01, 2 * len(seq)), gpu.opt_k(0.01), canonical=True, seed=7) as b, \
            gpu.Table(k, 1 << 16, shard_bits=2, shard_id=1) as t:
        b.insert_ascii(half + b"N" + half)
        b.sync()
        kmers = np.ascontiguousarray(O.extract(seq, k, True))
        uniq, inv = np.unique(kmers, axis=0, return_inverse=True)
        data, L = b.read(), O.lib()
        h0 = O.matrix_times(b.matrix1, 64, 2 * k, uniq)
        h1 = O.matrix_times(b.matrix2, 64, 2 * k, uniq)
        adm = np.array([L.jfo_bc_check(data.ctypes.data, b.m, b.nb_hashes, x, y) > 1 for x, y in zip(h0.tolist(), h1.tolist())])
        exp = np.ascontiguousarray(kmers[adm[inv.reshape(-1)]])
        assert len(kmers) // 3 < len(exp) < 2 * len(kmers) // 3
        t.attach_bloom(b)
        try:
            for lo in (0, 7):
                assert check(t, seq, True, lo, "bloom, lo %d" % lo, expect=exp) == len(exp)
        finally:
            t.attach_bloom(None)


@pytest.mark.parametrize("k", [21, 40])
def test_a_one_pass_filter_is_refused(gpu, k):
    """A one-pass Bloom filter (count --bf-size) changes as it is asked, and the two passes ask twice: refused before
    anything is launched."""
    seq = bytes(rnd(random.Random(k), 3000))
    with gpu.Bloom(k, gpu.opt_m(0.01, 3000), gpu.opt_k(0.01), canonical=True, one_pass_filter=True) as bf, \
            gpu.Table(k, 1 << 16) as t:
        t.attach_bloom(bf)
        try:
            with pytest.raises(gpu.JfgpuError) as e:
                route(t, seq, 0)
            assert e.value.code == gpu.E_UNSUPPORTED
        finally:
            t.attach_bloom(None)
        counts, out = route(t, seq, 0)                    # (and without the filter the same call routes)
        assert counts.tolist() == [3000 - k + 1] and (out[int(counts[0]) * t.key_words:] == SENT).all()
