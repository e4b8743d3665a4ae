"""jfgpu_query_ascii(_dev) on the GPU (-m gpu): the count of every k-mer of a contract buffer in one kernel
(query_ascii_kernel, jellyfish_amd/csrc/kernels.hip.hpp), for every key width -- what `query -s` and
examples/query_per_sequence ask of a database (sub_commands/query_main.cc:44-51).

The expected answer is built here from tests/oracle_lib.py alone: the end positions of the windows are those whose last
k bytes are all in ACGTacgt; O.extract gives the keys there, canonical and as the text has them (their difference is the
reverse-complement bit); O.count of what was counted gives the values.  vals and flags are compared exactly, entry by
entry, over all n.

k = 63, 64 and 128 start at 2^29, 2^31 and 2^31 slots (the slot formats' minimum: 8, 32 and 64 GB): on the device only,
skipped under the host emulation the way tests/test_gpu_wide.py skips k = 63."""
import os
import random

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

MER, FOUND, REVCOMP = 1, 2, 4
TILE = 4096                                                  # kTilePos: positions a workgroup stages at a time, 16 a lane
STAGE = 64 << 20                                             # kStageBytes (jellyfish_amd/csrc/jfgpu.hip): one piece of the host form
EMULATED = bool(os.environ.get("JFGPU_LIB"))
BIG_TABLES = {63: 29, 64: 31, 128: 31}                       # log2 of the smallest table the slot format admits
_COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
_VALID = np.zeros(256, dtype=bool)
_VALID[list(b"ACGTacgt")] = True


def rnd_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n)).encode()


def revcomp(s):
    return s.translate(_COMP)[::-1]


def end_positions(seq, k):
    """Positions p such that seq[p - k + 1 .. p] are all bases."""
    ok = _VALID[np.frombuffer(seq, dtype=np.uint8)]
    idx = np.arange(len(seq), dtype=np.int64)
    last_bad = np.maximum.accumulate(np.where(ok, -1, idx))  # position of the last byte that is no base, at or before p
    return np.nonzero(idx - last_bad >= k)[0]


def count_map(counted, k, canonical):
    keys, cnt = O.count(counted, k, canonical)
    return {keys[i].tobytes(): int(cnt[i]) for i in range(len(keys))}


def expected(seq, k, canonical, table):
    """(vals, flags) that a table holding `table` ({key bytes -> count}) must answer for seq."""
    n = len(seq)
    vals = np.zeros(n, dtype=np.uint64)
    flags = np.zeros(n, dtype=np.uint8)
    ends = end_positions(seq, k)
    keys = np.ascontiguousarray(O.extract(seq, k, canonical))
    text = np.ascontiguousarray(O.extract(seq, k, False))
    assert len(keys) == len(ends) == len(text)
    rc = (keys != text).any(axis=1) if canonical else np.zeros(len(ends), dtype=bool)
    for i, p in enumerate(ends.tolist()):
        c = table.get(keys[i].tobytes())
        flags[p] = MER | (FOUND if c is not None else 0) | (REVCOMP if rc[i] else 0)
        vals[p] = c or 0
    return vals, flags


def check(got, want, what=""):
    (gv, gf), (wv, wf) = got, want
    assert gv.dtype == np.uint64 and gf.dtype == np.uint8 and len(gv) == len(wv) and len(gf) == len(wf)
    bad = np.nonzero((gv != wv) | (gf != wf))[0]
    assert len(bad) == 0, "%s: %d of %d entries differ, first at %d: got (%d, %d), expected (%d, %d)" % (
        what, len(bad), len(wv), bad[0], gv[bad[0]], gf[bad[0]], wv[bad[0]], wf[bad[0]])


def palindrome(rng, k):
    half = rnd_seq(rng, k // 2)
    return half + revcomp(half)


# ---- key widths, positive and negative content -------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", [True, False], ids=["C", "fw"])
@pytest.mark.parametrize("k", [1, 12, 21, 31, 32, 33, 40, 63, 64, 65, 96, 100, 128])
def test_every_key_width_against_the_oracle(gpu, k, canonical):
    if k in BIG_TABLES and EMULATED:
        pytest.skip("k = %d needs 2^%d slots: not under the host emulation" % (k, BIG_TABLES[k]))
    rng = random.Random(1000 * k + canonical)
    # counted: random sequence with a homopolymer run (equal neighbouring keys) and lower case.  k = 1: only 'A' is
    # counted, or every 1-mer would be found
    a = rnd_seq(rng, 1200, "A" if k == 1 else "ACGT") + b"A" * (k + 20) + rnd_seq(rng, 600, "A" if k == 1 else "ACGTacgt")
    counted = a + b"N" + rnd_seq(rng, 700, "A" if k == 1 else "ACGT")
    parts = [a[100:1700], revcomp(a[300:1000 + k]), rnd_seq(rng, 1500 + k), b"n", a[:k + 3]]
    if k % 2 == 0:
        parts += [palindrome(rng, k), palindrome(rng, k)]
    query = b"N".join(parts)
    table = count_map(counted, k, canonical)
    with gpu.Table(k, 1 << (12 + k % 5), canonical=canonical) as t:
        t.count_ascii(counted)
        got = t.query_ascii(query)
        want = expected(query, k, canonical, table)
        check(got, want, "k = %d" % k)
        mers = int((want[1] & MER != 0).sum())
        found = int((want[1] & FOUND != 0).sum())
        assert mers > 3000 and 3 * found >= mers and 10 * (mers - found) >= mers, (mers, found)     # an all-zero answer cannot pass
        if canonical:
            assert (want[1] & REVCOMP != 0).sum() > 500
        assert t.stats().total == sum(table.values())        # (the table is as counted: the query added nothing)


# ---- tile edges: halo staging and window reset across lanes and tiles, for each view's halo (2, 4 and 8 words) -------------
@pytest.fixture(scope="module")
def edge_text():
    return rnd_seq(random.Random(5), 3 * TILE + 7 + 300)


@pytest.mark.parametrize("k", [21, 40, 100])
def test_tile_edges(gpu, edge_text, k):
    canonical = True
    table = count_map(edge_text, k, canonical)
    with gpu.Table(k, 1 << 15, canonical=canonical) as t:
        t.count_ascii(edge_text)
        t.sync()
        for n in (0, 1, k - 1, k, k + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 7):
            q = edge_text[:n]
            check(t.query_ascii(q), expected(q, k, canonical, table), "length %d" % n)
        base = bytearray(edge_text[:TILE + 200])
        for off in (15, 16, 17, TILE - 1, TILE, TILE + 1):
            for what, put in (("N", b"N"), ("lower case", bytes(base[off:off + 2 * k + 5]).lower()), ("IUPAC", b"R")):
                q = bytearray(base)
                q[off:off + len(put)] = put
                q = bytes(q)
                want = expected(q, k, canonical, table)
                check(t.query_ascii(q), want, "%s at %d" % (what, off))
                if what == "lower case":                     # the same answers as in upper case
                    check(want, expected(bytes(base), k, canonical, table), "oracle, lower case at %d" % off)
        # a run of bases that ends exactly at the tile's last position, the next run starts with the next tile
        q = edge_text[:TILE - 1 - 2 * k] + b"N" + edge_text[500:500 + 2 * k] + edge_text[700:700 + 3 * k]
        assert q[TILE - 1 - 2 * k] == ord("N") and len(q) > TILE + k
        want = expected(q, k, canonical, table)
        check(t.query_ascii(q), want, "runs meeting at the tile edge")
        q = q[:TILE] + b"N" + q[TILE + 1:]                   # ... and the second run is cut off from it
        want2 = expected(q, k, canonical, table)
        assert (want2[1][TILE:TILE + k] == 0).all() and (want[1][TILE:TILE + k] != 0).all()
        check(t.query_ascii(q), want2, "a reset on the tile's first position")
        q = q[:TILE - 1] + b"N" + edge_text[TILE:TILE + 3 * k]      # ... or the reset is the tile's last position and a run starts the next tile
        check(t.query_ascii(q), expected(q, k, canonical, table), "a run that starts with the tile")


# ---- device form: unaligned sequence pointer, guards behind the outputs, no flags ------------------------------------------
@pytest.mark.parametrize("k", [21, 40, 100])
def test_unaligned_device_buffers_and_guards(gpu, k):
    rng = random.Random(77 + k)
    text = rnd_seq(rng, 6000, "ACGTN" if k == 21 else "ACGT")
    table = count_map(text, k, True)
    with gpu.Table(k, 1 << 14) as t:
        t.count_ascii(text)
        t.sync()
        mers_before = t.counters()["mers"]
        pad = 32
        d_seq = t.malloc(len(text) + 4 * pad)
        d_vals = t.malloc(8 * (len(text) + 2))
        d_flags = t.malloc(len(text) + 32)
        try:
            for shift, n in ((0, TILE + 48), (1, 5000), (7, TILE + 9), (15, 4999), (0, 4993)):
                q = text[200:200 + n]
                # bases before and after the buffer: a kernel reading outside [0, n) would see windows that are not there
                t.h2d(d_seq, np.frombuffer(b"ACGT" * (pad // 4) + text[200 - shift:200] + q + b"ACGT" * (pad // 2), dtype=np.uint8))
                want = expected(q, k, True, table)
                for with_flags in (True, False):
                    t.h2d(d_vals, np.full(n + 2, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64))
                    t.h2d(d_flags, np.full(n + 32, 0xEE, dtype=np.uint8))
                    t.query_ascii_dev(d_seq + pad + shift, n, d_vals, d_flags if with_flags else None)
                    t.wait()
                    gv = t.d2h(d_vals, 8 * (n + 2)).view(np.uint64)
                    gf = t.d2h(d_flags, n + 32)
                    assert (gv[n:] == 0xA5A5A5A5A5A5A5A5).all() and (gf[n:] == 0xEE).all(), "written beyond n"
                    if not with_flags:                       # flags == NULL: the same counts, and nothing written for the flags
                        assert (gf == 0xEE).all()
                        gf = want[1]
                    check((gv[:n].copy(), gf[:n].copy()), want, "pointer + %d, n = %d, flags %s" % (shift, n, with_flags))
            assert t.counters()["mers"] == mers_before      # CTR_MERS is the count's, a query leaves it alone
        finally:
            t.free(d_seq); t.free(d_vals); t.free(d_flags)


# ---- counts beyond the slot's field --------------------------------------------------------------------------------------
def test_counts_beyond_the_slot_field(gpu):
    rng = random.Random(9)
    # a homopolymer long enough to wrap a 32-bit slot's count field into the side table
    k = 12
    with gpu.Table(k, 1 << 16) as t:
        assert t.info.slot_bytes == 4
        run = b"A" * 5000 + b"N" + rnd_seq(rng, 300)
        t.count_ascii(run)
        t.sync()
        assert t.counters()["ovf_used"] > 0
        q = b"A" * 40 + b"C" + b"T" * 30
        got = t.query_ascii(q)
        check(got, expected(q, k, True, count_map(run, k, True)), "homopolymer")
        assert got[0][k - 1] == 5000 - k + 1 and got[0][-1] == 5000 - k + 1 and got[1][-1] == MER | FOUND | REVCOMP
    # pairs whose values do not fit the field
    for k in (21, 40):
        kw = (2 * k + 63) // 64
        with gpu.Table(k, 1 << 14, canonical=False) as t:
            mers = [rnd_seq(rng, k) for _ in range(200)]
            keys = np.array([O.from_str(m.decode(), k) for m in mers], dtype=np.uint64).reshape(-1, kw)
            vals = np.array([rng.choice([1, 2 ** 40 + 3, 2 ** 63 + 11, 2 ** 64 - 1, rng.getrandbits(64)]) for _ in mers], dtype=np.uint64)
            table = {}
            for i in range(len(mers)):
                table[keys[i].tobytes()] = table.get(keys[i].tobytes(), 0) + int(vals[i])
            assert max(table.values()) < 2 ** 64
            t.add_key_vals(keys, vals)
            q = b"N".join(mers) + b"N" + rnd_seq(rng, 300)
            want = expected(q, k, False, table)
            assert (want[0] > 2 ** 62).sum() > 20
            check(t.query_ascii(q), want, "big values, k = %d" % k)


# ---- pending partitioned work, growth -------------------------------------------------------------------------------------
def test_query_sees_pending_partitioned_counts_and_survives_growth(gpu):
    rng = random.Random(41)
    k = 21
    first, second = rnd_seq(rng, 30000, "ACGTN"), rnd_seq(rng, 90000)
    q = first[1000:6000] + b"N" + rnd_seq(rng, 2000) + b"N" + second[:3000]
    with gpu.Table(k, 1 << 16) as t:
        t.set_mode(2)
        lsize0 = t.info.lsize
        d_seq = t.malloc(len(second) + 16)
        d_q = t.malloc(len(q) + 16)
        d_vals = t.malloc(8 * len(q))
        d_flags = t.malloc(len(q))
        try:
            t.h2d(d_q, np.frombuffer(q, dtype=np.uint8))

            def ask():
                t.query_ascii_dev(d_q, len(q), d_vals, d_flags)
                t.wait()
                return t.d2h(d_vals, 8 * len(q)).view(np.uint64).copy(), t.d2h(d_flags, len(q))

            t.h2d(d_seq, np.frombuffer(first, dtype=np.uint8))
            t.count_ascii_dev(d_seq, len(first))             # no sync: the batch is pending in the partition workspace
            check(ask(), expected(q, k, True, count_map(first, k, True)), "after an un-synced partitioned count")
            c = t.counters()
            assert c["p1_ring"] + c["p1_other"] > 0, "the partitioned path did not run"
            mers = c["mers"]
            check(ask(), expected(q, k, True, count_map(first, k, True)), "asked again")
            assert t.counters()["mers"] == mers
            t.h2d(d_seq, np.frombuffer(second, dtype=np.uint8))
            t.count_ascii_dev(d_seq, len(second))            # more distinct k-mers than 80 % of 2^16 slots: the table doubles
            got = ask()
            t.sync()
            assert t.info.lsize > lsize0
            check(got, expected(q, k, True, count_map(first + b"N" + second, k, True)), "after a growth")
        finally:
            t.free(d_seq); t.free(d_q); t.free(d_vals); t.free(d_flags)


# ---- host form: the seam between two stage pieces ------------------------------------------------------------------------
def test_host_form_across_a_stage_seam(gpu):
    """The real seam: kStageBytes (64 MiB) is left alone and the buffer is two pieces long -- 64 MiB and a little.  Nearly all
    of it is 'N' (no windows, nothing for the oracle to do); sequence sits at the start, across the seam (windows of both
    pieces, and the k - 1 positions the second piece must leave to the first), behind it and at the end.  On the device this is 64 MiB in and 0.6 GB out, a
    second or two; under the host emulation the same call takes longer and runs all the same."""
    rng = random.Random(3)
    k = 31
    n = STAGE + 5000
    text = rnd_seq(rng, 8000)
    table = count_map(text, k, True)
    regions = [(0, text[:2000]), (STAGE - 700, text[2000:3400]), (STAGE + 1000, text[4000:5000]), (n - 1500, text[5000:6500])]
    seq = np.full(n, ord("N"), dtype=np.uint8)
    want_v, want_f = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint8)
    for at, s in regions:
        assert (seq[at:at + len(s)] == ord("N")).all() and (at == 0 or seq[at - 1] == ord("N"))
        seq[at:at + len(s)] = np.frombuffer(s, dtype=np.uint8)
        v, f = expected(s, k, True, table)
        want_v[at:at + len(s)], want_f[at:at + len(s)] = v, f
    assert want_f[STAGE - 5:STAGE + 5].all() and want_f[n - 1] & (MER | FOUND) == MER | FOUND
    with gpu.Table(k, 1 << 14) as t:
        t.count_ascii(text)
        got = t.query_ascii(seq.tobytes())
    check(got, (want_v, want_f), "two stage pieces")


# ---- errors ---------------------------------------------------------------------------------------------------------------
def test_errors(gpu):
    import ctypes as C
    lib = gpu.load()
    seq = np.frombuffer(b"ACGTACGTACGTACGTACGTACGTACGT", dtype=np.uint8)
    vals, flags = np.zeros(len(seq), dtype=np.uint64), np.zeros(len(seq), dtype=np.uint8)
    with gpu.Table(21, 1 << 14) as t:
        for fn in (lib.jfgpu_query_ascii, lib.jfgpu_query_ascii_dev):
            assert fn(t._h, None, 0, None, None) == gpu.OK                           # nothing asked
            assert fn(t._h, seq.ctypes.data, 0, None, None) == gpu.OK
            assert fn(t._h, None, len(seq), vals.ctypes.data, flags.ctypes.data) == gpu.E_INVALID
            assert fn(t._h, seq.ctypes.data, len(seq), None, flags.ctypes.data) == gpu.E_INVALID
            assert fn(None, seq.ctypes.data, len(seq), vals.ctypes.data, flags.ctypes.data) == gpu.E_INVALID
        v, f = t.query_ascii(b"")
        assert len(v) == 0 and len(f) == 0
    with gpu.Table(21, 1 << 16, shard_bits=1, shard_id=1) as t:
        d = t.malloc(4096)
        try:
            for fn, ptrs in ((lib.jfgpu_query_ascii, (seq.ctypes.data, vals.ctypes.data, flags.ctypes.data)),
                             (lib.jfgpu_query_ascii_dev, (d, d + 1024, d + 2048))):
                assert fn(t._h, ptrs[0], len(seq), ptrs[1], ptrs[2]) == gpu.E_UNSUPPORTED
                assert b"shard" in lib.jfgpu_last_error()
                assert fn(t._h, ptrs[0], 0, ptrs[1], ptrs[2]) == gpu.OK
        finally:
            t.free(d)


# ---- add_key_vals at three and four words ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [65, 100, 128])
def test_add_key_vals_of_three_and_four_words(gpu, k):
    if k in BIG_TABLES and EMULATED:
        pytest.skip("k = %d needs 2^%d slots: not under the host emulation" % (k, BIG_TABLES[k]))
    rng = random.Random(k)
    kw = (2 * k + 63) // 64
    mers = sorted({rnd_seq(rng, k) for _ in range(3000)})
    keys = np.array([O.from_str(m.decode(), k) for m in mers], dtype=np.uint64).reshape(-1, kw)
    vals = np.array([rng.choice([1, 7, 65535, 65536, 2 ** 47 + 1, 2 ** 63 + 5, 2 ** 64 - 1]) for _ in mers], dtype=np.uint64)
    vals[:50] = 5
    with gpu.Table(k, 1 << 12, canonical=False) as t:        # 3000 pairs into 2^12 slots: the table doubles on the way
        half = len(keys) // 2
        t.add_key_vals(keys[:half], vals[:half])
        t.add_key_vals(keys[half:], vals[half:])
        t.add_key_vals(keys[:50], np.full(50, 3, dtype=np.uint64))                   # again: added to what is there
        want = vals.copy()
        want[:50] += np.uint64(3)
        lv, lf = t.lookup(keys)
        assert lf.all() and (lv == want).all()
        absent = np.array([O.from_str(rnd_seq(rng, k).decode(), k) for _ in range(100)], dtype=np.uint64).reshape(-1, kw)
        lv, lf = t.lookup(absent)
        assert not lf.any() and not lv.any()
        q = b"N".join(mers[:400]) + b"N" + rnd_seq(rng, 500)
        table = {keys[i].tobytes(): int(want[i]) for i in range(len(keys))}
        exp = expected(q, k, False, table)
        assert (exp[1] == MER | FOUND).sum() == 400 and (exp[1] == MER).sum() > 300
        check(t.query_ascii(q), exp, "k = %d" % k)
        st = t.stats()
        assert st.distinct == len(keys)
