"""The partitioned insert of keys of three and four words (65 <= k <= 128, kernels_nword_part.hip.hpp: P1n, the exact P2 on
256-bit items, Tn) through the C ABI with the mode forced to 2.  Judges: every distinct key's count from the oracle
(tests/oracle_lib.py) by look-up, stats against the oracle, and the content digest of a MODE_DIRECT table fed the same
bytes.  The engine's counters say that the items went through the tile kernel and, on uniform input with regions of twice
the mean, that none of them left the partition (CTR_DIRECT == 0: with 1024 items a bucket twice the mean is more than
30 standard deviations away).

Geometries (k, lsize): 65 / 12 three words, two tiles, b1 = 1;  96 / 14 exactly 192 key bits;  97 / 14 the first four-word
k;  100 / 21 one level at its widest, b1 = 10;  100 / 22 the smallest two-level table;  120 / 15 sixteen count bits;
128 / 31 the smallest table k = 128 has (64 GiB: skipped with less than 80 GiB free, compared by look-up and stats)."""
import os
import random

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

LUT = np.frombuffer(b"ACGT", dtype=np.uint8)


def uniform(seed, n):
    return LUT[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


def special_reads(rng, k):
    """reads with N, lower case and IUPAC letters, one shorter than k, one of exactly k, a homopolymer run longer than k + 1"""
    def rnd(n, alphabet="ACGT"):
        return "".join(rng.choice(alphabet) for _ in range(n))
    reads = [rnd(k - 1), rnd(k), "A" * (k + 7) + rnd(20), rnd(2 * k + 9, "ACGTacgt"), rnd(k + 30) + "N" + rnd(k + 3) + "R" + rnd(k + 1) + "y" + rnd(k - 2),
             rnd(3 * k), "t" * (k + 2), rnd(40, "ACGTNKM") + rnd(k + 5)]
    return ("N".join(reads) + "N").encode()


def oracle(seq, k, canonical):
    keys, cnt = O.count(seq, k, canonical)
    return keys, cnt


def feed(t, pieces):
    for p in pieces:
        t.count_ascii(p)


def check_against_oracle(gpu, t, keys, cnt):
    st = t.stats()
    assert (st.distinct, st.total, st.max_count) == (len(keys), int(cnt.sum()), int(cnt.max()))
    step = 1 << 16
    for a in range(0, len(keys), step):
        vals, found = t.lookup(keys[a:a + step])
        assert found.all()
        assert np.array_equal(np.asarray(vals, dtype=np.uint64), cnt[a:a + step])


def partitioned_table(gpu, k, lsize, canonical, growth=False):
    t = gpu.Table(k, 1 << lsize, canonical=canonical)
    assert t.info.lsize == lsize and t.info.slot_bytes == 32
    t.set_growth(growth)
    t.set_mode(2)                                       # (the parent refuses this for every table of these keys)
    return t


def free_device_bytes(capi):
    """free memory of the current device, asked of the HIP runtime the engine library is linked against; 0 where there is none
    to ask (the host emulation)"""
    import ctypes as C
    try:
        fn = capi.load().hipMemGetInfo
        fn.restype, fn.argtypes = C.c_int, [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        free, total = C.c_size_t(0), C.c_size_t(0)
        return free.value if fn(C.byref(free), C.byref(total)) == 0 else 0
    except Exception:
        return 0


SMALL = [(65, 12, 900), (96, 14, 4000), (97, 14, 4000), (120, 15, 8000)]


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k,lsize,n_random", SMALL)
def test_small_geometries_equal_the_oracle_and_the_direct_kernel(gpu, k, lsize, n_random, canonical):
    rng = random.Random(k * 1000 + lsize)
    a = special_reads(rng, k)
    b = uniform(k + lsize, n_random) + b"N" + a[: len(a) // 2]
    keys, cnt = oracle(a + b"N" + b, k, canonical)
    with partitioned_table(gpu, k, lsize, canonical) as t:
        t.profile_enable(True)
        feed(t, [a, b])                                 # two pending batches when the flush comes
        t.sync()
        check_against_oracle(gpu, t, keys, cnt)
        c = t.counters()
        ms, launches, units = t.profile_get(6)
        assert c["tile_nword"] >= 1 and launches >= 1 and units + c["direct"] == int(cnt.sum())
        assert c["mers"] == int(cnt.sum()) and c["full"] == 0
        dig = t.digest()
    with gpu.Table(k, 1 << lsize, canonical=canonical) as d:
        d.set_growth(False)
        d.set_mode(1)
        feed(d, [a, b])
        d.sync()
        assert d.counters()["tile_nword"] == 0
        assert d.digest() == dig == gpu.digest_of(keys, cnt)


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("lsize", [21, 22])
def test_uniform_input_stays_inside_the_partition(gpu, monkeypatch, lsize, canonical):
    """k = 100 at 2^21 slots (one level, 1024 buckets) and 2^22 (two levels): 2^20 k-mers of uniform random sequence in two
    batches, bucket regions of twice the mean (JFGPU_P1_SLACK = JFGPU_P2_SLACK = 1: head-room over the mean, tuning.hpp)."""
    k = 100
    monkeypatch.setenv("JFGPU_P1_SLACK", "1.0")
    monkeypatch.setenv("JFGPU_P2_SLACK", "1.0")
    half = (1 << 19) + k - 1
    a, b = uniform(lsize, half), uniform(lsize + 100, half)
    extra = special_reads(random.Random(lsize), k)
    keys, cnt = oracle(a + b"N" + b + b"N" + extra, k, canonical)
    assert int(cnt.sum()) >= 1 << 20
    with partitioned_table(gpu, k, lsize, canonical) as t:
        t.profile_enable(True)
        feed(t, [a, b + b"N" + extra])
        t.sync()
        c = t.counters()
        assert c["direct"] == 0 and c["full"] == 0 and c["mers"] == int(cnt.sum())
        assert c["tile_nword"] >= 1 and t.profile_get(6)[2] == int(cnt.sum())
        assert (c["p2_exact"] >= 1) == (lsize == 22) and c["p2_sort"] == 0
        check_against_oracle(gpu, t, keys, cnt)
        dig = t.digest()
    with gpu.Table(k, 1 << lsize, canonical=canonical) as d:
        d.set_growth(False)
        d.set_mode(1)
        feed(d, [a, b + b"N" + extra])
        d.sync()
        assert d.digest() == dig


def test_k128_in_its_smallest_table(gpu):
    k, lsize = 128, 31
    if free_device_bytes(gpu) < 80 << 30:
        pytest.skip("needs 80 GiB of free device memory (a 64 GiB table)")
    rng = random.Random(128)
    a = special_reads(rng, k)
    b = uniform(128, 20000)
    for canonical in (False, True):
        keys, cnt = oracle(a + b"N" + b, k, canonical)
        with partitioned_table(gpu, k, lsize, canonical) as t:
            feed(t, [a, b])
            t.sync()
            assert t.counters()["tile_nword"] >= 1 and t.counters()["p2_exact"] >= 1
            check_against_oracle(gpu, t, keys, cnt)
            dig = t.digest()
        assert dig == gpu.digest_of(keys, cnt)
        with gpu.Table(k, 1 << lsize, canonical=canonical) as d:
            d.set_growth(False)
            d.set_mode(1)
            feed(d, [a, b])
            d.sync()
            assert d.digest() == dig


def test_count_field_overflows_inside_the_tile_kernel(gpu):
    """70 000 copies of one 120-mer: the 16-bit count field wraps in LDS and the rest goes to the side table"""
    k, n = 120, 70000
    read = uniform(7, k)
    seq = (read + b"N") * n
    with partitioned_table(gpu, k, 15, True) as t:
        assert t.info.val_len == 16
        t.count_ascii(seq[: len(seq) // 2 // (k + 1) * (k + 1)])
        t.count_ascii(seq[len(seq) // 2 // (k + 1) * (k + 1):])
        t.sync()
        keys, cnt = oracle(read, k, True)
        vals, found = t.lookup(keys)
        assert found.all() and vals.tolist() == [n]
        st = t.stats()
        assert (st.distinct, st.total, st.max_count) == (1, n, n)
        c = t.counters()
        assert c["tile_nword"] >= 1 and c["ovf_used"] == 1


def test_a_repeated_read_overflows_its_bucket_regions(gpu, monkeypatch):
    """one read over and over: its 51 k-mers fill 51 bucket regions, what those cannot take is claimed in the table (the
    NWordDirect route).  No head-room over the mean (JFGPU_P1_SLACK = -1): a region is the reservations the workgroups may
    strand, 64 items each, which 40 000 copies of a k-mer pass on any device of up to 300 CUs."""
    k, lsize = 100, 21
    monkeypatch.setenv("JFGPU_P1_SLACK", "-1")
    read = uniform(11, 150) + b"N"
    seq = read * 40000
    keys, cnt = oracle(seq, k, False)
    with partitioned_table(gpu, k, lsize, False) as t:
        t.count_ascii(seq)
        t.count_ascii(seq)
        t.sync()
        c = t.counters()
        assert c["direct"] > 0 and c["tile_nword"] >= 1 and c["full"] == 0
        check_against_oracle(gpu, t, keys, 2 * cnt)


def test_growth_re_makes_the_partition_geometry(gpu):
    k = 65
    seq = uniform(3, 30000)
    keys, cnt = oracle(seq, k, True)
    with partitioned_table(gpu, k, 12, True, growth=True) as t:
        for a in range(0, len(seq), 6000):
            t.count_ascii(seq[max(0, a - (k - 1)): a + 6000])
        t.sync()
        assert t.refresh_info().lsize >= 14                # (doubled at least twice)
        assert t.counters()["tile_nword"] >= 2
        check_against_oracle(gpu, t, keys, cnt)
        assert t.digest() == gpu.digest_of(keys, cnt)


def test_pending_items_are_flushed_before_a_read_out(gpu):
    k = 97
    a, b = uniform(21, 3000), uniform(22, 3000)
    with partitioned_table(gpu, k, 14, True) as t:
        t.count_ascii(a)
        ka, ca = oracle(a, k, True)
        vals, found = t.lookup(ka)                       # (no sync: the look-up itself applies what is pending)
        assert found.all() and np.array_equal(np.asarray(vals, dtype=np.uint64), ca)
        t.count_ascii(b)
        t.count_ascii(a)
        kb, cb = oracle(a + b"N" + b + b"N" + a, k, True)
        vals, found = t.lookup(kb)
        assert found.all() and np.array_equal(np.asarray(vals, dtype=np.uint64), cb)
        assert t.counters()["tile_nword"] >= 2


def test_attach_bloom_and_set_operation_after_pending_items(gpu):
    """what is pending belongs to the plain COUNT: it is applied before a filter is attached or the operation changes, and
    from then on the direct kernel inserts (the cases that stay on it)"""
    k = 100
    a, b = uniform(31, 4000), uniform(32, 4000)
    ka, ca = oracle(a, k, True)
    exp_a = {tuple(r): int(c) for r, c in zip(ka.tolist(), ca.tolist())}
    with gpu.Bloom(k, gpu.opt_m(0.001, 10000), gpu.opt_k(0.001)) as bl:
        bl.insert_ascii(b)
        bl.insert_ascii(b)
        bl.sync()
        with partitioned_table(gpu, k, 15, True) as t:
            t.count_ascii(a)
            t.attach_bloom(bl)
            before = t.counters()["tile_nword"]
            assert before >= 1
            t.count_ascii(b)                             # every k-mer of b is in the counter twice: all admitted
            t.sync()
            assert t.counters()["tile_nword"] == before
            kab, cab = oracle(a + b"N" + b, k, True)
            check_against_oracle(gpu, t, kab, cab)
            t.attach_bloom(None)
    with partitioned_table(gpu, k, 15, True) as t:
        t.count_ascii(a)
        t.set_operation(2)                               # UPDATE: only keys that are there
        before = t.counters()["tile_nword"]
        assert before >= 1
        t.count_ascii(a[: len(a) // 2] + b"N" + b)
        t.sync()
        assert t.counters()["tile_nword"] == before
        kh, ch = oracle(a[: len(a) // 2], k, True)
        exp = dict(exp_a)
        for r, c in zip(kh.tolist(), ch.tolist()):
            exp[tuple(r)] += int(c)
        vals, found = t.lookup(ka)
        assert found.all() and vals.tolist() == [exp[tuple(r)] for r in ka.tolist()]
        assert t.stats().distinct == len(ka)


def test_auto_mode_keeps_small_batches_on_the_direct_kernel(gpu):
    """AUTO takes the partitioned path only for device batches of 1 GiB and more (profiles/nword_part_rate.txt): everything a
    test feeds stays on the direct kernel, as before the path existed"""
    k = 100
    a, b = uniform(41, 5000), uniform(42, 5000)
    keys, cnt = oracle(a + b"N" + b, k, True)
    with gpu.Table(k, 1 << 15, canonical=True) as t:
        t.set_growth(False)
        feed(t, [a, b])
        t.sync()
        c = t.counters()
        assert c["tile_nword"] == 0 and c["p1_other"] == 0
        check_against_oracle(gpu, t, keys, cnt)
