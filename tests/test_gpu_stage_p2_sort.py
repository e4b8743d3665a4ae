"""The sort-based P2 ALONE, both schemes, at the three item widths the host launches (4, 8 and 16 bytes), through
tests/kernels/stage_harness.hip (jfkt_p2_sort):

  scheme 0, single pass   p2_granule_kernel<ITEM, recording DIRECT, PER> on grid (4, nbk), then granule_finish_kernel (once:
                          granule_finish_range_kernel over a sub-range)
  scheme 1, exact         p2_kernel<ITEM, false>, scan_matrix_kernel, p2_scatter_sorted_kernel<ITEM, PER>, 32 workgroups a bucket

Items are made here in numpy as pairs of 64-bit words (low, high); an item's destination is
D = bucket * 2^b2e + ((item >> tag_bits) & (2^b2e - 1)).  A segment is what a pending batch is to part_flush_t: sh = 1, a
granule batch (a region per bucket given by a (begin, end) pair, all-ones entries are holes, a run of holes at its tail), or
sh = 0, an exact batch (packed, every entry an item -- the all-ones one too).

Scheme 0, per launched destination D:
  * the non-hole entries of out[D cap, off2 end) plus the recorded DIRECT calls of D are D's input items, as multisets;
  * off2[D] = (D cap, D cap + used), used = cap - gshort[D] if gshort[D] else min(gcur[D], cap) (granule_finish_kernel);
    every entry in front of `used` was written (item or hole), none behind it;
  * gcur[D] is a multiple of kGran; gshort[D] != 0 only where gcur[D] > cap (a reservation was refused), and a destination
    whose reservations all fitted has no DIRECT call except for an all-ones item;
  * the direct counter equals the number of recorded calls;
  * destinations of buckets that were not launched keep the sentinel, and zero cursors.
Scheme 1:
  * goff is the exclusive prefix of the per-destination counts from base[bucket] on, bucket by bucket, and the entry behind a
    bucket's last destination is its end;
  * tmp[goff[D], goff[D + 1]) is D's multiset, no hole among it;
  * nothing is written outside the launched buckets' ranges."""
import numpy as np
import pytest

import stage_harness
from stage_harness import M64

pytestmark = pytest.mark.gpu

SENT = {4: 0x5EA5EA5E, 8: 0x5EA5EA5E5EA5EA5E, 16: (0x5EA5EA5E5EA5EA5E << 64) | 0x0123456789ABCDEF}
PER0 = {4: "kP2PairPer", 8: "kP2MidPer", 16: "kP2WidePer"}
PER1 = {4: "16", 8: "14", 16: "7"}
TYPE = {4: "uint32_t", 8: "uint64_t", 16: "u128"}


@pytest.fixture(scope="module")
def kt(gpu):
    return stage_harness.load()


@pytest.fixture(scope="module")
def table(kt):
    t = kt.capi.Table(14, 1 << 16, canonical=False)          # (the launches take its stream and nothing else)
    yield t
    t.close()


# ---- items as (low, high) word arrays ------------------------------------------------------------------------------------
def width_mask(wb):
    return (np.uint64(M64 if wb >= 8 else 0xFFFFFFFF), np.uint64(M64 if wb == 16 else 0))


def put_field(lo, hi, d, tag_bits, b2e):
    m = ((1 << b2e) - 1) << tag_bits
    lo &= np.uint64(~m & M64)
    hi &= np.uint64((~m >> 64) & M64)
    d = d.astype(np.uint64)
    if tag_bits < 64:
        lo |= d << np.uint64(tag_bits)
        if tag_bits + b2e > 64:
            hi |= d >> np.uint64(64 - tag_bits)
    else:
        hi |= d << np.uint64(tag_bits - 64)


def dest_of(lo, hi, tag_bits, b2e):
    if tag_bits >= 64:
        v = hi >> np.uint64(tag_bits - 64)
    else:
        v = lo >> np.uint64(tag_bits)
        if tag_bits + b2e > 64:
            v = v | (hi << np.uint64(64 - tag_bits))
    return v & np.uint64((1 << b2e) - 1)


def items(rng, n, wb, b2e, tag_bits, dest=None):
    """n random items of wb bytes, never the hole and never the sentinel; dest: all of them into one sub-bucket"""
    ml, mh = width_mask(wb)
    lo = rng.integers(0, 1 << 64, n, dtype=np.uint64) & ml
    hi = rng.integers(0, 1 << 64, n, dtype=np.uint64) & mh
    d = rng.integers(0, 1 << b2e, n) if dest is None else np.full(n, dest)
    put_field(lo, hi, d, tag_bits, b2e)
    bad = ((lo == ml) & (hi == mh)) | ((lo == np.uint64(SENT[wb] & M64)) & (hi == (np.uint64(SENT[wb] >> 64) & mh)))
    lo[bad] ^= np.uint64(1 if tag_bits > 0 else 1 << b2e)
    return np.stack([lo, hi], axis=1)


def native(w, wb):
    w = np.asarray(w, dtype=np.uint64).reshape(-1, 2)
    return w[:, 0].astype(np.uint32) if wb == 4 else np.ascontiguousarray(w[:, 0]) if wb == 8 else np.ascontiguousarray(w)


def words(a, wb):
    """what came back, as (n, 2) words"""
    if wb == 16:
        return np.asarray(a, dtype=np.uint64).reshape(-1, 2)
    a = np.asarray(a).astype(np.uint64)
    return np.stack([a, np.zeros_like(a)], axis=1)


def is_value(w, v):
    return (w[..., 0] == np.uint64(v & M64)) & (w[..., 1] == np.uint64(v >> 64))


def hole_of(wb):
    return (1 << (8 * wb)) - 1


EMPTY = np.zeros((0, 2), dtype=np.uint64)


def build(rng, wb, kinds, buckets, nb1):
    """kinds[s]: sh of segment s; buckets[j][s]: the items (n, 2) of bucket j in segment s.  Returns the harness's segments."""
    ml, mh = width_mask(wb)
    hole = np.array([[ml, mh]], dtype=np.uint64)
    segs = []
    for s, sh in enumerate(kinds):
        parts, off, at = [], [], 0
        for j in range(nb1):
            it = buckets.get(j, [EMPTY] * len(kinds))[s]
            if sh == 1:
                parts.append(np.full((3, 2), 12345, dtype=np.uint64) & np.array([ml, mh])); at += 3      # (entries of no bucket between the regions)
                if len(it):
                    n = len(it) + len(it) // 32 + 1
                    e = np.repeat(hole, n + 5, axis=0)                # holes sprinkled in, and a run of five at the tail
                    e[np.sort(rng.choice(n, len(it), replace=False))] = it
                    it = e
                off += [at, at + len(it)]
            else:
                off += [at]
            parts.append(it); at += len(it)
        if sh == 0:
            off += [at]
        segs.append((native(np.concatenate(parts), wb), np.array(off, dtype=np.uint64), sh))
    return segs


def expected_rows(buckets, bucket0, nbk, tag_bits, b2e):
    """(D, low, high) of every item of the launched buckets, sorted"""
    rows = []
    for j in range(bucket0, bucket0 + nbk):
        for it in buckets.get(j, []):
            if len(it):
                d = (np.uint64(j << b2e) | dest_of(it[:, 0], it[:, 1], tag_bits, b2e))
                rows.append(np.stack([d, it[:, 0], it[:, 1]], axis=1))
    rows = np.concatenate(rows) if rows else np.zeros((0, 3), dtype=np.uint64)
    return rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]


def sort_rows(rows):
    return rows[np.lexsort((rows[:, 2], rows[:, 1], rows[:, 0]))]


def ample_cap(kt, exp, n_dest):
    """the fullest destination, plus the reservation each of the four workgroups may strand"""
    gran = kt.const["kGran"]
    most = int(np.bincount(exp[:, 0].astype(np.int64), minlength=1).max()) if len(exp) else 0
    return (most + 4 * gran + gran - 1) // gran * gran


def run_scheme0(kt, table, wb, b2e, tag_bits, kinds, buckets, bucket0, nbk, cap=None, finish_range=None, all_ones=0):
    gran = kt.const["kGran"]
    nb1 = bucket0 + nbk + 1                                   # (a bucket behind the launched ones, with items of its own)
    n_dest = nb1 << b2e
    exp = expected_rows(buckets, bucket0, nbk, tag_bits, b2e)
    ample = cap is None
    if ample:
        cap = ample_cap(kt, exp, n_dest)
    segs = build(np.random.default_rng(len(exp)), wb, kinds, buckets, nb1)
    r = kt.p2_sort(table, 0, wb, b2e, tag_bits, segs, bucket0, nbk, n_dest, SENT[wb], cap=cap, finish_range=finish_range, rec_cap=max(1 << 12, 2 * len(exp)))
    assert r["launched"] == "p2_granule_kernel<%s,RecordDirectT<%s>,%s>+%s" % (
        TYPE[wb], TYPE[wb], PER0[wb], "granule_finish_range_kernel" if finish_range else "granule_finish_kernel")
    out = words(r["out"], wb).reshape(n_dest, cap, 2)
    gcur, gshort, off2, rec = r["gcur"].astype(np.int64), r["gshort"].astype(np.int64), r["off2"], r["rec"]
    d0, d1 = bucket0 << b2e, (bucket0 + nbk) << b2e
    launched = np.zeros(n_dest, dtype=bool); launched[d0:d1] = True
    # outside the launch
    assert is_value(out[~launched], SENT[wb]).all(), "a region of a bucket that was not launched was written"
    assert (gcur[~launched] == 0).all() and (gshort[~launched] == 0).all()
    # cursors, notes, bounds
    assert (gcur % gran == 0).all()
    used = np.where(gshort > 0, cap - gshort, np.minimum(gcur, cap))
    assert (gshort <= cap).all() and (gcur[gshort > 0] > cap).all(), "an overflow note where every reservation fitted"
    fin = np.zeros(n_dest, dtype=bool)
    if finish_range:
        fin[finish_range[0]:finish_range[0] + finish_range[1]] = True
    else:
        fin[:] = True
    D = np.arange(n_dest, dtype=np.int64)
    assert (off2[fin, 0] == (D * cap)[fin].astype(np.uint64)).all() and (off2[fin, 1] == (D * cap + used)[fin].astype(np.uint64)).all()
    assert (off2[~fin] == np.uint64(M64)).all(), "bounds written outside the range asked for"
    col = np.arange(cap)[None, :]
    sent = is_value(out, SENT[wb])
    assert not sent[col < used[:, None]].any(), "a reservation was handed out and left as it was (neither items nor holes)"
    assert sent[col >= used[:, None]].all(), "an entry behind the region's end"
    # the multiset
    stored = (col < used[:, None]) & ~is_value(out, hole_of(wb))
    rows_d, rows_c = np.nonzero(stored)
    got = np.stack([rows_d.astype(np.uint64), out[rows_d, rows_c, 0], out[rows_d, rows_c, 1]], axis=1)
    assert r["n_rec"] == len(rec) == r["ctr_direct"], "direct counter %d, recorded calls %d" % (r["ctr_direct"], r["n_rec"])
    got = sort_rows(np.concatenate([got, rec]))
    assert len(got) == len(exp), "%d items in, %d out (%d direct calls)" % (len(exp), len(got), len(rec))
    assert (got == exp).all()
    # who called DIRECT
    rec_hole = is_value(rec[:, 1:], hole_of(wb)) if len(rec) else np.zeros(0, dtype=bool)
    assert int(rec_hole.sum()) == all_ones
    by_dest = np.bincount(rec[~rec_hole, 0].astype(np.int64), minlength=n_dest) if len(rec) else np.zeros(n_dest, dtype=np.int64)
    assert (by_dest[gcur <= cap] == 0).all(), "a DIRECT call for a destination whose reservations all fitted"
    assert (by_dest[gcur > cap] > 0).all(), "a refused reservation without a DIRECT call"
    if ample:
        assert (gcur <= cap).all() and len(rec) == all_ones
    r["cap"] = cap
    return r


def run_scheme1(kt, table, wb, b2e, tag_bits, kinds, buckets, bucket0, nbk, pair=False):
    nb1 = bucket0 + nbk + 1
    nb, n_dest = 1 << b2e, nb1 << b2e
    exp = expected_rows(buckets, bucket0, nbk, tag_bits, b2e)
    tot = [sum(len(it) for it in buckets.get(j, [])) for j in range(nb1)]          # (bucket_tot of part_flush_t: items, not holes)
    base = np.concatenate([[0], np.cumsum(tot)[:-1]]).astype(np.uint64)
    n_out = int(sum(tot)) + 100
    segs = build(np.random.default_rng(len(exp) + 1), wb, kinds, buckets, nb1)
    r = kt.p2_sort(table, 1, wb, b2e, tag_bits, segs, bucket0, nbk, n_dest, SENT[wb], pair=pair, base=base, n_out=n_out)
    assert r["launched"] == "p2_kernel<%s,false>+scan_matrix_kernel+p2_scatter_sorted_kernel<%s,%s>" % (TYPE[wb], TYPE[wb], "kP2PairPer" if pair else PER1[wb])
    assert r["n_rec"] == 0 and r["ctr_direct"] == 0
    out, goff = words(r["out"], wb), r["goff"]
    d0, d1 = bucket0 << b2e, (bucket0 + nbk) << b2e
    counts = np.bincount(exp[:, 0].astype(np.int64), minlength=n_dest)
    want = np.full(n_dest + 1, M64, dtype=np.uint64)
    for j in range(bucket0, bucket0 + nbk):
        c = counts[j << b2e:(j + 1) << b2e]
        want[j << b2e:((j + 1) << b2e) + 1] = int(base[j]) + np.concatenate([[0], np.cumsum(c)])
    assert (goff == want).all(), "goff is not the exclusive prefix of the destinations' counts from base on"
    lo_, hi_ = int(goff[d0]), int(goff[d1])
    assert is_value(out[:lo_], SENT[wb]).all() and is_value(out[hi_:], SENT[wb]).all(), "an entry outside the launched buckets' ranges"
    dest = np.repeat(np.arange(d0, d1, dtype=np.uint64), counts[d0:d1])
    got = sort_rows(np.stack([dest, out[lo_:hi_, 0], out[lo_:hi_, 1]], axis=1))
    assert len(got) == len(exp) and (got == exp).all(), "a destination's range does not hold its multiset"
    return r


def run(kt, table, scheme, wb, b2e, tag_bits, kinds, buckets, bucket0, nbk, **kw):
    if scheme == 0:
        return run_scheme0(kt, table, wb, b2e, tag_bits, kinds, buckets, bucket0, nbk, **kw)
    return run_scheme1(kt, table, wb, b2e, tag_bits, kinds, buckets, bucket0, nbk, pair=kw.get("pair", False))


def top_tag(wb, b2e):
    """the sub-bucket in the item's top bits: the widest item the host makes (for 16 bytes tag_full goes up to 110)"""
    return {4: 32 - b2e, 8: 64 - b2e, 16: 110}[wb]


def low_tag(wb):
    """... and the narrowest tags: a full-size tile and no remainder bits (+ 1 for a pair of tiles); 76 = 13 + 63 for two words"""
    return {4: 14, 8: 30, 16: 76}[wb]


WIDTHS = (4, 8, 16)


# ---- the shapes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b2e", (1, 5, 10))
@pytest.mark.parametrize("scheme", (0, 1))
@pytest.mark.parametrize("wb", WIDTHS)
def test_forty_thousand_items_in_one_granule_segment(kt, table, wb, scheme, b2e):
    """each of the four workgroups of scheme 0 gets 10 000 entries: for 16-byte items one full chunk of 7168 (the unconditional
    prefetch, its holes among the items) and a partial one; 2, 32 and 1024 destinations; the sub-bucket in the item's top bits
    and right above the narrowest tag"""
    rng = np.random.default_rng(100 * wb + b2e)
    for tag_bits in (top_tag(wb, b2e), low_tag(wb)):
        buckets = {2: [items(rng, 40000, wb, b2e, tag_bits)], 0: [items(rng, 50, wb, b2e, tag_bits)], 3: [items(rng, 70, wb, b2e, tag_bits)]}
        run(kt, table, scheme, wb, b2e, tag_bits, [1], buckets, 2, 1)


@pytest.mark.parametrize("scheme", (0, 1))
@pytest.mark.parametrize("wb", WIDTHS)
def test_a_chunk_that_straddles_a_granule_and_an_exact_segment(kt, table, wb, scheme):
    """20 000 + 20 000: the granule segment's holes end where the exact segment's items begin, inside a workgroup's chunk
    (load_chunk's two parts; for 16-byte items the prefetch falls back to it)"""
    rng = np.random.default_rng(200 + wb)
    b2e, tag_bits = 5, top_tag(wb, 5)
    for kinds in ([1, 0], [0, 1]):
        buckets = {2: [items(rng, 20000, wb, b2e, tag_bits), items(rng, 20000, wb, b2e, tag_bits)], 1: [items(rng, 9, wb, b2e, tag_bits), EMPTY]}
        run(kt, table, scheme, wb, b2e, tag_bits, kinds, buckets, 2, 1)


@pytest.mark.parametrize("scheme", (0, 1))
@pytest.mark.parametrize("wb", WIDTHS)
def test_three_buckets_an_empty_one_between_two_full_ones_and_a_bucket_of_one_item(kt, table, wb, scheme):
    """nbk = 3 from bucket 2 on; scheme 0's bounds once by granule_finish_range_kernel over the last two buckets' destinations"""
    rng = np.random.default_rng(300 + wb)
    b2e, tag_bits = 5, low_tag(wb)
    mk = lambda n: items(rng, n, wb, b2e, tag_bits)
    buckets = {0: [mk(20), mk(3)], 2: [mk(9000), mk(500)], 3: [EMPTY, EMPTY], 4: [mk(3000), mk(5000)], 5: [mk(11), mk(12)]}
    run(kt, table, scheme, wb, b2e, tag_bits, [1, 0], buckets, 2, 3)
    if scheme == 0:
        run_scheme0(kt, table, wb, b2e, tag_bits, [1, 0], buckets, 2, 3, finish_range=(3 << b2e, 2 << b2e))
    buckets = {2: [mk(1), EMPTY], 3: [mk(300), mk(1)], 4: [EMPTY, EMPTY]}
    run(kt, table, scheme, wb, b2e, tag_bits, [1, 0], buckets, 2, 3)
    buckets = {2: [EMPTY, mk(1)], 3: [EMPTY, EMPTY], 4: [mk(2), EMPTY]}
    run(kt, table, scheme, wb, b2e, tag_bits, [0, 1], buckets, 2, 3)


@pytest.mark.parametrize("wb", WIDTHS)
def test_regions_of_one_and_two_reservations(kt, table, wb):
    """all 3000 items of a bucket in one destination, regions of kGran and 2 kGran items: reservations are refused, the
    overflow note is set, what does not fit is handed to DIRECT -- and the exact scheme puts the 3000 in one range"""
    rng = np.random.default_rng(400 + wb)
    b2e, tag_bits = 5, top_tag(wb, 5)
    gran = kt.const["kGran"]
    buckets = {2: [items(rng, 1500, wb, b2e, tag_bits, dest=7), np.concatenate([items(rng, 1500, wb, b2e, tag_bits, dest=7), items(rng, 40, wb, b2e, tag_bits)])]}
    for cap in (gran, 2 * gran):
        r = run_scheme0(kt, table, wb, b2e, tag_bits, [1, 0], buckets, 2, 1, cap=cap)
        assert r["n_rec"] >= 3000 - cap and r["gcur"][(2 << b2e) + 7] > cap
    # uniform items into regions of two reservations: some destinations are refused, some are not
    buckets = {2: [items(rng, 32 * 2 * gran, wb, b2e, tag_bits)]}
    r = run_scheme0(kt, table, wb, b2e, tag_bits, [1], buckets, 2, 1, cap=2 * gran)
    assert r["n_rec"] > 0
    run_scheme1(kt, table, wb, b2e, tag_bits, [1, 0], {2: [items(rng, 1500, wb, b2e, tag_bits, dest=7), items(rng, 1500, wb, b2e, tag_bits, dest=7)]}, 2, 1)


def test_the_all_ones_item_of_an_exact_segment(kt, table):
    """4-byte items only: an exact batch stores the all-ones item like any other.  The single-pass kernel hands it to DIRECT
    (in a region it would read as a hole), the exact scheme stores it in its destination's range."""
    rng = np.random.default_rng(500)
    b2e, tag_bits = 5, 27
    ones = np.array([[0xFFFFFFFF, 0]], dtype=np.uint64)
    exact = np.concatenate([items(rng, 700, 4, b2e, tag_bits), ones, items(rng, 800, 4, b2e, tag_bits)])
    buckets = {2: [items(rng, 2000, 4, b2e, tag_bits), exact]}
    r = run_scheme0(kt, table, 4, b2e, tag_bits, [1, 0], buckets, 2, 1, all_ones=1)
    assert r["n_rec"] == 1 and int(r["rec"][0, 0]) == (2 << b2e) + 31
    run_scheme1(kt, table, 4, b2e, tag_bits, [1, 0], buckets, 2, 1)
    run_scheme1(kt, table, 4, b2e, tag_bits, [1, 0], buckets, 2, 1, pair=True)


@pytest.mark.parametrize("scheme", (0, 1))
def test_pairs_of_tiles_take_chunks_of_28_ki_items(kt, table, scheme):
    """4-byte items, 120 000 of a bucket: scheme 0's workgroups get a full chunk of 28 672 entries and a partial one; the exact
    scheme's scatter in the instantiation for pairs of tiles does with 32 workgroups what the one of 16 items a lane does"""
    rng = np.random.default_rng(600)
    b2e, tag_bits = 9, 14
    buckets = {2: [items(rng, 90000, 4, b2e, tag_bits), items(rng, 30000, 4, b2e, tag_bits)]}
    if scheme == 0:
        run_scheme0(kt, table, 4, b2e, tag_bits, [1, 0], buckets, 2, 1)
    else:
        run_scheme1(kt, table, 4, b2e, tag_bits, [1, 0], buckets, 2, 1, pair=True)


def test_the_harness_refuses_what_the_kernels_cannot_take(kt, table):
    """2048 destinations a bucket are beyond the single-pass kernel (one destination per thread, GranuleLds of kGranMaxB
    entries): the host takes the exact scheme there, and the harness does not launch it"""
    rng = np.random.default_rng(700)
    buckets = {0: [items(rng, 10, 8, 11, 40)]}
    segs = build(rng, 8, [1], buckets, 1)
    with pytest.raises(kt.capi.JfgpuError):
        kt.p2_sort(table, 0, 8, 11, 40, segs, 0, 1, 1 << 11, SENT[8], cap=64)
