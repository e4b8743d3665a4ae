"""One stage at a time of the partitioned insert of three- and four-word keys (kernels_nword_part.hip.hpp), through the
harness of tests/kernels/stage_harness_nword.hip:

  P1n  the multiset of items per bucket and the hole padding equal what Python derives from the oracle's k-mers and the
       table's matrix: item = ((local mod 2^rest_shift) << rem_bits) | (key >> lsize), bucket = local >> rest_shift
  P2   every item lands in its tile's segment, holes stay holes (k = 100 at 2^22 slots)
  Tn   hand-picked item lists -- duplicates, probe sequences that wrap the tile end, items that differ only in lo2 or only
       in the hi word, a full tile plus one item, a preloaded tile with counts at cnt_max - 1 -- read back by look-up."""
import random

import numpy as np
import pytest

import oracle_lib as O
import stage_harness_nword as SH

pytestmark = pytest.mark.gpu

LUT = np.frombuffer(b"ACGT", dtype=np.uint8)
SENTINEL = 0x1234567890ABCDEF1122334455667788AABBCCDDEEFF00110F0E0D0C0B0A0908


def uniform(seed, n):
    return LUT[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


@pytest.fixture(scope="module")
def H(gpu):
    return SH.load()


def key_int(row):
    return sum(int(w) << (64 * q) for q, w in enumerate(row))


def key_rows(ints, nw):
    return np.array([[(x >> (64 * q)) & SH.M64 for q in range(nw)] for x in ints], dtype=np.uint64).reshape(-1, nw)


def table_of(H, k, lsize, canonical=True):
    t = H.capi.Table(k, 1 << lsize, canonical=canonical)
    t.set_growth(False)
    g = H.geom(t)
    assert g["lsize_l"] == lsize and g["item256"] and g["part_ok"] and g["tag_full"] == g["tile_bits"] + g["rem_bits"]
    return t, g


def positions(t, g, keys):
    return [int(p) for p in O.matrix_times(t.matrix(), g["lsize_g"], g["key_bits"], keys)]


def item_of(g, b1, key, local):
    """(bucket, item) of a k-mer: make_item_nword restated"""
    rest_shift = g["lsize_l"] - b1
    return local >> rest_shift, ((local & ((1 << rest_shift) - 1)) << g["rem_bits"]) | (key >> g["lsize_g"])


def multiset(xs):
    d = {}
    for x in xs:
        d[x] = d.get(x, 0) + 1
    return d


# ---- P1n ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,lsize,b1,canonical", [(65, 12, 1, True), (100, 21, 10, False), (100, 21, 10, True), (65, 13, 2, False)])
def test_p1_items_and_hole_padding(H, k, lsize, b1, canonical):
    reads = [uniform(k + i, 150 + 7 * i) for i in range(40)] + [b"A" * (k + 5), uniform(1, k - 1), uniform(2, k), b"acgtRYn" * 30 + uniform(3, k + 9)]
    buf = b"N".join(reads) + b"N"
    lo = 5
    hi = len(buf) - (len(reads[-1]) // 2)                    # the range ends inside the last read
    assert buf[hi - 1:hi] != b"N" and buf[hi:hi + 1] != b"N"
    kmers = O.extract(buf[lo:hi], k, canonical)              # every occurrence, in order
    t, g = table_of(H, k, lsize, canonical)
    with t:
        assert g["b1"] == b1
        pos = positions(t, g, kmers)
        exp = [dict() for _ in range(1 << b1)]
        for row, p in zip(kmers.tolist(), pos):
            b, it = item_of(g, b1, key_int(row), p)
            exp[b][it] = exp[b].get(it, 0) + 1
        grid, gran = 3, H.const["kGran"]
        cap = (max(sum(e.values()) for e in exp) + grid * gran + gran - 1) // gran * gran
        r = H.p1(t, b1, buf, lo, hi, cap, grid, SENTINEL)
        assert r["launched"].startswith("p1_nword_granule_kernel") and r["mers"] == len(kmers) and r["ctr_direct"] == 0
        for b in range(1 << b1):
            region = SH.from_words(r["out"][b])
            used = int(r["gcur"][b])
            assert used % gran == 0 and used <= cap and r["gshort"][b] == 0
            items = [x for x in region[:used] if x != SH.HOLE256]
            assert multiset(items) == exp[b] and int(r["tot"][b]) == len(items)
            assert all(x == SENTINEL for x in region[used:])              # nothing behind the reservations
            assert SENTINEL not in region[:used]                           # every reserved entry is an item or a hole
        assert all(x == SENTINEL for x in SH.from_words(r["out"][1 << b1]))  # the guard region
        assert t.stats().distinct == 0                                     # nothing went to the table


@pytest.mark.parametrize("k,lsize,b1,cap", [(65, 12, 1, 1088), (100, 21, 10, 64)])
def test_p1_region_overflow_goes_to_the_table(H, k, lsize, b1, cap):
    """regions that take the first round's items and not the rest (a round is 2048 items over 2^b1 buckets)"""
    read = uniform(9, 200)
    buf = (read + b"N") * 40
    kmers = O.extract(buf, k, True)
    keys, cnt = O.count(buf, k, True)
    t, g = table_of(H, k, lsize, True)
    with t:
        assert cap % H.const["kGran"] == 0
        r = H.p1(t, b1, buf, 0, len(buf), cap, 2, SENTINEL)
        assert r["ctr_direct"] > 0 and r["mers"] == len(kmers)
        stored = {}
        for b in range(1 << b1):
            # what granule_finish_kernel makes of the cursors: everything below a reservation that did not fit was handed out
            short = int(r["gshort"][b])
            used = cap - short if short else min(int(r["gcur"][b]), cap)
            for x in SH.from_words(r["out"][b])[:used]:
                if x != SH.HOLE256:
                    stored[(b, x)] = stored.get((b, x), 0) + 1
        assert SENTINEL not in [x for _, x in stored] and sum(stored.values()) > 0
        assert sum(stored.values()) + r["ctr_direct"] == len(kmers) == sum(int(x) for x in r["tot"]) + r["ctr_direct"]
        pos = positions(t, g, keys)
        vals, found = t.lookup(keys)
        for row, p, c, v, f in zip(keys.tolist(), pos, cnt.tolist(), np.asarray(vals).tolist(), np.asarray(found).tolist()):
            in_regions = stored.get(item_of(g, b1, key_int(row), p), 0)
            assert in_regions + (int(v) if f else 0) == c             # what its region could not take is in the table
        t.sync()


# ---- P2 -----------------------------------------------------------------------------------------------------------------
def test_p2_routes_every_item_to_its_tile(H):
    k, lsize = 100, 22
    t, g = table_of(H, k, lsize, True)
    with t:
        b1, b2 = g["b1"], g["b2"]
        assert (b1, b2) == (5, 6)
        keys, _ = O.count(uniform(5, 6000), k, True)
        pos = positions(t, g, keys)
        per = [[] for _ in range(1 << b1)]
        for row, p in zip(keys.tolist(), pos):
            b, it = item_of(g, b1, key_int(row), p)
            per[b].append(it)
        rng = random.Random(5)
        nb = 1 << b1
        # segment 0: packed (an exact batch); segment 1: a granule batch, regions of `cap` items with holes inside and behind
        seg0, off0, seg1, off1 = [], [0], [], []
        cap = 256
        exp = [[] for _ in range(nb << b2)]
        for b in range(nb):
            half = len(per[b]) // 2
            a, c = per[b][:half], per[b][half:] + per[b][:3]            # (three items twice: duplicates travel like any item)
            assert len(c) + 8 <= cap
            seg0 += a; off0.append(len(seg0))
            region = list(c)
            for _ in range(8):
                region.insert(rng.randrange(len(region) + 1), SH.HOLE256)
            off1 += [b * cap, b * cap + len(region)]
            seg1 += region + [SENTINEL] * (cap - len(region))
            for it in a + c:
                exp[(b << b2) | ((it >> g["tag_full"]) & ((1 << b2) - 1))].append(it)
        base, run = [], 0
        for b in range(nb):
            base.append(run); run += sum(len(exp[(b << b2) + d]) for d in range(1 << b2))
        r = H.p2(t, b2, g["tag_full"], [(seg0, off0, 0), (seg1, off1, 1)], 0, nb, nb << b2, base, run + 16, SENTINEL)
        assert "p2_scatter_sorted_kernel<u256" in r["launched"]
        out, goff = SH.from_words(r["out"]), [int(x) for x in r["goff"]]
        assert goff[0] == 0 and goff[-1] == run
        for d in range(nb << b2):
            assert multiset(out[goff[d]:goff[d + 1]]) == multiset(exp[d])
        assert SH.HOLE256 not in out[:run]
        assert all(x == SENTINEL for x in out[run:])


# ---- Tn -----------------------------------------------------------------------------------------------------------------
class Pool:
    """k-mers of a random sequence with their positions in a small table: what hand-made item lists are picked from"""
    def __init__(self, H, k, lsize, n, seed):
        self.t, self.g = table_of(H, k, lsize, True)
        self.keys, _ = O.count(uniform(seed, n), k, True)
        self.pos = positions(self.t, self.g, self.keys)
        self.tile_bits = self.g["tile_bits"]

    def item(self, i):
        return item_of(self.g, 0, key_int(self.keys[i]), self.pos[i] & ((1 << self.tile_bits) - 1))[1]

    def by_tile(self, tile):
        return [i for i, p in enumerate(self.pos) if p >> self.tile_bits == tile]


def run_tile(H, P, tile, lists, grid=1):
    """lists: item lists, one segment each, all for `tile`; segment s alternates between the packed and the granule format"""
    n_tiles = 1 << (P.g["lsize_l"] - P.tile_bits)
    segs = []
    for s, items in enumerate(lists):
        if s % 2 == 0:
            off = [0] * (tile + 1) + [len(items)] * (n_tiles - tile)
            segs.append((list(items) or [SENTINEL], off, 0))
        else:
            body = [SH.HOLE256] + list(items) + [SH.HOLE256, SH.HOLE256]
            off = []
            for u in range(n_tiles):
                off += [0, len(body)] if u == tile else [0, 0]
            segs.append((body, off, 1))
    return H.tile(P.t, segs, tile0=0, n_units=n_tiles, grid=grid)


def looked_up(P, idx):
    vals, found = P.t.lookup(P.keys[idx])
    return [int(v) if f else None for v, f in zip(np.asarray(vals).tolist(), np.asarray(found).tolist())]


def test_tile_duplicates_wraps_and_near_twins(H):
    k, lsize = 100, 12
    P = Pool(H, k, lsize, 30000, 12)
    with P.t:
        mask = (1 << P.tile_bits) - 1
        tile1 = P.by_tile(1)
        # duplicates of one item; items whose probe sequences start at the tile's last slots and wrap; a crowd on one idx0
        dup = tile1[0]
        last = [i for i in tile1 if (P.pos[i] & mask) >= mask - 2][:12]
        crowd_at = P.pos[tile1[5]] & mask
        crowd = [i for i in tile1 if (P.pos[i] & mask) == crowd_at]
        assert len(last) >= 6 and len(crowd) >= 2
        chosen = sorted(set([dup] + last + crowd))
        mult = {i: 1 + (j % 3) for j, i in enumerate(chosen)}
        mult[dup] = 500
        a, b, c = [], [], []
        for i in chosen:
            for m in range(mult[i]):
                (a, b, c)[m % 3].append(P.item(i))
        r = run_tile(H, P, 1, [a, b, c])
        assert r["launched"].startswith("tile_insert_nword_kernel") and r["full"] == 0
        assert looked_up(P, chosen) == [mult[i] for i in chosen]
        assert P.t.stats().distinct == len(chosen)
        P.t.sync()


def test_tile_items_that_differ_in_one_slot_word(H):
    """keys that share everything above the table's bits (the whole remainder) and differ in their position alone: their tags
    differ only in idx0, which lies in lo2's top bit (bit 0 of idx0) and in the hi word (the rest) at this geometry"""
    k, lsize = 100, 12
    t, g = table_of(H, k, lsize, True)
    with t:
        assert g["rem_bits"] == 188 and g["tag_bits"] == 10      # tag bits 126 .. 188 are lo2, 189 .. 198 the hi word's
        base = key_int(O.count(uniform(77, k), k, False)[0][0])
        variants = [(base >> lsize << lsize) | v for v in range(1 << lsize)]
        keys = key_rows(variants, 4)
        pos = positions(t, g, keys)
        tile0 = [i for i, p in enumerate(pos) if p >> g["tile_bits"] == 0]
        idx = {pos[i] & 2047: i for i in tile0}
        pairs_lo2 = [(idx[x], idx[x ^ 1]) for x in idx if x % 2 == 0 and (x ^ 1) in idx][:6]
        pairs_hi = [(idx[x], idx[x ^ 0x400]) for x in idx if x < 0x400 and (x ^ 0x400) in idx][:6]
        assert pairs_lo2 and pairs_hi
        chosen = sorted({i for p in pairs_lo2 + pairs_hi for i in p})
        items = []
        for j, i in enumerate(chosen):
            items += [item_of(g, 0, variants[i], pos[i] & 2047)[1]] * (j + 1)
        for a, b in pairs_lo2:
            ia, ib = item_of(g, 0, variants[a], pos[a] & 2047)[1], item_of(g, 0, variants[b], pos[b] & 2047)[1]
            assert ia ^ ib == 1 << 188
        random.Random(1).shuffle(items)
        n_tiles = 1 << (lsize - g["tile_bits"])
        r = H.tile(t, [(items, [0] + [len(items)] * n_tiles, 0)], tile0=0, n_units=n_tiles, grid=2)
        assert r["full"] == 0
        vals, found = t.lookup(keys[chosen])
        assert np.asarray(found).all() and np.asarray(vals).tolist() == [j + 1 for j in range(len(chosen))]
        assert t.stats().distinct == len(chosen)


def test_tile_filled_to_the_last_slot_and_one_more(H):
    """2048 items with 2048 different home slots fill tile 0 whatever the order of the claims; one more item then finds no
    free slot within its max_probe + 1 = 1024 probes: CTR_FULL reads 1 and the item is not in the table"""
    k, lsize = 65, 12
    P = Pool(H, k, lsize, 60000, 65)
    with P.t:
        assert P.g["max_probe"] == 1023
        mask = (1 << P.tile_bits) - 1
        home = {}
        for i in P.by_tile(0):
            home.setdefault(P.pos[i] & mask, i)
        assert len(home) == 2048
        placed = list(home.values())
        taken = set(placed)
        extra = next(i for i in P.by_tile(0) if i not in taken)
        random.Random(2).shuffle(placed)
        r = run_tile(H, P, 0, [[P.item(i) for i in placed[:1000]], [P.item(i) for i in placed[1000:]]])
        assert r["full"] == 0
        st = P.t.stats()
        assert st.distinct == 2048 and st.total == 2048
        r = run_tile(H, P, 0, [[P.item(extra), P.item(placed[0])]])      # (the one that is there is still counted)
        assert r["full"] == 1
        assert looked_up(P, [extra, placed[0]]) == [None, 2]
        assert P.t.stats().distinct == 2048


def test_second_flush_into_a_preloaded_tile_overflows_the_count_field(H):
    k, lsize = 120, 15
    P = Pool(H, k, lsize, 4000, 120)
    with P.t:
        assert P.g["cnt_bits"] == 16 and P.g["returning"]
        cnt_max = (1 << 16) - 1
        tile = 3
        some = P.by_tile(tile)[:5]
        assert len(some) == 5
        P.t.add_keys(P.keys[some], val=cnt_max - 1)          # the preload: counts at cnt_max - 1, through the direct kernel
        assert looked_up(P, some) == [cnt_max - 1] * 5
        items = []
        for j, i in enumerate(some):
            items += [P.item(i)] * j                         # 0, 1, 2, 3, 4 more: the last three pass cnt_max
        fresh = P.by_tile(tile)[5:9]
        items += [P.item(i) for i in fresh]
        r = run_tile(H, P, tile, [items[::2], items[1::2]])
        assert r["full"] == 0 and r["ovf_used"] == 3
        assert looked_up(P, some) == [cnt_max - 1 + j for j in range(5)]
        assert looked_up(P, fresh) == [1] * 4
        P.t.sync()


def test_items_direct_kernel_of_a_small_flush(H):
    k, lsize = 65, 12
    P = Pool(H, k, lsize, 3000, 6)
    with P.t:
        b1, cap = P.g["b1"], 2048
        assert b1 == 1
        regions, off = [], []
        chosen = []
        for b in range(2):
            idx = P.by_tile(b)[:300]
            chosen += idx
            body = [SH.HOLE256] + [P.item(i) for i in idx] + [P.item(idx[0])]
            off += [b * cap, b * cap + len(body)]
            regions += body + [SENTINEL] * (cap - len(body))
        r = H.tile(P.t, [(regions, off, 1)], kernel="direct", grid=2, cap=cap)
        assert r["launched"].startswith("items_direct_nword_kernel")
        got = looked_up(P, chosen)
        assert got == [2 if j % 300 == 0 else 1 for j in range(len(chosen))]
