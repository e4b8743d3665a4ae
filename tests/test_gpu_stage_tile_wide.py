"""Stage Tw of the two-word partitioned path ALONE: tile_insert_wide_kernel (1 to 3 item arrays), tile_insert_wide_pipe_kernel
(one item array; a unit of more than 8192 items takes several rounds) and items_direct_wide_kernel (one granule batch,
global claims), through tests/kernels/stage_harness.hip (jfkt_tile_wide) on small real tables: k = 40 at 2^17 slots (16
tiles, a count field no add can wrap) and k = 56 at 2^15 slots (4 tiles, a 16-bit count field: RETURNING); k = 63 at 2^29
slots on the device only.

Keys are drawn in numpy as (low, high) words; a key's position is M * key under the table's own matrix (computed here from
matrix(), checked against oracle_lib.matrix_times); its item is make_item_wide restated with the tile's slot index as the
position's part: (pos mod 2^13) << rem_bits | key >> lsize_g, its tile pos >> 13.

The reference is a collections.Counter of the keys, added to what the table held before.  After a launch the table holds
exactly that, judged by the library's own read-back:
  * dump_records: no key twice, (pos, key) order, the Counter (counts saturate at the record's four bytes);
  * lookup finds every key with its exact count, and none of 500 absent keys;
  * stats: distinct, total, max_count;
  * digest equals the digest of a second table that got the same keys through add_key_vals (the global path)."""
import collections
import os

import numpy as np
import pytest

import oracle_lib as O
import stage_harness
from stage_harness import M64

pytestmark = pytest.mark.gpu

ROUND = 8192                                                  # items of a round of the pipelined kernel (8 a lane)
HOLE = np.array([M64, M64], dtype=np.uint64)
KERNELS = ("plain", "pipe")


@pytest.fixture(scope="module")
def kt(gpu):
    return stage_harness.load()


class Geometry:
    def __init__(self, kt, k, lsize, pool, seed, twin=True):
        self.kt, self.k = kt, k
        self.t = kt.capi.Table(k, 1 << lsize, canonical=False)
        self.t.set_growth(False)
        self.t2 = kt.capi.Table(k, 1 << lsize, canonical=False) if twin else None       # the same keys by the global path
        if twin:
            self.t2.set_growth(False)
            assert (self.t2.matrix() == self.t.matrix()).all()
        self.g = kt.geom(self.t)
        g = self.g
        assert g["tile_bits"] == 13 and g["key_bits"] == 2 * k and g["tag_full"] == 13 + g["rem_bits"] and g["b2"] == 0 or not twin
        self.cols = self.t.matrix()
        rng = np.random.default_rng(seed)
        lo = rng.integers(0, 1 << 64, pool, dtype=np.uint64)
        hi = rng.integers(0, 1 << (2 * k - 64), pool, dtype=np.uint64)
        self.keys = np.stack([lo, hi], axis=1)                  # (random keys of 80 bits and more: no two alike)
        self.pos = self.positions(self.keys)
        assert (self.pos[:500] == O.matrix_times(self.cols, g["lsize_g"], 2 * k, self.keys[:500])).all()
        self.tile = (self.pos >> np.uint64(13)).astype(np.int64)

    def positions(self, keys):
        """M * key: column c - 1 - j of the matrix is the image of key bit j"""
        c = 2 * self.k
        pos = np.zeros(len(keys), dtype=np.uint64)
        for j in range(c):
            bit = (keys[:, j >> 6] >> np.uint64(j & 63)) & np.uint64(1)
            pos ^= bit * self.cols[c - 1 - j]
        return pos

    def items(self, keys):
        """(tile, item words) of every key"""
        g, pos = self.g, self.positions(keys)
        rb, ls = g["rem_bits"], g["lsize_g"]
        assert 0 < ls < 64 and rb + 13 <= 128
        kl, kh = keys[:, 0], keys[:, 1]
        lo = (kl >> np.uint64(ls)) | (kh << np.uint64(64 - ls))            # key >> lsize_g
        hi = kh >> np.uint64(ls)
        idx0 = pos & np.uint64(8191)
        if rb >= 64:
            hi = hi | (idx0 << np.uint64(rb - 64))
        else:
            lo = lo | (idx0 << np.uint64(rb))
            hi = hi | (idx0 >> np.uint64(64 - rb))
        it = np.stack([lo, hi], axis=1)
        for i in (0, len(keys) - 1):                           # (the same in Python ints)
            key, p = (int(kh[i]) << 64) | int(kl[i]), int(pos[i])
            want = ((p & 8191) << rb) | (key >> ls)
            assert (int(it[i, 1]) << 64) | int(it[i, 0]) == want
        return (pos >> np.uint64(13)).astype(np.int64), it

    def pool_of(self, tile):
        return self.keys[self.tile == tile]

    def close(self):
        self.t.close()
        if self.t2 is not None:
            self.t2.close()


@pytest.fixture(scope="module")
def g40(kt):
    g = Geometry(kt, 40, 17, 1 << 17, 1); yield g; g.close()


@pytest.fixture(scope="module")
def g56(kt):
    g = Geometry(kt, 56, 15, 1 << 19, 2); yield g; g.close()


def draw(rng, pool, n, distinct):
    """n keys of the pool (with repeats) over at most `distinct` different ones"""
    if n == 0:
        return np.zeros((0, 2), dtype=np.uint64)
    d = pool[rng.choice(len(pool), min(distinct, n, len(pool)), replace=False)]
    return np.concatenate([d, d[rng.integers(0, len(d), n - len(d))]]) if n > len(d) else d


def segment(G, unit_keys, tile0, sh, rng, hole_rate=0.04):
    """one item array of the units' keys: sh = 1 -- (begin, end) pairs, holes inside the ranges, entries of no unit between
    them; sh = 0 -- packed, no holes"""
    parts, off, at = [], [], 0
    for i, keys in enumerate(unit_keys):
        tile, it = G.items(keys) if len(keys) else (np.zeros(0, dtype=np.int64), np.zeros((0, 2), dtype=np.uint64))
        assert (tile == tile0 + i).all(), "a key outside the tile it is stored for"
        if sh == 1:
            if len(it):
                n = len(it) + int(len(it) * hole_rate) + 1
                e = np.tile(HOLE, (n, 1))
                e[np.sort(rng.choice(n, len(it), replace=False))] = it
                it = e
            parts.append(np.full((3, 2), 12345, dtype=np.uint64)); at += 3
            off += [at, at + len(it)]
        else:
            off += [at]
        parts.append(it); at += len(it)
    if sh == 0:
        off += [at]
    return np.concatenate(parts), np.array(off, dtype=np.uint64), sh


def launch(G, kernel, unit_keys, tile0, grid, rng, shs=(1,)):
    """unit_keys[i]: keys (n, 2) of tile tile0 + i, split over len(shs) item arrays (the pipelined kernel takes one)"""
    if kernel == "pipe":
        shs = shs[:1]
    n_seg = len(shs)
    segs = []
    for s, sh in enumerate(shs):
        segs.append(segment(G, [k_[s::n_seg] for k_ in unit_keys], tile0, sh, rng))
    name = G.kt.tile_wide(G.t, kernel, segs, tile0=tile0, n_units=len(unit_keys), grid=grid)
    rt = "true" if G.g["returning"] else "false"
    assert name == ("tile_insert_wide_kernel<%s>" if kernel == "plain" else "tile_insert_wide_pipe_kernel<%s>") % rt
    return name


def count_up(total, keys):
    total.update(map(tuple, keys.tolist()))


def judge(G, counter, rng, twin=True):
    """the table holds exactly `counter` ((low, high) -> count), by every read-back path"""
    t, capi, k = G.t, G.kt.capi, G.k
    t.sync()                                                   # (raises "Hash full" if a kernel gave up on a key)
    exp_k = np.array(sorted(counter, key=lambda x: (x[1], x[0])), dtype=np.uint64).reshape(-1, 2)
    exp_c = np.array([counter[tuple(x)] for x in exp_k.tolist()], dtype=np.uint64)
    keys, cnts = capi.decode_records(t.dump_records(), k, 4)
    keys = keys.reshape(-1, 2)
    assert len(np.unique(keys, axis=0)) == len(keys), "a key is in the table twice"
    assert len(keys) == len(exp_k), "%d keys in the table, %d expected" % (len(keys), len(exp_k))
    pos = G.positions(keys)
    order = np.lexsort((keys[:, 0], keys[:, 1], pos))
    assert (order == np.arange(len(keys))).all(), "the dump is not in (pos, key) order"
    by_key = np.lexsort((keys[:, 0], keys[:, 1]))
    assert (keys[by_key] == exp_k).all() and (cnts[by_key] == np.minimum(exp_c, np.uint64(2 ** 32 - 1))).all()
    if len(exp_k):
        vals, found = t.lookup(exp_k)
        assert found.all(), "%d keys are in the table but not found from their home slot on" % int((~found).sum())
        assert (vals == exp_c).all(), "lookup's counts differ for %d keys" % int((vals != exp_c).sum())
    absent = np.stack([rng.integers(0, 1 << 64, 500, dtype=np.uint64), rng.integers(0, 1 << (2 * k - 64), 500, dtype=np.uint64)], axis=1)
    absent = np.array([x for x in absent.tolist() if tuple(x) not in counter], dtype=np.uint64).reshape(-1, 2)
    _, found = t.lookup(absent)
    assert not found.any()
    st = t.stats()
    assert (st.distinct, st.total, st.max_count) == (len(exp_k), int(exp_c.sum()), int(exp_c.max()) if len(exp_c) else 0)
    if twin:
        G.t2.clear()
        if len(exp_k):
            G.t2.add_key_vals(exp_k, exp_c)
        G.t2.sync()
        assert t.digest() == G.t2.digest()
    else:
        assert t.digest() == capi.digest_of(exp_k, exp_c)


# ---- units of every size, chained by one workgroup in every order --------------------------------------------------------
LAYOUT_A = (0, ROUND + 1, 1, 0, 2 * ROUND + 5, ROUND - 1, 0)
LAYOUT_B = (ROUND, 0, 0, 2 * ROUND + 5, ROUND, 1, 5000)


@pytest.mark.parametrize("grid", (1, 2, 3, 7))
@pytest.mark.parametrize("kernel", KERNELS)
def test_seven_units_chained_over_clean_dirty_empty_and_multi_round_tiles(kt, g40, kernel, grid):
    """units of 0, 1, 8191, 8192, 8193 and 2 x 8192 + 5 items (the long ones over at most 4000 different keys) from tile 3 on,
    empty units first, last and between; two of the tiles filled by add_keys before (dirty byte set); then a second launch,
    another layout, onto the tiles the first one stored -- keys that are there already and new ones.  With grid = 1, 2, 3 one
    workgroup takes clean, dirty, empty and multi-round units in every order; grid = 7 is a unit each.  The pipelined
    kernel's further rounds start from the tile as the round before stored it, and its last round may be partial."""
    G, rng = g40, np.random.default_rng(10 * grid + (kernel == "pipe"))
    tile0 = 3
    G.t.clear()
    total = collections.Counter()
    before = np.concatenate([G.pool_of(tile0 + 1)[:1500], G.pool_of(tile0 + 5)[:700], G.pool_of(tile0 + 6)[:300]])
    G.t.add_keys(before, 3)
    for x in before.tolist():
        total[tuple(x)] += 3
    judge(G, total, rng)
    for n_launch, layout in enumerate((LAYOUT_A, LAYOUT_B)):
        unit_keys = [draw(rng, G.pool_of(tile0 + u)[:5000], n, 4000) for u, n in enumerate(layout)]
        shs = ((1,), (0,), (1, 0, 1), (1, 1))[(grid + n_launch) % 4]
        launch(G, kernel, unit_keys, tile0, grid, rng, shs=shs)
        for keys in unit_keys:
            count_up(total, keys)
        judge(G, total, rng)


@pytest.mark.parametrize("kernel", KERNELS)
def test_more_workgroups_asked_for_than_units_and_the_table_s_last_tiles(kt, g40, kernel):
    """the last three tiles of the table, one workgroup each however many are asked for; the first unit empty"""
    G, rng = g40, np.random.default_rng(21)
    G.t.clear()
    unit_keys = [draw(rng, G.pool_of(13 + u), n, 3000) for u, n in enumerate((0, ROUND + 77, 600))]
    launch(G, kernel, unit_keys, 13, 64, rng)
    total = collections.Counter()
    for keys in unit_keys:
        count_up(total, keys)
    judge(G, total, rng)


# ---- the count field wraps inside the LDS tile ------------------------------------------------------------------------------
def hot_unit(G, rng, tile):
    pool = G.pool_of(tile)
    hot, warm, rest = pool[0], pool[1], pool[2:2002]
    keys = rng.permutation(np.concatenate([np.repeat(hot[None, :], 70000, axis=0), np.repeat(warm[None, :], 65535, axis=0), rest]))
    return hot, warm, keys


@pytest.mark.parametrize("kernel", KERNELS)
def test_one_key_seventy_thousand_times_in_a_tile_of_sixteen_bit_counts(kt, g56, kernel):
    """k = 56 at 2^15 slots: 70 000 occurrences of one key and 65 535 of another in one unit, among 2000 others.  The first
    passes cnt_max inside the LDS tile (ovf_add with the slot's GLOBAL index: tile 2, not tile 0), the second stops one short
    of it; lookup gives both exactly."""
    G, rng = g56, np.random.default_rng(31)
    assert G.g["returning"] and G.g["cnt_bits"] == 16 and G.t.info.val_len == 16
    G.t.clear()
    hot, warm, keys = hot_unit(G, rng, 2)
    other = draw(rng, G.pool_of(1), 900, 900)
    launch(G, kernel, [other, keys], 1, 2, rng)
    vals, found = G.t.lookup(np.stack([hot, warm]))
    assert found.all() and vals.tolist() == [70000, 65535]
    total = collections.Counter()
    count_up(total, other)
    count_up(total, keys)
    judge(G, total, rng)


def test_the_same_at_k_63_in_a_table_of_2_29_slots(kt):
    """the pipelined kernel where the engine's own flushes select it (test_wide_partitioned_path_equals_direct_and_oracle's
    geometry), tile 40 000 of 65 536.  The device only: the emulation would spend its time on 8 GB of table."""
    if os.environ.get("JFGPU_LIB"):                          # (the engine library is named only for the emulation)
        pytest.skip("2^29 slots of 16 bytes: not under the host emulation")
    G = Geometry(kt, 63, 29, 1 << 21, 3, twin=False)
    try:
        rng = np.random.default_rng(41)
        assert G.g["returning"] and G.g["cnt_bits"] == 16
        tile = int(G.tile[0])
        pool = G.pool_of(tile)
        assert len(pool) >= 10
        hot, warm, rest = pool[0], pool[1], pool[2:]
        keys = rng.permutation(np.concatenate([np.repeat(hot[None, :], 70000, axis=0), np.repeat(warm[None, :], 65535, axis=0), rest]))
        launch(G, "pipe", [keys], tile, 1, rng)
        vals, found = G.t.lookup(np.stack([hot, warm]))
        assert found.all() and vals.tolist() == [70000, 65535]
        total = collections.Counter()
        count_up(total, keys)
        judge(G, total, rng, twin=False)
    finally:
        G.close()


# ---- probing ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS + ("direct",))
def test_thirteen_keys_at_home_in_one_slot(kt, g56, kernel):
    """thirteen keys of one idx0: the last one finds its twelve nearest probe slots taken by the others; then the same keys
    again, into the dirty tile"""
    G, rng = g56, np.random.default_rng(51)
    G.t.clear()
    pos, n = np.unique(G.pos, return_counts=True)
    home = pos[n >= 13]
    assert len(home) >= 2, "the pool has no slot with thirteen keys at home"
    crowded = [G.keys[G.pos == p][:13] for p in home[:2]]
    total = collections.Counter()
    for _ in range(2):
        for keys in crowded:
            tile = int(G.positions(keys)[0]) >> 13
            filler = draw(rng, G.pool_of(tile)[:3000], 500, 500)
            both = np.concatenate([keys, filler])
            if kernel == "direct":
                launch_direct(G, both, rng)
            else:
                launch(G, kernel, [both], tile, 1, rng)
            count_up(total, both)
        judge(G, total, rng)


# ---- items_direct_wide_kernel ----------------------------------------------------------------------------------------------
def launch_direct(G, keys, rng, cap=None):
    """one granule batch of the table's own P1 geometry (single-level tables: a bucket is a tile): 2^b1 regions of cap entries"""
    g = G.g
    assert g["b2"] == 0 and g["rest_shift"] == 13
    nb = 1 << g["b1"]
    tile, it = G.items(keys)
    per = [it[tile == b] for b in range(nb)]
    cap = cap or max(64, (max(len(p) for p in per) * 5 // 4 + 70) // 64 * 64)
    items = np.tile(np.array([0x5EA5EA5E, 0x5EA5EA5E], dtype=np.uint64), (nb * cap, 1))     # (what lies behind a region's end is no item: never read)
    off = []
    for b, p in enumerate(per):
        n = min(cap, len(p) + len(p) // 8)
        e = np.tile(HOLE, (n, 1))
        if len(p):
            e[np.sort(rng.choice(n, len(p), replace=False))] = p
        items[b * cap:b * cap + n] = e
        off += [b * cap, b * cap + n]
    name = G.kt.tile_wide(G.t, "direct", [(items, np.array(off, dtype=np.uint64), 1)], grid=5, cap=cap)
    assert name == "items_direct_wide_kernel<%s>" % ("true" if g["returning"] else "false")


@pytest.mark.parametrize("geometry", ("g40", "g56"))
def test_a_granule_batch_inserted_with_global_claims(kt, request, geometry):
    """every tile's region at once, holes among the items, keys that repeat; a second batch onto the first; at k = 56 one key
    66 000 times (the count field wraps in the table: ovf_add)"""
    G, rng = request.getfixturevalue(geometry), np.random.default_rng(61)
    G.t.clear()
    total = collections.Counter()
    n_tiles = 1 << G.g["b1"]
    for _ in range(2):
        keys = np.concatenate([draw(rng, G.pool_of(u)[:3000], 1500 + 100 * u, 1000) for u in range(n_tiles)])
        if G.g["returning"]:
            keys = np.concatenate([keys, np.repeat(G.pool_of(1)[:1], 66000, axis=0)])
        launch_direct(G, rng.permutation(keys), rng)
        count_up(total, keys)
        judge(G, total, rng)
