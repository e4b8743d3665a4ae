"""Stage T of the partitioned insert path ALONE: tile_rank_insert_kernel, every instantiation the host launches, through
tests/kernels/stage_harness.hip on small real tables (k = 12 at 2^16 and 2^17 slots, k = 16 at 2^22, 64-bit slots at k = 25
and at k = 14), with units of items built in numpy.

Keys are drawn in numpy; a key's position is M * key under the table's own matrix (oracle_lib.matrix_times, vectorised
here and checked against it); its item is restated from make_item: (local & (2^rest_shift - 1)) << rem_bits | key >> lsize,
with rest_shift = log2(slots of a unit), i.e. idx0 and -- for a pair of tiles -- the tile-select bit right above it.
Unit u of a launch is items[off[2u], off[2u + 1]) (or off[u], off[u + 1] for packed offsets).

The reference is a collections.Counter of the keys, added to what the table held before.  Judged through the library's
own read-back after the launch:
  * dump_records decodes to exactly the Counter, no key twice, in (pos, key) order;
  * lookup finds every key with its count and none of 500 absent keys -- no key was stranded behind a free slot
    (the probe rule of table_find_at);
  * stats and digest agree with capi.digest_of of the Counter."""
import collections
import os

import numpy as np
import pytest

import oracle_lib as O
import stage_harness

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kt(gpu):
    return stage_harness.load()


class Geometry:
    """one small table and pools of keys grouped by the unit (tile, pair of tiles) they hash to"""

    def __init__(self, kt, k, size, slot64=False, pool=1 << 18, seed=1):
        self.kt, self.k = kt, k
        old = os.environ.get("JFGPU_SLOT64")
        os.environ["JFGPU_SLOT64"] = "1" if slot64 else "0"          # (read when the table is created: tuning.hpp)
        try:
            self.t = kt.capi.Table(k, size, canonical=False)
        finally:
            if old is None:
                del os.environ["JFGPU_SLOT64"]
            else:
                os.environ["JFGPU_SLOT64"] = old
        self.t.set_growth(False)
        self.g = kt.geom(self.t)
        self.cols = self.t.matrix()
        assert self.g["tile_bits"] == kt.const["kMaxTileBits"] == 13, "full-size tiles"
        rng = np.random.default_rng(seed)
        self.keys = np.unique(rng.integers(0, 1 << (2 * k), pool, dtype=np.uint64))
        rng.shuffle(self.keys)
        self.pos = self.positions(self.keys)
        sample = slice(0, 1500)
        assert (self.pos[sample] == O.matrix_times(self.cols, self.g["lsize_g"], 2 * k, self.keys[sample])).all()

    def positions(self, keys):
        """M * key: column c - 1 - j of the matrix is the image of key bit j (rectangular_binary_matrix.hpp: times)"""
        keys = np.asarray(keys, dtype=np.uint64)
        c = 2 * self.k
        pos = np.zeros(len(keys), dtype=np.uint64)
        for j in range(c):
            pos ^= np.where((keys >> np.uint64(j)) & np.uint64(1), self.cols[c - 1 - j], np.uint64(0)).astype(np.uint64)
        return pos

    def items(self, keys, tpb, dtype):
        """(unit, item) of every key: make_item with rest_shift = log2(tpb * 2^13)"""
        keys = np.asarray(keys, dtype=np.uint64)
        pos = self.positions(keys)
        ubits = 13 + (tpb - 1)
        it = ((pos & np.uint64((1 << ubits) - 1)) << np.uint64(self.g["rem_bits"])) | (keys >> np.uint64(self.g["lsize_g"]))
        assert ubits + self.g["rem_bits"] <= 8 * np.dtype(dtype).itemsize
        return (pos >> np.uint64(ubits)).astype(np.int64), it.astype(dtype)

    def pool_of_unit(self, u, tpb):
        return self.keys[(self.pos >> np.uint64(13 + tpb - 1)) == np.uint64(u)]

    def close(self):
        self.t.close()


@pytest.fixture(scope="module")
def g12_16(kt):
    g = Geometry(kt, 12, 1 << 16, pool=1 << 20); yield g; g.close()


@pytest.fixture(scope="module")
def g12_17(kt):
    g = Geometry(kt, 12, 1 << 17, seed=2); yield g; g.close()


@pytest.fixture(scope="module")
def g16_22(kt):
    g = Geometry(kt, 16, 1 << 22, pool=1 << 20, seed=3); yield g; g.close()


@pytest.fixture(scope="module")
def g25_16(kt):
    g = Geometry(kt, 25, 1 << 16, seed=4); yield g; g.close()


@pytest.fixture(scope="module")
def g14_18_wide_count(kt):
    g = Geometry(kt, 14, 1 << 18, slot64=True, seed=5); yield g; g.close()


def launch(G, unit_keys, tpb, dtype=np.uint32, heavy=False, sample=False, holes=True, hole_rate=0.0, sh=1, tile0_unit=0, grid=0, rng=None):
    """unit_keys[i]: the keys (with repeats) of unit tile0_unit + i, in the order they are to be stored.  Returns the kernel's name."""
    kt = G.kt
    parts, off, at = [], [], 0
    hole = np.iinfo(dtype).max
    for i, keys in enumerate(unit_keys):
        u, it = G.items(keys, tpb, dtype)
        assert (u == tile0_unit + i).all(), "a key outside the unit it is stored for"
        if hole_rate and len(it):
            assert holes and sh == 1
            n = len(it) + int(len(it) * hole_rate) + 1
            e = np.full(n, hole, dtype=dtype)
            e[np.sort(rng.choice(n, len(it), replace=False))] = it
            it = e
        if sh == 1:
            parts.append(np.full(3, 12345, dtype=dtype)); at += 3           # (entries of no unit between the ranges)
            off += [at, at + len(it)]
        else:
            off += [at]
        parts.append(it); at += len(it)
    if sh == 0:
        off += [at]
    items = np.concatenate(parts) if parts else np.zeros(0, dtype=dtype)
    name = kt.tile(G.t, items, np.array(off, dtype=np.uint64), sh, len(unit_keys), tpb, heavy=heavy, sample=sample, holes=holes,
                   tile0=tile0_unit * tpb, grid=grid)
    want = "tile_rank_insert_kernel<%s,%s,%s,%d,kTileBlock,%s,%s,%s>" % (
        "uint32_t" if dtype == np.uint32 else "uint64_t", "true" if G.g["returning"] else "false",
        "unsigned int" if G.g["slot32"] else "unsigned long long", tpb, str(bool(heavy)).lower(), str(bool(sample)).lower(), str(bool(holes)).lower())
    assert name == want
    return name


def judge(G, counter, rng):
    """the table holds exactly `counter` (key -> count), by every read-back path"""
    t, capi = G.t, G.kt.capi
    t.sync()                                               # (raises "Hash full" if a kernel gave up on a key)
    exp_k = np.array(sorted(counter), dtype=np.uint64)
    exp_c = np.array([counter[int(x)] for x in exp_k], dtype=np.uint64)
    keys, cnts = capi.decode_records(t.dump_records(), G.k, 4)
    assert len(np.unique(keys)) == len(keys), "a key is in the table twice"
    assert len(keys) == len(exp_k), "%d keys in the table, %d expected" % (len(keys), len(exp_k))
    pos = G.positions(keys)
    order = np.lexsort((keys, pos))
    assert (order == np.arange(len(keys))).all(), "the dump is not in (pos, key) order"
    by_key = np.argsort(keys)
    assert (keys[by_key] == exp_k).all() and (cnts[by_key] == exp_c).all()
    if len(exp_k):
        vals, found = t.lookup(exp_k)
        assert found.all(), "%d keys are in the table but not found from their home bucket on" % int((~found.astype(bool)).sum())
        assert (vals == exp_c).all()
    absent = np.setdiff1d(rng.integers(0, 1 << (2 * G.k), 600, dtype=np.uint64), exp_k)[:500]
    _, found = t.lookup(absent)
    assert not found.any()
    st = t.stats()
    assert (st.distinct, st.total, st.max_count) == (len(exp_k), int(exp_c.sum()), int(exp_c.max()) if len(exp_c) else 0)
    assert t.digest() == capi.digest_of(exp_k, exp_c)


def draw(rng, pool, n, distinct):
    """n keys of the pool (with repeats) over `distinct` different ones"""
    if n == 0:
        return np.zeros(0, dtype=np.uint64)
    d = pool[rng.choice(len(pool), min(distinct, n, len(pool)), replace=False)]
    return np.concatenate([d, d[rng.integers(0, len(d), n - len(d))]]) if n > len(d) else d


def row_walk(kt, itemsize):
    B, R = kt.const["kTileBlock"], kt.const["kTileRound4"] if itemsize == 4 else kt.const["kTileRound8"]
    assert B == 512 and R == (9216 if itemsize == 4 else 4608)
    return [0, 1, B - 1, B, B + 1, 2 * B + 1, R - 1, R, R + 1, 2 * R + 5]


VARIANTS = {"plain": dict(), "heavy": dict(heavy=True), "sample": dict(sample=True)}


# ---- items per unit walk the rows and the rounds, in every instantiation of 4-byte items into 32-bit slots -----------------
# (the hole-free instantiation is the plain kernel's, sampling or not: a static_assert in kernels_tile.hip.hpp)
INST32 = [(tpb, True, v) for tpb in (1, 2) for v in sorted(VARIANTS)] + [(2, False, "plain"), (2, False, "sample")]


@pytest.mark.parametrize("tpb,holes,variant", INST32)
def test_rows_and_rounds_into_32bit_slots(kt, g12_17, tpb, holes, variant):
    """0, 1, 511, 512, 513, 1025, 9215, 9216, 9217 and 2 x 9216 + 5 items a unit (over at most 1500 different keys: a unit
    holds 8192 or 16384 slots), in launches of five units on two workgroups -- the long units first, into clean tiles, then
    the short ones into the tiles the first launch left dirty (load_tile), with keys that occur again.  HOLES = true: hole entries sprinkled into the units; HOLES = false:
    the plain and the sampling kernel on dense units of pairs."""
    G, rng = g12_17, np.random.default_rng(10 * tpb + holes)
    assert G.t.info.slot_bytes == 4
    G.t.clear()
    walk = row_walk(kt, 4)
    total = collections.Counter()
    for counts in (walk[5:], walk[:5]):                    # (units of several rounds into clean tiles: a later round reads what the first stored)
        unit_keys = [draw(rng, G.pool_of_unit(u, tpb)[:3000], n, 1500) for u, n in enumerate(counts)]
        launch(G, unit_keys, tpb, holes=holes, hole_rate=0.05 if holes else 0.0, grid=2, rng=rng, **VARIANTS[variant])
        for keys in unit_keys:
            total.update(keys.tolist())
        judge(G, total, rng)


def test_packed_offsets_and_a_first_unit_that_is_not_tile_zero(kt, g12_17):
    """sh = 0 (an exact batch of a single-level table: no holes, off[u], off[u + 1]) from unit 3 on; units that differ: one
    empty, one of a single partial row, one of several rounds"""
    G, rng = g12_17, np.random.default_rng(77)
    G.t.clear()
    for tpb in (1, 2):
        G.t.clear()
        unit_keys = [draw(rng, G.pool_of_unit(3 + i, tpb), n, 2000) for i, n in enumerate((0, 37, 2 * 9216 + 700))]
        launch(G, unit_keys, tpb, sh=0, tile0_unit=3)
        judge(G, collections.Counter(np.concatenate(unit_keys).tolist()), rng)


# ---- contents ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("tpb", (1, 2))
def test_all_distinct_and_every_key_fifty_times(kt, g12_16, tpb, variant):
    """distinct keys at load 0.45 of a unit (phase A and the queue), then 100 keys 50 times each in the same units (phase M:
    equal tags merged before the queue walks)"""
    G, rng = g12_16, np.random.default_rng(20 + tpb)
    assert G.t.info.slot_bytes == 4
    G.t.clear()
    n_units = 2
    first = [G.pool_of_unit(u, tpb)[:int(0.45 * 8192 * tpb)] for u in range(n_units)]
    launch(G, first, tpb, hole_rate=0.02, rng=rng, **VARIANTS[variant])
    total = collections.Counter(np.concatenate(first).tolist())
    judge(G, total, rng)
    second = []
    for u in range(n_units):
        pool = G.pool_of_unit(u, tpb)
        d = np.concatenate([pool[:50], pool[-50:]])               # 50 that are in the table already, 50 new ones
        second.append(rng.permutation(np.repeat(d, 50)))
    launch(G, second, tpb, hole_rate=0.02, rng=rng, **VARIANTS[variant])
    total.update(np.concatenate(second).tolist())
    judge(G, total, rng)


def keys_of_bucket(G, tpb, unit, bucket, n=12):
    """n distinct keys whose home is one bucket (four slots) of a unit, picked from the pool by their computed position"""
    kB = 1 << G.kt.const["kBucketBits"]
    ubits = 13 + tpb - 1
    m = ((G.pos >> np.uint64(ubits)) == np.uint64(unit)) & (((G.pos & np.uint64((1 << ubits) - 1)) // np.uint64(kB)) == np.uint64(bucket))
    keys = G.keys[m]
    assert len(keys) >= n, "only %d of %d keys of the pool are at home in bucket %d of unit %d" % (len(keys), n, bucket, unit)
    return keys[:n]


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("tpb", (1, 2))
def test_twelve_keys_at_home_in_one_bucket(kt, g12_16, tpb, variant):
    """the queue phase walking on: twelve keys of one bucket need three -- in the middle of a tile; in the LAST bucket of a
    tile, where the walk wraps to the tile's first buckets (with pairs: the last bucket of the pair's FIRST tile must not
    leak into the sibling, and the last bucket of the second must not leave the pair); then the same keys again into the
    dirty tiles"""
    G, rng = g12_16, np.random.default_rng(30 + tpb)
    G.t.clear()
    nbk = (8192 >> kt.const["kBucketBits"])
    buckets = [(0, 777), (1, nbk - 1)] + ([(2, 2 * nbk - 1), (3, nbk - 1)] if tpb == 2 else [(2, 0)])
    unit_keys = [np.zeros(0, dtype=np.uint64)] * 4
    for u, b in buckets:
        unit_keys[u] = keys_of_bucket(G, tpb, u, b)
    if tpb == 2:                                           # a few keys at home at the start of BOTH tiles of unit 3: the wrap's landing place is taken
        unit_keys[3] = np.concatenate([keys_of_bucket(G, tpb, 3, 0, 4), keys_of_bucket(G, tpb, 3, nbk, 4), unit_keys[3]])
    total = collections.Counter()
    for _ in range(2):
        launch(G, unit_keys, tpb, hole_rate=0.2, rng=rng, **VARIANTS[variant])
        total.update(np.concatenate(unit_keys).tolist())
        judge(G, total, rng)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("tpb", (1, 2))
def test_one_key_a_thousand_times_wraps_the_count_field(kt, g16_22, tpb, variant):
    """a count field of at most 10 bits: 1000 occurrences of one key in one unit wrap it inside the kernel, and the overflow
    side table is written through ovf_add_call (from the merge, the bulk adds of HEAVY, the queue)"""
    G, rng = g16_22, np.random.default_rng(40 + tpb)
    assert G.t.info.slot_bytes == 4 and G.t.info.val_len <= 10
    G.t.clear()
    pool = G.pool_of_unit(1, tpb)
    hot, rest = pool[0], pool[1:400]
    unit_keys = [np.zeros(0, dtype=np.uint64), rng.permutation(np.concatenate([np.repeat(hot, 1000), rest, rest[:100]]))]
    launch(G, unit_keys, tpb, hole_rate=0.05, rng=rng, **VARIANTS[variant])
    total = collections.Counter(unit_keys[1].tolist())
    vals, found = G.t.lookup(np.array([hot], dtype=np.uint64))
    assert found.all() and int(vals[0]) == 1000
    judge(G, total, rng)
    launch(G, unit_keys, tpb, hole_rate=0.05, rng=rng, **VARIANTS[variant])      # ... and 1000 more on top of a wrapped field
    total.update(unit_keys[1].tolist())
    judge(G, total, rng)


@pytest.mark.parametrize("tpb,holes", [(1, True), (2, True), (2, False)])
def test_into_tiles_filled_by_add_keys(kt, g12_16, tpb, holes):
    """earlier content in the global-atomic path's layout (add_keys: table_add claims slots one by one), keys that occur
    again in the units and new ones"""
    G, rng = g12_16, np.random.default_rng(50 + tpb)
    G.t.clear()
    before = np.concatenate([G.pool_of_unit(u, tpb)[:1500] for u in range(2)])
    G.t.add_keys(before, 3)
    G.t.sync()
    total = collections.Counter({int(x): 3 for x in before})
    judge(G, total, rng)
    unit_keys = [np.concatenate([G.pool_of_unit(u, tpb)[1000:2500], G.pool_of_unit(u, tpb)[1200:1300]]) for u in range(2)]
    launch(G, unit_keys, tpb, holes=holes, hole_rate=0.03 if holes else 0.0, rng=rng)
    total.update(np.concatenate(unit_keys).tolist())
    judge(G, total, rng)


# ---- the other slot and item widths -----------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_eight_byte_items_into_eight_byte_slots(kt, g25_16, variant):
    """k = 25 at 2^16 slots: 64-bit slots, items of 47 bits -- the instantiations with rounds of 4608 items"""
    G, rng = g25_16, np.random.default_rng(60)
    assert G.t.info.slot_bytes == 8 and G.g["rem_bits"] + 13 > 32 and G.g["returning"]
    G.t.clear()
    walk = row_walk(kt, 8)
    total = collections.Counter()
    for counts in (walk[:5], walk[5:]):
        unit_keys = [draw(rng, G.pool_of_unit(u, 1)[:3000], n, 1500) for u, n in enumerate(counts)]
        launch(G, unit_keys, 1, dtype=np.uint64, hole_rate=0.05, grid=2, rng=rng, **VARIANTS[variant])
        for keys in unit_keys:
            total.update(keys.tolist())
        judge(G, total, rng)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("dtype", (np.uint32, np.uint64))
def test_count_fields_of_forty_bits(kt, g14_18_wide_count, dtype, variant):
    """64-bit slots whose count field has 40 bits: RETURNING = false (no add looks at what it returns), 4- and 8-byte items"""
    G, rng = g14_18_wide_count, np.random.default_rng(70)
    assert G.t.info.slot_bytes == 8 and G.t.info.val_len >= 40 and not G.g["returning"]
    G.t.clear()
    unit_keys = [draw(rng, G.pool_of_unit(u, 1)[:4000], n, 3000) for u, n in enumerate((513, 0, 9216 + 9 if dtype == np.uint32 else 4608 + 9, 3000))]
    total = collections.Counter()
    for _ in range(2):
        launch(G, unit_keys, 1, dtype=dtype, hole_rate=0.05, rng=rng, **VARIANTS[variant])
        total.update(np.concatenate(unit_keys).tolist())
        judge(G, total, rng)


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_eight_byte_items_into_32bit_slots(kt, g16_22, variant):
    """what a table of 32-bit slots gets when its items do not fit 32 bits (large tables: more position bits in the item)"""
    G, rng = g16_22, np.random.default_rng(80)
    G.t.clear()
    unit_keys = [draw(rng, G.pool_of_unit(u, 1), n, 2500) for u, n in enumerate((1, 4608 + 600, 0, 700))]
    launch(G, unit_keys, 1, dtype=np.uint64, hole_rate=0.05, grid=3, rng=rng, **VARIANTS[variant])
    judge(G, collections.Counter(np.concatenate(unit_keys).tolist()), rng)
