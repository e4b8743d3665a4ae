"""The second half of the partitioned Bloom insert, stage by stage, through tests/kernels/stage_harness.hip:

  Tb      bloom_segment_kernel (jfkt_bloom_seg): one workgroup owns one 64 KiB segment in LDS
  direct  bloom_items_direct_kernel (jfkt_bloom_items_direct): a small flush's granule batch by global compare-and-swap
  P2      p2_granule_kernel<uint32_t, BloomDirect, kP2PairPer>, p2_ring_roles_kernel<uint32_t, 2, BloomRingDirect, 3> and
          p2_ring_kernel<BloomRingDirect> (jfkt_bloom_p2): the count path's P2 kernels with the Bloom overflow functors,
          which turn what a region cannot take into a global compare-and-swap on the filter

The reference is tests/bloom_stage_ref.py: the expected filter of a multiset of cell updates over a starting filter is, per
cell, min(start + count, 2).

Tb and the direct kernel: the filter starts as random valid bytes (each < 243, so cells start at 0, 1 and 2); after the launch
it equals the expected filter of the items of the launched segments over that start -- the bytes of segments without items and
of segments outside the launch are identical.  Items carry arbitrary bits above bit 18 (Tb reads the byte offset and the digit
only).  A packed array never holds the all-ones entry (its digit field would be 7).

P2, per destination D = bucket << b2 | (item >> 19): the non-hole entries A of D's region [D cap2, off2[D] end) are input
items of D (a sub-multiset), F -- zero before -- equals the expected filter of the input minus A, and the direct counter is
that difference's size; off2[D] = (D cap2, D cap2 + used) with used as granule_finish_kernel computes it; regions, cursors and
bounds outside the launched buckets are untouched.  Where the difference is not empty at most 1 % of the input's updates fall
on cells the input alone takes beyond 2 (asserted), so saturation cannot hide a dropped or misplaced update.  The ring kernels
are launched on bucket 1 of two (b1 = 1, b2 = 10: 2048 segments, 128 MiB): a functor that drops `bucket << b2` bumps bucket 0's
half of the filter."""
import numpy as np
import pytest

import bloom_stage_ref as BR
import stage_harness
from stage_harness import HOLE, M64

pytestmark = pytest.mark.gpu

SENT = 0x5EA5EA5E
SEG = BR.SEG_CELLS
JUNK = 0x00C0FFEE            # between the ranges: its digit field is 6, so a kernel that reads past a range spoils a byte
U = np.uint64


@pytest.fixture(scope="module")
def kt(gpu):
    return stage_harness.load()


@pytest.fixture(scope="module")
def blooms(kt):
    made = {}

    def get(m):
        if m not in made:
            made[m] = kt.bloom(31, m, 10)
        return made[m]
    yield get
    for b in made.values():
        b.close()


def start_bytes(rng, b):
    return rng.integers(0, 243, b.nb_bytes).astype(np.uint8)


# ---- Tb ---------------------------------------------------------------------------------------------------------------------
def seg_items(rng, cells_in_seg):
    """items of one segment from cell numbers relative to it, arbitrary bits above bit 18"""
    c = np.asarray(cells_in_seg, dtype=np.uint64)
    it = ((c // U(5)) << U(3)) | (c % U(5)) | (rng.integers(0, 1 << 13, len(c)).astype(np.uint64) << U(19))
    return it.astype(np.uint32)


def packed(per_seg, start=3):
    off = np.concatenate([[0], np.cumsum([len(x) for x in per_seg])]).astype(np.uint64) + U(start)
    return np.concatenate([np.full(start, JUNK, dtype=np.uint32)] + list(per_seg) + [np.full(5, JUNK, dtype=np.uint32)]), off, 0


def granule(rng, per_seg, holes=0.05):
    parts, off, at = [], [], 0
    for it in per_seg:
        n = len(it) + int(len(it) * holes) + (2 if len(it) else 0)
        e = np.full(n, HOLE, dtype=np.uint32)
        e[np.sort(rng.choice(n, len(it), replace=False))] = it
        parts.append(np.full(3, JUNK, dtype=np.uint32)); at += 3
        off += [at, at + n]
        parts.append(e); at += n
    return np.concatenate(parts + [np.full(3, JUNK, dtype=np.uint32)]), np.array(off, dtype=np.uint64), 1


def run_tb(kt, b, rng, arrays, n_seg, seg0, grid, start=None):
    """arrays: [(sh, [cells of segment seg0 + t, relative to it] for t < n_seg)]"""
    start = start_bytes(rng, b) if start is None else start
    b.load(start)
    segs, cells = [], []
    for sh, per_seg in arrays:
        its = [seg_items(rng, c) for c in per_seg]
        segs.append(granule(rng, its) if sh else packed(its))
        cells += [np.asarray(c, dtype=np.uint64) + U((seg0 + t) * SEG) for t, c in enumerate(per_seg)]
    assert kt.bloom_seg(b, segs, n_seg, seg0=seg0, grid=grid) == "bloom_segment_kernel"
    F = b.read()
    exp = BR.expected_filter(start, np.concatenate(cells))
    bad = np.nonzero(F != exp)[0]
    assert len(bad) == 0, "%d bytes differ, the first at %d (segment %d): %d for %d, from %d" % (len(bad), bad[0], bad[0] >> 16, F[bad[0]], exp[bad[0]], start[bad[0]])
    return F, start


@pytest.mark.parametrize("seg0,grid", [(0, 1), (2, 2), (2, 8), (0, 8)])
def test_segment_sizes_arrays_and_offsets(kt, blooms, seg0, grid):
    """three of five segments from seg0 on; 0, 1, 8 x 1024 - 1, 8 x 1024 and 8 x 1024 + 1 items a segment (a lane's eight loads in
    flight: one short of, at, and one past a sweep of the workgroup); one to three arrays, packed and granule with holes"""
    b = blooms(5 * SEG)
    rng = np.random.default_rng(seg0 * 10 + grid)
    mk = lambda n: rng.integers(0, SEG, n)
    for sizes in ((0, 1, 8191), (8192, 0, 8193), (8193, 8191, 8192)):
        for kinds in ((0,), (1,), (1, 0), (0, 1, 1)):
            arrays = [(sh, [mk(n if a == 0 else (n // 3 if a == 1 else 0 if n < 2 else 5)) for n in sizes]) for a, sh in enumerate(kinds)]
            run_tb(kt, b, rng, arrays, 3, seg0, grid)


def test_a_hundred_thousand_items_on_fifty_cells(kt, blooms):
    """every lane's compare-and-swap meets others on the same words; cells that start at 0, 1 and 2, all end at 2"""
    b = blooms(5 * SEG)
    rng = np.random.default_rng(50)
    cells = rng.choice(SEG, 50, replace=False)
    F, start = run_tb(kt, b, rng, [(0, [cells[rng.integers(0, 50, 100000)], np.zeros(0, dtype=np.int64)])], 2, 1, 2)
    digits = (F[SEG // 5 + cells // 5].astype(np.int64) // BR.POW3[cells % 5]) % 3
    assert (digits == 2).all()


def test_the_twenty_cells_of_one_word_from_every_lane(kt, blooms):
    """1024 lanes x 20 cells of one 32-bit word, neighbouring lanes on different cells of it; then each of the twenty exactly
    once, in one sweep, over cells that hold 0, 1 and 2: every one that held less than 2 grows by exactly one"""
    b = blooms(5 * SEG)
    rng = np.random.default_rng(20)
    word = 4 * 5 * 1234                                        # the first cell of byte 4936: a 32-bit word's four bytes
    twenty = word + np.arange(20)
    run_tb(kt, b, rng, [(0, [rng.permutation(np.tile(twenty, 1024))])], 1, 3, 1)
    for sh in (0, 1):
        start = np.zeros(b.nb_bytes, dtype=np.uint8)
        start[3 * (1 << 16) + 4936: 3 * (1 << 16) + 4940] = [0 + 3 * 1 + 9 * 2 + 27 * 0 + 81 * 1, 2 + 3 * 2 + 9 * 0 + 27 * 1 + 81 * 0, 242, 0]
        F, _ = run_tb(kt, b, rng, [(sh, [rng.permutation(twenty)])], 1, 3, 1, start=start)
        assert F[3 * (1 << 16) + 4936: 3 * (1 << 16) + 4940].tolist() == [1 + 3 * 2 + 9 * 2 + 27 * 1 + 81 * 2, 2 + 3 * 2 + 9 * 1 + 27 * 2 + 81 * 1, 242, 121]


def test_empty_segments_and_segments_outside_the_launch_keep_their_bytes(kt, blooms):
    b = blooms(5 * SEG)
    rng = np.random.default_rng(21)
    F, start = run_tb(kt, b, rng, [(1, [[], rng.integers(0, SEG, 700), []]), (0, [[], rng.integers(0, SEG, 9), []])], 3, 1, 2)
    seg = np.arange(b.nb_bytes) >> 16
    assert (F[seg != 2] == start[seg != 2]).all() and (F[seg == 2] != start[seg == 2]).any()


def test_the_harness_refuses_segments_and_items_tb_cannot_take(kt, blooms):
    b = blooms(5 * SEG)
    rng = np.random.default_rng(22)
    ok = packed([seg_items(rng, rng.integers(0, SEG, 10))])
    with pytest.raises(kt.capi.JfgpuError):
        kt.bloom_seg(b, [ok], 1, seg0=5)
    with pytest.raises(kt.capi.JfgpuError):
        kt.bloom_seg(b, [packed([np.array([HOLE], dtype=np.uint32)])], 1, seg0=0)


# ---- the direct kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("part,m", [((2, 1), 8 * SEG - 3), ((2, 0), 4 * SEG - 1)])
def test_direct_kernel_on_four_regions_with_holes(kt, blooms, part, m):
    """four regions of 512 entries; holes among the items; behind off[2 b + 1] entries that look like valid items of the bucket,
    which must not be applied"""
    b = blooms(m)
    b1, b2 = part
    rng = np.random.default_rng(m % 1000)
    start = start_bytes(rng, b)
    start[-1] = 0
    b.load(start)
    cap, nb = 512, 1 << b1
    upd = BR.updates_of_cells(rng.integers(0, m, 40000).astype(np.uint64), b2)
    items = np.full(nb * cap, SENT, dtype=np.uint32)
    off, applied = np.zeros(2 * nb, dtype=np.uint64), []
    for q, n in enumerate((300, 0, 512, 1)):
        mine = (upd[(upd >> U(32)) == U(q)] & U(0xFFFFFFFF)).astype(np.uint32)
        assert len(mine) >= cap
        region = mine[:cap].copy()                             # (valid items of this bucket everywhere, also behind the end)
        holes = rng.random(n) < 0.1
        region[:n][holes] = HOLE
        items[q * cap:(q + 1) * cap] = region
        off[2 * q], off[2 * q + 1] = q * cap, q * cap + n
        applied.append((U(q) << U(32)) | region[:n][~holes].astype(np.uint64))
    assert kt.bloom_items_direct(b, part, items, off, cap, grid=3) == "bloom_items_direct_kernel"
    exp = BR.expected_filter(start, BR.cells_of_updates(np.concatenate(applied), b2))
    F = b.read()
    assert (F == exp).all(), "%d bytes differ" % int((F != exp).sum())


# ---- P2 with the Bloom functors --------------------------------------------------------------------------------------------------------
def p2_input(rng, m, b1, b2, counts):
    """counts[j] random cells of P1b bucket j each, as updates (bucket << 32 | item), per bucket"""
    per = []
    for j, n in enumerate(counts):
        lo, hi = (j << b2) * SEG, min(((j + 1) << b2) * SEG, m)
        u = BR.updates_of_cells(rng.integers(lo, hi, n).astype(np.uint64), b2)
        assert ((u >> U(32)) == U(j)).all()
        per.append(u)
    return per


def as_segments(rng, per_bucket, kinds):
    """the updates of every bucket dealt over len(kinds) arrays, granule (sh = 1: ranges from multiples of 16 bytes, holes) or packed"""
    segs = []
    for a, sh in enumerate(kinds):
        mine = [(u[a::len(kinds)] & U(0xFFFFFFFF)).astype(np.uint32) for u in per_bucket]
        if sh:
            parts, off, at = [], [], 0
            for it in mine:
                it = it.copy()
                n = len(it) + len(it) // 20
                e = np.full(n, HOLE, dtype=np.uint32)
                if len(it):
                    e[np.sort(rng.choice(n, len(it), replace=False))] = it
                pad = (-at) % 4
                parts.append(np.full(pad + 4, JUNK, dtype=np.uint32)); at += pad + 4
                off += [at, at + n]
                parts.append(e); at += n
            segs.append((np.concatenate(parts + [np.full(3, JUNK, dtype=np.uint32)]), np.array(off, dtype=np.uint64), 1))
        else:
            segs.append(packed(mine))
    return segs


KERNEL = {"granule": "p2_granule_kernel<uint32_t,BloomDirect,kP2PairPer>",
          "roles": "p2_ring_roles_kernel<uint32_t,2,BloomRingDirect,3>+p1_stragglers_kernel<uint32_t,BloomRingDirect>",
          "shared": "p2_ring_kernel<BloomRingDirect>+p1_stragglers_kernel<uint32_t,BloomRingDirect>"}


def run_p2(kt, b, kernel, part, per_bucket, kinds, bucket0, nbk, cap2, rng):
    b1, b2 = part
    b.clear()
    segs = as_segments(rng, per_bucket, kinds)
    r = kt.bloom_p2(b, kernel, part, segs, cap2, bucket0, nbk, SENT)
    assert r["launched"] == KERNEL[kernel] + "+granule_finish_range_kernel"
    n_dest, gran = 1 << (b1 + b2), kt.const["kGran"]
    out, gcur, gshort, off2 = r["out"], r["gcur"].astype(np.int64), r["gshort"].astype(np.int64), r["off2"]
    lo, hi = bucket0 << b2, (bucket0 + nbk) << b2
    launched = np.zeros(n_dest, dtype=bool); launched[lo:hi] = True
    assert (out[~launched] == SENT).all(), "a region of a bucket that was not launched was written"
    assert (gcur[~launched] == 0).all() and (gshort[~launched] == 0).all() and (off2[~launched] == U(M64)).all()
    used = np.where(gshort > 0, np.maximum(cap2 - gshort, 0), np.minimum(gcur, cap2))
    D = np.arange(n_dest, dtype=np.int64)
    assert (off2[launched, 0] == (D * cap2)[launched].astype(np.uint64)).all() and (off2[launched, 1] == (D * cap2 + used)[launched].astype(np.uint64)).all()
    col = np.arange(cap2)[None, :]
    if kernel == "granule":
        assert (gcur % gran == 0).all()
        assert (gcur[gshort > 0] > cap2).all(), "an overflow note where every reservation fitted"
        assert (out[launched][col < used[launched][:, None]] != SENT).all(), "a reservation was handed out and left as it was"
        assert (out[launched][col >= used[launched][:, None]] == SENT).all(), "an entry behind the region's end"
    if kernel == "roles":
        assert (gcur <= cap2).all() and not gshort.any()
    stored = (col < used[:, None]) & (out != HOLE) & launched[:, None]
    rows, cols_ = np.nonzero(stored)
    A = (rows.astype(np.uint64) << U(32)) | out[rows, cols_].astype(np.uint64)
    X = np.concatenate(per_bucket[bucket0:bucket0 + nbk])
    Xd = ((((X >> U(32)) << U(b2)) | ((X & U(0xFFFFFFFF)) >> U(BR.ITEM_LOW))) << U(32)) | (X & U(0xFFFFFFFF))       # destination << 32 | item
    rest = BR.multiset_minus(Xd, A, "region entries")
    cells_X = BR.cells_of_updates(X, b2)
    if len(rest):
        BR.assert_saturation_cannot_hide(cells_X)
    rest_cells = BR.cells_of_updates(((rest >> U(32)) >> U(b2)) << U(32) | (rest & U(0xFFFFFFFF)), b2)
    F = b.read()
    exp = BR.expected_filter(np.zeros(b.nb_bytes, dtype=np.uint8), rest_cells)
    bad = np.nonzero(F != exp)[0]
    assert len(bad) == 0, "the filter is not the expected filter of the %d updates no region holds: %d bytes differ, the first at %d (segment %d)" % (
        len(rest), len(bad), bad[0], bad[0] >> 16)
    assert r["ctr_direct"] == len(rest), "direct counter %d, %d updates outside the regions" % (r["ctr_direct"], len(rest))
    r.update(rest=len(rest), cells=cells_X, segs=segs)
    return r


def ample(kt, per_bucket, bucket0, nbk, b2):
    """the fullest destination, plus what four workgroups may strand: a reservation in hand and one asked for, each"""
    gran = kt.const["kGran"]
    X = np.concatenate(per_bucket[bucket0:bucket0 + nbk])
    d = (((X >> U(32)) << U(b2)) | ((X & U(0xFFFFFFFF)) >> U(BR.ITEM_LOW))).astype(np.int64)
    return (int(np.bincount(d).max()) + 8 * gran + gran + gran - 1) // gran * gran


@pytest.mark.parametrize("b2,n_seg", [(2, 8), (5, 64)])
def test_sort_based_p2_with_bloomdirect(kt, blooms, b2, n_seg):
    """bucket 1 of two, 4 and 32 segments a bucket, over a granule and a packed array; regions ample (nothing reaches the filter)
    of one reservation (nearly everything does, through bloom_item_direct) and of half the need (both at once)"""
    m = n_seg * SEG - 3
    b = blooms(m)
    rng = np.random.default_rng(b2)
    per_bucket = p2_input(rng, m, 1, b2, (3000, 60000))
    r = run_p2(kt, b, "granule", (1, b2), per_bucket, (1, 0), 1, 1, ample(kt, per_bucket, 1, 1, b2), rng)
    assert r["rest"] == 0
    r = run_p2(kt, b, "granule", (1, b2), per_bucket, (1, 0), 1, 1, kt.const["kGran"], rng)
    assert r["rest"] > 30000
    half = ample(kt, per_bucket, 1, 1, b2) // 2 // kt.const["kGran"] * kt.const["kGran"]
    r = run_p2(kt, b, "granule", (1, b2), per_bucket, (1, 0), 1, 1, half, rng)
    assert 0 < r["rest"] < 60000 - 10000, "regions of half the need: some updates in them, some in the filter (%d)" % r["rest"]


@pytest.mark.parametrize("kernel", ("roles", "shared"))
def test_ring_p2_with_bloomringdirect(kt, blooms, kernel):
    """b1 = 1, b2 = 10 (2048 segments, 128 MiB), bucket 1 only; ample regions, and regions of one reservation: the lists fill and
    the kernels call BloomRingDirect themselves"""
    m = 2048 * SEG - 3
    b = blooms(m)
    rng = np.random.default_rng(10)
    per_bucket = p2_input(rng, m, 1, 10, (5000, 150000))
    kinds = (1, 0) if kernel == "roles" else (1, 1)
    r = run_p2(kt, b, kernel, (1, 10), per_bucket, kinds, 1, 1, ample(kt, per_bucket, 1, 1, 10), rng)
    r = run_p2(kt, b, kernel, (1, 10), per_bucket, kinds, 1, 1, kt.const["kGran"], rng)
    assert r["rest"] > 50000


@pytest.mark.parametrize("tight", (False, True))
def test_p2_then_tb_on_its_bounds(kt, blooms, tight):
    """the chain of a flush: p2_granule_kernel, then bloom_segment_kernel over the regions by off2, from seg0 = bucket0 << b2:
    the bytes are the expected filter of the whole input, whether the updates went through the regions or straight to the filter"""
    b2, m = 2, 8 * SEG - 3
    b = blooms(m)
    rng = np.random.default_rng(30 + tight)
    per_bucket = p2_input(rng, m, 1, b2, (2000, 50000))
    gran = kt.const["kGran"]
    cap2 = ample(kt, per_bucket, 1, 1, b2)
    if tight:                                                  # (half of what a segment gets: the first reservations fit, the later ones are refused)
        cap2 = cap2 // 2 // gran * gran
    r = run_p2(kt, b, "granule", (1, b2), per_bucket, (1,), 1, 1, cap2, rng)
    assert (r["rest"] > 0) == tight and (not tight or 10000 < r["rest"] < 40000), r["rest"]
    seg0, nseg = 1 << b2, 1 << b2
    assert kt.bloom_seg(b, [(r["out"].reshape(-1), r["off2"].reshape(-1)[2 * seg0:], 1)], nseg, seg0=seg0, grid=3) == "bloom_segment_kernel"
    BR.assert_saturation_cannot_hide(r["cells"])
    exp = BR.expected_filter(np.zeros(b.nb_bytes, dtype=np.uint8), r["cells"])
    F = b.read()
    assert (F == exp).all(), "%d bytes differ" % int((F != exp).sum())
