"""Stage P1b of the partitioned Bloom insert ALONE: one of p1_bloom_granule_kernel<NB> (byte tables, 10 cells a round),
p1_bloom_granule2_kernel<NB> (nibble tables, 5 cells a round) and p1_bloom_ring_kernel<NB, PER> (rings of 256 bytes) over a
contract buffer, through tests/kernels/stage_harness.hip (jfkt_bloom_p1), on a zeroed filter.

The reference is tests/bloom_stage_ref.py.  With R the reference multiset of (bucket, item) of the buffer's k-mers, A the
non-hole entries of the regions, L the entries of the ring family's straggler lists times their counts and F the filter:

  * A + L is contained in R (as multisets), and F is the expected filter of R - A - L: what left P1b as items plus what it
    applied itself is exactly the reference, update by update;
  * tot[b] is the number of A's entries in bucket b; gcur[b] is a multiple of kGran (until the straggler kernel appends);
  * a region is written (items and holes) up to its used length -- cap - gshort[b] if a reservation was refused, else
    min(gcur[b], cap) -- and holds the sentinel behind it; the guard region behind the last bucket keeps the sentinel;
  * a bucket beyond the array's end holds no item (the sort-based kernels do not touch it; the ring kernel's owner lanes
    reserve and leave holes);
  * the k-mer counter grows by the number of valid windows;
  * sort-based kernels with ample regions: A = R, F all zero; the ring kernel followed by p1_stragglers_kernel: L is empty.

Where R - A - L is not empty the shape is chosen so that at most 1 % of R's updates fall on cells R alone takes beyond 2
(asserted: bloom_stage_ref.assert_saturation_cannot_hide) -- else saturation could hide a dropped or doubled update."""
import numpy as np
import pytest

import bloom_stage_ref as BR
import stage_harness
from stage_harness import HOLE

pytestmark = pytest.mark.gpu

SENT = 0x5EA5EA5E            # (its digit field is 6: no cell update looks like it)
SEG = BR.SEG_CELLS           # cells of a 64 KiB segment
M8 = 8 * SEG - 3             # eight segments, the last byte partial: 2.6 M cells


@pytest.fixture(scope="module")
def kt(gpu):
    return stage_harness.load()


@pytest.fixture(scope="module")
def blooms(kt):
    made = {}

    def get(k, canonical, m, nh):
        key = (k, canonical, m, nh)
        if key not in made:
            made[key] = kt.bloom(k, m, nh, canonical=canonical)
        made[key].clear()
        return made[key]
    yield get
    for b in made.values():
        b.close()


def reads(rng, n, alphabet="ACGT", every=151):
    s = np.frombuffer(alphabet.encode(), dtype=np.uint8)[rng.integers(0, len(alphabet), n)].copy()
    if every:
        s[every - 1::every] = ord("N")
    return s.tobytes()


NAMES = {"granule": "p1_bloom_granule_kernel<%d>", "granule2": "p1_bloom_granule2_kernel<%d>"}


def run_and_check(kt, blooms, family, nbt, per, k, canonical, m, nh, part, seq, lo=0, hi=None, cap=None, grid=2, run_stragglers=False):
    b = blooms(k, canonical, m, nh)
    b1, b2 = part
    hi = len(seq) if hi is None else hi
    nb, gran, LCAP = 1 << b1, kt.const["kGran"], kt.const["kStragPerBlock"]
    cells, n_mers = BR.cells_of(b, seq, lo, hi, canonical)
    R = np.sort(BR.updates_of_cells(cells, b2))
    assert len(R) == 0 or int(R[-1] >> np.uint64(32)) < nb
    per_bucket = np.bincount((R >> np.uint64(32)).astype(np.int64), minlength=nb)
    ample = cap is None
    if ample:        # the fullest bucket, and what the workgroups may strand: a reservation in hand and one asked for, each
        cap = (int(per_bucket.max()) + 2 * grid * gran + gran - 1) // gran * gran
    r = kt.bloom_p1(b, family, nbt, per, part, seq, lo, hi, cap, grid, SENT, run_stragglers=run_stragglers)
    want = NAMES[family] % nbt if family != "ring" else "p1_bloom_ring_kernel<%d,%d>" % (nbt, per)
    assert r["launched"] == want + ("+p1_stragglers_kernel<uint32_t,BloomP1RingDirect>" if run_stragglers else "")
    out, gcur, gshort = r["out"], r["gcur"].astype(np.int64), r["gshort"].astype(np.int64)
    # regions: written up to their used length, the sentinel behind it and in the guard
    assert (out[nb] == SENT).all(), "entries behind the last bucket's region"
    if not run_stragglers:
        assert (gcur % gran == 0).all()
    assert (gshort <= cap).all() and (gcur[gshort > 0] > cap).all(), "an overflow note where every reservation fitted"
    used = np.where(gshort > 0, cap - gshort, np.minimum(gcur, cap))
    if not run_stragglers:
        assert (used % gran == 0).all(), "a region holds whole reservations"
    col = np.arange(cap)[None, :]
    assert (out[:nb][col >= used[:, None]] == SENT).all(), "an entry outside every reservation of its region"
    assert (out[:nb][col < used[:, None]] != SENT).all(), "a reservation was handed out and left as it was (neither items nor holes)"
    stored = (col < used[:, None]) & (out[:nb] != HOLE)
    assert (stored.sum(axis=1) == r["tot"].astype(np.int64)).all(), "tot is not the number of items in the region"
    # buckets beyond the array's end
    beyond = (np.arange(nb) << b2) >= b.n_seg
    assert (stored[beyond].sum() == 0) and (r["tot"][beyond] == 0).all()
    if family != "ring":
        assert (gcur[beyond] == 0).all() and (out[:nb][beyond] == SENT).all(), "a region of a bucket beyond the array's end was touched"
    # A + L within R, the filter is the rest
    rows, cols_ = np.nonzero(stored)
    got = [(rows.astype(np.uint64) << np.uint64(32)) | out[:nb][rows, cols_].astype(np.uint64)]
    assert (r["strag_n"] <= LCAP).all()
    if family != "ring":
        assert (r["strag_n"] == 0).all()
    n_list = int(r["strag_n"].sum())
    if not run_stragglers:
        for blk in range(grid):
            e = r["strag"][blk, :int(r["strag_n"][blk])]
            cnt = (e >> np.uint64(56)).astype(np.int64)
            assert (cnt >= 1).all() and (((e >> np.uint64(32)) & np.uint64(0xFFFFFF)) < nb).all()
            got.append(np.repeat(e & np.uint64(0x00FFFFFFFFFFFFFF), cnt))
    got = np.concatenate(got)
    rest = BR.multiset_minus(R, got, "items in the regions or on the lists")
    F = b.read()
    if len(rest):
        BR.assert_saturation_cannot_hide(cells)
    exp = BR.expected_filter(np.zeros(b.nb_bytes, dtype=np.uint8), BR.cells_of_updates(rest, b2))
    bad = np.nonzero(F != exp)[0]
    assert len(bad) == 0, "the filter is not the expected filter of the %d updates that are neither in a region nor on a list: %d bytes differ, the first at %d" % (
        len(rest), len(bad), bad[0])
    if ample and family != "ring":
        assert len(rest) == 0 and not F.any(), "ample regions, and updates went to the filter"
    assert r["mers"] == n_mers
    r.update(cap=cap, rest=len(rest), n_updates=len(R), n_list=n_list)
    return r


# ---- the instantiations and the mer lengths --------------------------------------------------------------------------------
# (k, NB): 31 -> 8 bytes, 21 -> 6, 32 -> 8 (the full key mask, windows of 32 bits), 16 -> 4, 10 -> 3 (five nibbles: NB = 0's
# nibble loop is bounded at run time inside a byte)
INST = [(31, 8), (31, 0), (21, 6), (21, 0), (32, 8), (32, 0), (16, 0), (10, 0)]


def test_the_restatement_agrees_with_the_oracle(kt, blooms):
    rng = np.random.default_rng(1)
    b = blooms(25, True, 14 * 3000, 10)
    BR.check_against_oracle(b, reads(rng, 3000, "ACGTacgtN", every=0), True)


@pytest.mark.parametrize("family", ("granule", "granule2"))
@pytest.mark.parametrize("k,nbt", INST)
def test_sort_based_instantiations_and_mer_lengths(kt, blooms, family, k, nbt):
    """every instantiation the host launches, canonical or not, on eight segments as (3, 0) and (1, 2), two tiles on two workgroups"""
    rng = np.random.default_rng(k * 10 + nbt)
    T = kt.const["kPTilePos"]
    seq = reads(rng, T + 2111, "ACGTacgtN", every=0) if k != 10 else reads(rng, T + 2111)
    per = 10 if family == "granule" else 5
    for canonical, part in ((True, (3, 0)), (False, (1, 2))):
        run_and_check(kt, blooms, family, nbt, per, k, canonical, M8, 7, part, seq)


@pytest.mark.parametrize("k,nbt,per", [(31, 8, 10), (21, 6, 10), (31, 0, 10), (10, 0, 10), (32, 8, 5), (16, 0, 5)])
def test_ring_instantiations(kt, blooms, k, nbt, per):
    """(5, 1) on 64 segments: 32 rings take a round's 10 Ki (5 Ki) updates with some overflow; lists as left, and consumed"""
    rng = np.random.default_rng(k + per)
    seq = reads(rng, 9000, "ACGTacgtN", every=0) if k != 10 else reads(rng, 9000)
    m = 64 * SEG - 3
    for canonical, strag in ((True, False), (False, True)):
        run_and_check(kt, blooms, "ring", nbt, per, k, canonical, m, per, (5, 1), seq, run_stragglers=strag)


# ---- hash counts ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,per", [("granule", 10), ("granule2", 5), ("ring", 10), ("ring", 5)])
@pytest.mark.parametrize("nh", (1, 5, 7, 10, 11, 64))
def test_hash_counts(kt, blooms, family, per, nh):
    """nh below, at and above the cells of a round, with a partial last round (11 and 64 on ten a round; 7 and 11 on five)"""
    rng = np.random.default_rng(nh)
    seq = reads(rng, 2000 if nh == 64 else 6000)
    part = (3, 0) if family != "ring" else (2, 1)
    run_and_check(kt, blooms, family, 8, per, 31, True, M8, nh, part, seq, run_stragglers=(family == "ring" and nh % 2 == 1))


# ---- filter sizes and bucket geometries ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,per", [("granule", 10), ("granule2", 5)])
def test_filter_sizes(kt, blooms, family, per):
    """a filter that ends with a full byte at a segment's end; one cell more (a last segment of one cell); seven cells (every
    k-mer's cells collide: ample regions, so nothing reaches the filter); one segment"""
    rng = np.random.default_rng(77)
    seq = reads(rng, 5000)
    run_and_check(kt, blooms, family, 8, per, 31, True, 5 * SEG, 10, (3, 0), seq)
    run_and_check(kt, blooms, family, 8, per, 31, True, 5 * SEG + 1, 10, (3, 0), seq)
    run_and_check(kt, blooms, family, 8, per, 31, True, 7, 10, (0, 0), seq[:3000])
    run_and_check(kt, blooms, family, 8, per, 31, True, 300001, 10, (0, 0), seq[:3000])


def test_the_last_segment_of_one_cell_gets_its_updates(kt, blooms):
    """m = 5 x 327 680 + 1 and nh = 64 on an input (found by the reference) one of whose cells is m - 1: segment 5 holds exactly that cell"""
    rng = np.random.default_rng(209)
    seq = reads(rng, 6000)
    r = run_and_check(kt, blooms, "granule2", 8, 5, 31, True, 5 * SEG + 1, 64, (3, 0), seq)
    assert r["tot"][5] >= 1, "no update fell on the last segment's only cell: the input does not test it"
    vals = r["out"][5][(r["out"][5] != HOLE) & (r["out"][5] != SENT)]
    assert len(vals) == r["tot"][5] and (vals == 0).all()      # byte 0, digit 0 of segment 5


@pytest.mark.parametrize("family,per", [("granule", 10), ("granule2", 5), ("ring", 5)])
@pytest.mark.parametrize("part,nseg", [((3, 0), 8), ((1, 2), 8), ((0, 3), 8), ((1, 2), 5)])
def test_bucket_geometries(kt, blooms, family, per, part, nseg):
    """eight segments as 8 x 1, 2 x 4 and 1 x 8 buckets x sub-buckets; five segments in 2 x 4: the array ends inside the last bucket"""
    rng = np.random.default_rng(nseg * 10 + part[0])
    seq = reads(rng, 7000, "ACGTacgtN", every=0)
    run_and_check(kt, blooms, family, 8, per, 31, True, nseg * SEG - 3, 10, part, seq, run_stragglers=(family == "ring"))


# ---- the ring family's own cases -----------------------------------------------------------------------------------------------
def test_rings_clean_path_on_512_buckets(kt, blooms):
    """(9, 0) on 512 segments, a 32 MiB filter: a round puts 20 updates on a ring of 64, nothing overflows"""
    rng = np.random.default_rng(90)
    seq = reads(rng, 20000)
    r = run_and_check(kt, blooms, "ring", 8, 10, 31, True, 512 * SEG - 3, 10, (9, 0), seq)
    assert r["n_list"] == 0 and r["rest"] == 0, "the clean path put %d updates on the lists and %d into the filter" % (r["n_list"], r["rest"])


@pytest.mark.parametrize("strag", (False, True))
def test_rings_overflow_into_the_list_and_past_it(kt, blooms, strag):
    """(1, 2) with 40 000 bases: every round overflows its two rings, the one workgroup's list passes kStragPerBlock and the
    kernel calls its direct functor itself"""
    rng = np.random.default_rng(91)
    seq = reads(rng, 40000, every=100)                         # (27 600 windows: 276 000 updates on 2.6 M cells)
    r = run_and_check(kt, blooms, "ring", 8, 10, 31, True, M8, 10, (1, 2), seq, grid=1, run_stragglers=strag)
    assert r["strag_n"][0] == kt.const["kStragPerBlock"] and r["rest"] > 0


# ---- buffers, lo, grids, cap ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,per", [("granule", 10), ("granule2", 5), ("ring", 10)])
def test_buffer_edges(kt, blooms, family, per):
    """k - 1 bases (nothing) and k; one short of, at and one past a tile; 40 000 bases with runs of N and lower case; lo = 5 and
    15 as bloom_ingest rebases its pieces; one to three workgroups on one to three tiles"""
    T, k = kt.const["kPTilePos"], 31
    rng = np.random.default_rng(per)
    big = reads(rng, 40000, "ACGTacgtN", every=0)
    big = big[:9000] + b"N" * 70 + big[9070:20000] + b"n" * 31 + big[20031:]
    part = (3, 0) if family != "ring" else (2, 1)
    st = family == "ring"
    go = lambda seq, **kw: run_and_check(kt, blooms, family, 8, per, k, True, M8, 5 if st else 10, part, seq, run_stragglers=st, **kw)
    clean = reads(rng, T + 40, every=0)
    r = go(clean[:k - 1 + 16], hi=k - 1, grid=1)
    assert r["mers"] == 0 and r["n_updates"] == 0
    assert go(clean[:k + 16], hi=k, grid=1)["mers"] == 1
    for n in (T - 1, T, T + 1):
        go(clean[:n + 16], hi=n, grid=2)
    go(big, grid=3)
    go(big, grid=1, hi=2 * T + 5)
    go(big, lo=5, hi=T + 333, grid=2)
    go(big, lo=15, hi=2 * T + 4321, grid=3)


@pytest.mark.parametrize("family,per", [("granule", 10), ("granule2", 5), ("ring", 10), ("ring", 5)])
def test_regions_of_one_reservation(kt, blooms, family, per):
    """cap = kGran: nearly every update finds its region exhausted and is applied to the filter by the kernel (the sort-based
    kernels' bloom_item_direct; the ring kernel through its list and, with the straggler kernel, BloomP1RingDirect)"""
    rng = np.random.default_rng(per + 100)
    seq = reads(rng, 18000, "ACGTacgtN", every=0)
    for part in ((3, 0), (1, 2)):
        r = run_and_check(kt, blooms, family, 8, per, 31, True, M8, 10, part, seq, cap=kt.const["kGran"], grid=2, run_stragglers=(family == "ring"))
        assert r["rest"] > r["n_updates"] // 2


def test_the_harness_refuses_what_the_host_never_launches(kt, blooms):
    b = blooms(21, True, M8, 10)
    seq = reads(np.random.default_rng(3), 500)
    for family, nbt, per, part in (("granule", 8, 10, (3, 0)), ("ring", 6, 5, (3, 0)), ("granule2", 6, 10, (3, 0)), ("granule", 6, 10, (2, 0)), ("ring", 6, 10, (10, 0))):
        with pytest.raises(kt.capi.JfgpuError):
            kt.bloom_p1(b, family, nbt, per, part, seq, 0, len(seq), 64, 1, SENT)
