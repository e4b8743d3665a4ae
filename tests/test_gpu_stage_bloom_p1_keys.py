"""Stage P1b of the partitioned Bloom insert for keys of two, three and four words ALONE: p1_bloom_keys_kernel<WideTable, PER>
(33 <= k <= 64) and p1_bloom_keys_kernel<NTable, PER> (65 <= k <= 128) over a contract buffer, through
tests/kernels/stage_harness_bloom_keys.hip (jfktb_p1), on a zeroed filter.

The reference is tests/bloom_stage_ref.py (oracle_lib.extract and matrix_times take keys of any word count), and the contract
is the one tests/test_gpu_stage_bloom_p1.py states for the sort-based family.  With R the reference multiset of
(bucket, item) of the buffer's k-mers, A the non-hole entries of the regions and F the filter:

  * A is contained in R (as multisets), and F is the expected filter of R - A: what left P1b as items plus what it applied
    itself is exactly the reference, update by update;
  * tot[b] is the number of A's entries in bucket b; gcur[b] is a multiple of kGran;
  * a region is written (items and holes) up to its used length -- cap - gshort[b] if a reservation was refused, else
    min(gcur[b], cap) -- and holds the sentinel behind it; the guard region behind the last bucket keeps the sentinel;
  * a bucket beyond the array's end is untouched;
  * the k-mer counter grows by the number of valid windows;
  * with ample regions: A = R, F all zero.

Where R - A is not empty the shape is chosen so that at most 1 % of R's updates fall on cells R alone takes beyond 2
(asserted: bloom_stage_ref.assert_saturation_cannot_hide) -- else saturation could hide a dropped or doubled update."""
import numpy as np
import pytest

import bloom_stage_ref as BR
import stage_harness_bloom_keys
from stage_harness_bloom_keys import HOLE

pytestmark = pytest.mark.gpu

SENT = 0x5EA5EA5E            # (its digit field is 6: no cell update looks like it)
SEG = BR.SEG_CELLS           # cells of a 64 KiB segment
M8 = 8 * SEG - 3             # eight segments, the last byte partial: 2.6 M cells


@pytest.fixture(scope="module")
def kt(gpu):
    return stage_harness_bloom_keys.load()


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


def run_and_check(kt, blooms, k, canonical, m, nh, part, seq, lo=0, hi=None, cap=None, grid=2):
    b = blooms(k, canonical, m, nh)
    b1, b2 = part
    hi = len(seq) if hi is None else hi
    nb, gran = 1 << b1, kt.const["kGran"]
    cells, n_mers = BR.cells_of(b, seq, lo, hi, canonical)
    R = np.sort(BR.updates_of_cells(cells, b2))
    assert len(R) == 0 or int(R[-1] >> np.uint64(32)) < nb
    per_bucket = np.bincount((R >> np.uint64(32)).astype(np.int64), minlength=nb)
    ample = cap is None
    if ample:        # the fullest bucket, and what the workgroups may strand: a reservation in hand and one asked for, each
        cap = (int(per_bucket.max()) + 2 * grid * gran + gran - 1) // gran * gran
    r = kt.bloom_p1(b, part, seq, lo, hi, cap, grid, SENT)
    assert r["launched"] == "p1_bloom_keys_kernel<%s,%d>" % ("NTable" if k > 64 else "WideTable", kt.const["kBloomKeysPer"])
    out, gcur, gshort = r["out"], r["gcur"].astype(np.int64), r["gshort"].astype(np.int64)
    # regions: written up to their used length, the sentinel behind it and in the guard
    assert (out[nb] == SENT).all(), "entries behind the last bucket's region"
    assert (gcur % gran == 0).all()
    assert (gshort <= cap).all() and (gcur[gshort > 0] > cap).all(), "an overflow note where every reservation fitted"
    used = np.where(gshort > 0, cap - gshort, np.minimum(gcur, cap))
    assert (used % gran == 0).all(), "a region holds whole reservations"
    col = np.arange(cap)[None, :]
    assert (out[:nb][col >= used[:, None]] == SENT).all(), "an entry outside every reservation of its region"
    assert (out[:nb][col < used[:, None]] != SENT).all(), "a reservation was handed out and left as it was (neither items nor holes)"
    stored = (col < used[:, None]) & (out[:nb] != HOLE)
    assert (stored.sum(axis=1) == r["tot"].astype(np.int64)).all(), "tot is not the number of items in the region"
    # buckets beyond the array's end
    beyond = (np.arange(nb) << b2) >= b.n_seg
    assert (stored[beyond].sum() == 0) and (r["tot"][beyond] == 0).all()
    assert (gcur[beyond] == 0).all() and (out[:nb][beyond] == SENT).all(), "a region of a bucket beyond the array's end was touched"
    # A within R, the filter is the rest
    rows, cols_ = np.nonzero(stored)
    got = (rows.astype(np.uint64) << np.uint64(32)) | out[:nb][rows, cols_].astype(np.uint64)
    rest = BR.multiset_minus(R, got, "items in the regions")
    F = b.read()
    if len(rest):
        BR.assert_saturation_cannot_hide(cells)
    exp = BR.expected_filter(np.zeros(b.nb_bytes, dtype=np.uint8), BR.cells_of_updates(rest, b2))
    bad = np.nonzero(F != exp)[0]
    assert len(bad) == 0, "the filter is not the expected filter of the %d updates that are not in a region: %d bytes differ, the first at %d" % (
        len(rest), len(bad), bad[0])
    if ample:
        assert len(rest) == 0 and not F.any(), "ample regions, and updates went to the filter"
    assert r["mers"] == n_mers
    r.update(cap=cap, rest=len(rest), n_updates=len(R))
    return r


def test_the_restatement_agrees_with_the_oracle_on_wide_keys(kt, blooms):
    rng = np.random.default_rng(1)
    b = blooms(100, True, 14 * 3000, 10)
    BR.check_against_oracle(b, reads(rng, 3000, "ACGTacgtN", every=0), True)


# ---- mer lengths: two words (64 is the full mask), three, four -----------------------------------------------------------------
@pytest.mark.parametrize("k", (33, 48, 64, 65, 96, 97, 128))
def test_mer_lengths(kt, blooms, k):
    """canonical or not, on eight segments as (3, 0) and (1, 2); two tiles on two workgroups: windows straddle a tile, a
    workgroup and the halo of 4 and 8 code words"""
    rng = np.random.default_rng(k)
    n = kt.const["kPTilePos"] + 2111
    dense = reads(rng, n, "ACGTacgtN", every=0)                 # an N every nine bases: (8/9)^k of the windows are k-mers, none to speak of above k = 64
    sparse = reads(rng, n, "ACGTacgt", every=701)               # ... so the long mers also get an input that has them
    for canonical, part in ((True, (3, 0)), (False, (1, 2))):
        run_and_check(kt, blooms, k, canonical, M8, 7, part, dense)
        r = run_and_check(kt, blooms, k, canonical, M8, 7, part, sparse)
        assert r["mers"] > n // 2


# ---- hash counts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (64, 100))
@pytest.mark.parametrize("nh", (1, 5, 7, 10, 11, 64))
def test_hash_counts(kt, blooms, k, nh):
    """nh below, at and above the cells of a round, with a partial last round for rounds of five and of ten"""
    rng = np.random.default_rng(nh)
    seq = reads(rng, 2000 if nh == 64 else 6000)
    run_and_check(kt, blooms, k, True, M8, nh, (3, 0), seq)


# ---- filter sizes and bucket geometries ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (64, 100))
def test_filter_sizes(kt, blooms, k):
    """a filter that ends with a full byte at a segment's end; one cell more (a last segment of one cell); seven cells (every
    k-mer's cells collide: ample regions, so nothing reaches the filter); one segment; five segments in (1, 2): the array ends
    inside the last bucket"""
    rng = np.random.default_rng(77)
    seq = reads(rng, 5000)
    run_and_check(kt, blooms, k, True, 5 * SEG, 10, (3, 0), seq)
    run_and_check(kt, blooms, k, True, 5 * SEG + 1, 10, (3, 0), seq)
    run_and_check(kt, blooms, k, True, 7, 10, (0, 0), seq[:3000])
    run_and_check(kt, blooms, k, True, 300001, 10, (0, 0), seq[:3000])
    run_and_check(kt, blooms, k, True, 5 * SEG - 3, 10, (1, 2), seq)


# ---- buffers, lo ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (33, 64, 65, 128))
def test_buffer_edges(kt, blooms, k):
    """hi - lo below k (nothing) and exactly k; lo in 1 .. 15 with hi inside a tile, as bloom_ingest rebases its pieces; an N every
    151 bases; two N exactly k bases apart (nothing between them); a homopolymer of k + 1 bases: the same cells twice in a row"""
    rng = np.random.default_rng(k)
    clean = reads(rng, 4000, every=0)
    go = lambda seq, **kw: run_and_check(kt, blooms, k, True, M8, 10, (3, 0), seq, **kw)
    r = go(clean[:k - 1 + 16], hi=k - 1, grid=1)
    assert r["mers"] == 0 and r["n_updates"] == 0
    assert go(clean[:k + 16], hi=k, grid=1)["mers"] == 1
    assert go(clean, lo=7, hi=7 + k - 1, grid=1)["mers"] == 0
    for lo in (1, 5, 15):
        assert go(clean, lo=lo, hi=3000 + lo, grid=2)["mers"] == 3000 - k + 1
    go(reads(rng, 6000, "ACGTacgtN", every=151))
    two_n = bytearray(clean[:600])
    two_n[100] = two_n[100 + k] = ord("N")
    assert go(bytes(two_n[100:100 + k + 1] + b"\0" * 16), hi=k + 1, grid=1)["mers"] == 0
    go(bytes(two_n))
    homo = b"N" + b"A" * (k + 1) + b"N" + clean[:50]
    r = go(homo, hi=k + 3, grid=1)
    assert r["mers"] == 2 and r["n_updates"] == 20


@pytest.mark.parametrize("k", (64, 128))
def test_exhausted_regions(kt, blooms, k):
    """regions of a few reservations: most updates find their region exhausted and are applied to the filter by the kernel
    itself (bloom_item_direct).  A round's run of a bucket is reserved whole or not at all (375 lanes x 10 cells over 8 or 2
    buckets: 470 or 1900 updates), so regions of two reservations take nothing, regions of 24 and 88 the first three rounds.
    6000 random bases x 10 cells on 2.6 M cells: about (n/m)^2 / 2 = 0.03 % of the updates fall on cells the input takes
    beyond 2 (asserted below 1 % before the comparison)"""
    rng = np.random.default_rng(k + 100)
    seq = reads(rng, 6000, every=0)
    for part, ngran, some in (((3, 0), 2, False), ((3, 0), 24, True), ((1, 2), 2, False), ((1, 2), 88, True)):
        r = run_and_check(kt, blooms, k, True, M8, 10, part, seq, cap=ngran * kt.const["kGran"], grid=2)
        assert r["rest"] > r["n_updates"] // 2
        assert (r["rest"] < r["n_updates"]) == some, "regions of %d reservations: %d of %d updates went to the filter" % (ngran, r["rest"], r["n_updates"])


def test_the_harness_refuses_one_word_keys_and_bad_geometries(kt, blooms):
    seq = reads(np.random.default_rng(3), 500)
    with kt.capi.Bloom(31, M8, 10, seed=7) as b:
        b.set_mode(1)
        b.n_seg = 8
        with pytest.raises(kt.capi.JfgpuError):
            kt.bloom_p1(b, (3, 0), seq, 0, len(seq), 64, 1, SENT)
    b = blooms(64, True, M8, 10)
    for part, cap in (((2, 0), 64), ((3, 0), 65), ((11, 0), 64)):
        with pytest.raises(kt.capi.JfgpuError):
            kt.bloom_p1(b, part, seq, 0, len(seq), cap, 1, SENT)
