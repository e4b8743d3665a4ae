"""Stage P2 of the partitioned insert path ALONE: p2_ring_roles_kernel (every NV / PD the host launches) and
p2_ring_kernel, each followed by p1_stragglers_kernel, launched through tests/kernels/stage_harness.hip on a few buckets
of items built in numpy, and judged against the stage's own contract instead of the table at the end of the pipe.

An item's destination is bucket * 2^b2e + ((item >> tag_bits) & (2^b2e - 1)).  After the launch, for every destination
D of the launched buckets:
  * multiset: the non-hole entries of D's region [D * cap, D * cap + end[D]) plus the recorded DIRECT calls for D, times
    their occurrences, are exactly the input items of D -- nothing lost, doubled or moved to another destination;
  * cursor: end[D] <= cap, where end is what the flush takes as the region's end (granule_finish_kernel, restated in
    region_end); for the loader / storer kernel that is the cursor itself, gcur[D] <= cap;
  * direct counter: the kernels' counter equals the number of recorded calls;
  * guards: every region outside the launched range, pre-filled with a sentinel, comes back unchanged;
  * density (loader / storer kernel): no entry of [0, gcur[D]) is the hole marker -- what SegList::dense promises the
    hole-free tile kernel;
  * ample capacity: with cap = 16 * (ceil(max items of a destination / 16) + 1) and, by the model below, fewer stragglers
    than a list holds, no DIRECT call is made (but for the all-ones item, which can never be a region entry).

The straggler model (straggler_bound): the storers flush round k while the loaders append round k + 1, and a flush leaves
fewer than 16 items of the rounds before it, so while round k is appended a ring holds at most 15 + c[k-1] + c[k] items
(c: the round's items for the destination).  Only a ring past 32 refuses an append; then at most the round's c[k] items go
on the list.  Which entries form a round follows from the layout alone: RS consecutive entries of a bucket's range.

Which loader of the roles kernel a case reaches: exact segments (sh = 0) -> load_exact; a granule segment's whole rounds
-> load_full (every range of at least RS entries; the prefetch loop and its epilogue for n_full = 1 .. 7); a granule
range's last, partial round -> load_partial (ranges of 1, 3, 5, RS - 1, RS + 1 and n_full * RS + 7 entries)."""
import numpy as np
import pytest

import stage_harness
from stage_harness import HOLE

pytestmark = pytest.mark.gpu

SENT = 0xA5A5A5A5                 # what the regions hold before the launch
NVPD = [(nv, pd) for nv in (1, 2) for pd in (1, 2, 3)]


@pytest.fixture(scope="module")
def kt(gpu):
    return stage_harness.load()


@pytest.fixture(scope="module")
def table(kt):
    # (the launches take the table's stream and device; with the recording DIRECT they touch none of its slots)
    with kt.capi.Table(14, 1 << 16, canonical=False) as t:
        yield t


# ---- inputs ------------------------------------------------------------------------------------------------------------
def make_items(rng, dests, tag_bits, b2e):
    n = len(dests)
    hi_bits = 32 - tag_bits - b2e
    it = (np.asarray(dests, dtype=np.uint64) << np.uint64(tag_bits)) | rng.integers(0, 1 << tag_bits, n, dtype=np.uint64)
    if hi_bits:
        it |= rng.integers(0, 1 << hi_bits, n, dtype=np.uint64) << np.uint64(tag_bits + b2e)
    it[it == HOLE] -= 1               # (the tag's lowest bit: the destination stays)
    return it.astype(np.uint32)


def balanced(rng, n, nb):
    """n destinations, every run of nb consecutive ones a permutation: any RS entries hold at most RS / nb + 1 of one."""
    reps = -(-n // nb) if n else 0
    return np.concatenate([rng.permutation(nb) for _ in range(reps)])[:n] if reps else np.zeros(0, dtype=np.int64)


def granule_segment(rng, per_bucket, holes=0.03, align=4):
    """sh = 1: bucket j's range [off[2j], off[2j+1]) starts at a multiple of 16 bytes; some entries are holes (the count of
    ENTRIES is what is asked for: that is what walks the rounds); between the ranges lie entries of no bucket."""
    parts, off = [], []
    at = 0
    for it in per_bucket:
        it = it.copy()
        if len(it) >= 8 and holes:
            it[rng.random(len(it)) < holes] = HOLE
        pad = (-at) % align
        parts.append(np.full(pad + align, 0x00C0FFEE, dtype=np.uint32)); at += pad + align       # (read by a kernel that runs past a range: misplaced items)
        off += [at, at + len(it)]
        parts.append(it); at += len(it)
    return np.concatenate(parts + [np.full(3, 0x00C0FFEE, dtype=np.uint32)]), np.array(off, dtype=np.uint64), 1


def exact_segment(per_bucket, start=3):
    """sh = 0: packed, bucket j = [off[j], off[j+1]), starting anywhere; every entry is an item, the all-ones one too."""
    off = np.concatenate([[0], np.cumsum([len(it) for it in per_bucket])]).astype(np.uint64) + np.uint64(start)
    return np.concatenate([np.full(start, 0x00C0FFEE, dtype=np.uint32)] + list(per_bucket) + [np.full(5, 0x00C0FFEE, dtype=np.uint32)]), off, 0


def seg_range(seg, j):
    items, off, sh = seg
    return items[int(off[j << sh]):int(off[(j << sh) + 1])]


# ---- the model ---------------------------------------------------------------------------------------------------------
def expected_pairs(segs, bucket0, nbk, b2e, tag_bits):
    """sorted (destination << 32 | item) of every item of the launched buckets"""
    nb = 1 << b2e
    out = []
    for seg in segs:
        for j in range(bucket0, bucket0 + nbk):
            e = seg_range(seg, j).astype(np.uint64)
            if seg[2] == 1:
                e = e[e != HOLE]
            d = np.uint64(j * nb) + ((e >> np.uint64(tag_bits)) & np.uint64(nb - 1))
            out.append((d << np.uint64(32)) | e)
    return np.sort(np.concatenate(out)) if out else np.zeros(0, dtype=np.uint64)


def straggler_bound(segs, j, b2e, tag_bits, RS):
    """upper bound on the entries bucket j's workgroup of the roles kernel puts on its list (module docstring)"""
    nb = 1 << b2e
    rounds, ones = [], 0
    for seg in segs:
        e = seg_range(seg, j).astype(np.uint64)
        if seg[2] == 0:
            ones += int((e == HOLE).sum())
        for r0 in range(0, len(e), RS):
            x = e[r0:r0 + RS]
            x = x[x != HOLE]
            rounds.append(np.bincount(((x >> np.uint64(tag_bits)) & np.uint64(nb - 1)).astype(np.int64), minlength=nb))
    bound, prev = ones, np.zeros(nb, dtype=np.int64)
    for c in rounds:
        bound += int(c[(15 + prev + c) > 32].sum())
        prev = c
    return bound


def region_end(r, cap):
    """granule_finish_kernel: where the flush takes a region to end"""
    g, s = r["gcur"].astype(np.int64), r["gshort"].astype(np.int64)
    return np.where(s > 0, np.maximum(cap - s, 0), np.minimum(g, cap))


def ample_cap(exp_pairs):
    if not len(exp_pairs):
        return 16
    _, n = np.unique(exp_pairs >> np.uint64(32), return_counts=True)
    return 16 * (-(-int(n.max()) // 16) + 1)


def run_and_check(kt, table, kernel, nv, pd, b2e, tag_bits, segs, cap, bucket0, nbk, ample=False):
    nb = 1 << b2e
    roles = kernel == "roles"
    RS = (kt.const["kPBlock"] // 2) * 4 * nv if roles else kt.const["kPBlock"] * 8
    n_dest = (bucket0 + nbk) * nb + 1                     # (one destination above the launched range; all of them below it)
    exp = expected_pairs(segs, bucket0, nbk, b2e, tag_bits)
    r = kt.p2(table, kernel, nv, pd, b2e, tag_bits, segs, cap, bucket0, nbk, np.full(n_dest * cap, SENT, dtype=np.uint32), rec_cap=max(1 << 12, 2 * len(exp)))
    want = "p2_ring_roles_kernel<uint32_t,%d,RecordDirect,%d>+p1_stragglers_kernel<uint32_t,RecordDirect>" % (nv, pd) if roles \
        else "p2_ring_kernel<RecordDirect>+p1_stragglers_kernel<uint32_t,RecordDirect>"
    assert r["launched"] == want
    lo, hi = bucket0 * nb, (bucket0 + nbk) * nb
    out, gcur, rec = r["out"], r["gcur"], r["rec"]
    # guards
    assert (out[:lo] == SENT).all() and (out[hi:] == SENT).all(), "a region outside the launched range was written"
    assert not gcur[:lo].any() and not gcur[hi:].any() and not r["gshort"][:lo].any() and not r["gshort"][hi:].any()
    # cursor
    end = region_end(r, cap)
    assert (end <= cap).all()
    if roles:
        assert (gcur[lo:hi] <= cap).all(), "cursor beyond the region: max %d, cap %d" % (int(gcur.max()), cap)
        assert not r["gshort"].any()
    # direct counter
    assert r["n_rec"] == len(rec) == r["ctr_direct"]
    if len(rec):
        assert ((rec[:, 0] >= lo) & (rec[:, 0] < hi)).all() and (rec[:, 2] >= 1).all()
    # multiset
    inside = np.arange(cap)[None, :] < end[:, None]
    inside[:lo] = False; inside[hi:] = False
    if roles:
        assert (out[inside] != HOLE).all(), "a hole inside [0, gcur) of a region the hole-free tile kernel would read"
    rows, cols = np.nonzero(inside & (out != HOLE))
    got = (rows.astype(np.uint64) << np.uint64(32)) | out[rows, cols].astype(np.uint64)
    if len(rec):
        got = np.concatenate([got, np.repeat((rec[:, 0] << np.uint64(32)) | rec[:, 1], rec[:, 2].astype(np.int64))])
    got = np.sort(got)
    assert len(got) == len(exp), "%d items in, %d out (%d direct calls)" % (len(exp), len(got), len(rec))
    assert (got == exp).all()
    # ample capacity
    bounds = [straggler_bound(segs, j, b2e, tag_bits, RS) for j in range(bucket0, bucket0 + nbk)] if roles else []
    if ample:
        assert roles and cap == ample_cap(exp) and max(bounds) < kt.const["kP2StragPerBlock"], "the case is meant to stay inside the model: %r" % (bounds,)
        ones = int(((exp & np.uint64(0xFFFFFFFF)) == HOLE).sum())
        assert r["n_rec"] == ones, "%d direct calls with ample capacity (%d all-ones items)" % (r["n_rec"], ones)
    r["bounds"] = bounds
    return r


def geometry(nv):
    return 9 if nv == 1 else 10            # NV = 1: 512 destinations a bucket, NV = 2: 1024 (launch_p2_rings)


def buckets_of(rng, counts, bucket0, b2e, tag_bits, dist=balanced):
    """items per bucket 0 .. bucket0 + len(counts): the buckets below the launched ones hold items too (never to be seen)"""
    nb = 1 << b2e
    return [make_items(rng, dist(rng, n, nb), tag_bits, b2e) for n in [37] * bucket0 + list(counts) + [21]]


# ---- the round structure -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv,pd", NVPD)
def test_roles_kernel_walks_the_rounds(kt, table, nv, pd):
    """ranges of 0, 1, 3, 5 (the partial 16-byte load), RS - 1, RS, RS + 1 entries: load_partial alone, load_full alone, both"""
    b2e = geometry(nv)
    RS = (kt.const["kPBlock"] // 2) * 4 * nv
    rng = np.random.default_rng(100 * nv + pd)
    for counts, bucket0, tag_bits in (((0, 1, 3), 0, 8), ((5, RS - 1), 5, 32 - b2e), ((RS, RS + 1), 0, 32 - b2e)):
        per = buckets_of(rng, counts, bucket0, b2e, tag_bits)
        segs = [granule_segment(rng, per)]
        cap = ample_cap(expected_pairs(segs, bucket0, len(counts), b2e, tag_bits))
        run_and_check(kt, table, "roles", nv, pd, b2e, tag_bits, segs, cap, bucket0, len(counts), ample=True)


@pytest.mark.parametrize("nv,pd", NVPD)
def test_roles_kernel_prefetch_epilogue(kt, table, nv, pd):
    """n_full * RS + 7 entries for n_full = 1 .. 7: the prefetch loop's epilogue for every n_full % PD, then load_partial"""
    b2e = geometry(nv)
    RS = (kt.const["kPBlock"] // 2) * 4 * nv
    rng = np.random.default_rng(200 * nv + pd)
    for nfull, bucket0, tag_bits in (((1, 2, 3), 0, 8), ((4, 5, 6), 0, 32 - b2e), ((7, 2), 5, 8)):
        counts = [n * RS + 7 for n in nfull]
        per = buckets_of(rng, counts, bucket0, b2e, tag_bits)
        segs = [granule_segment(rng, per)]
        cap = ample_cap(expected_pairs(segs, bucket0, len(counts), b2e, tag_bits))
        run_and_check(kt, table, "roles", nv, pd, b2e, tag_bits, segs, cap, bucket0, len(counts), ample=True)


@pytest.mark.parametrize("nv,pd", NVPD)
def test_roles_kernel_three_segments_and_the_all_ones_item(kt, table, nv, pd):
    """granule, exact, granule in one launch: load_full + load_partial, load_exact (an arbitrary start, the all-ones item
    in it: a DIRECT call, never a region entry), and a bucket that is empty in the first segment"""
    b2e = geometry(nv)
    tag_bits = 32 - b2e                                   # (the only geometry in which an item can be all ones)
    RS = (kt.const["kPBlock"] // 2) * 4 * nv
    rng = np.random.default_rng(300 * nv + pd)
    bucket0, nbk = 5, 2
    s0 = buckets_of(rng, (RS + 9, 0), bucket0, b2e, tag_bits)
    s1 = buckets_of(rng, (300, RS + 2), bucket0, b2e, tag_bits)
    s2 = buckets_of(rng, (2 * RS + 7, 11), bucket0, b2e, tag_bits)
    s1[bucket0][17] = HOLE; s1[bucket0 + 1][RS + 1] = HOLE           # (one in a round's middle, one as a bucket's last entry)
    segs = [granule_segment(rng, s0), exact_segment(s1), granule_segment(rng, s2)]
    exp = expected_pairs(segs, bucket0, nbk, b2e, tag_bits)
    assert int(((exp & np.uint64(0xFFFFFFFF)) == HOLE).sum()) == 2
    r = run_and_check(kt, table, "roles", nv, pd, b2e, tag_bits, segs, ample_cap(exp), bucket0, nbk, ample=True)
    nb = 1 << b2e
    assert sorted(r["rec"][:, 0].tolist()) == [bucket0 * nb + nb - 1, (bucket0 + 1) * nb + nb - 1] and (r["rec"][:, 1] == HOLE).all() and (r["rec"][:, 2] == 1).all()


# ---- destination distributions -----------------------------------------------------------------------------------------
def uniform(rng, n, nb):
    return rng.integers(0, nb, n)


def one_destination(d):
    return lambda rng, n, nb: np.full(n, d % nb, dtype=np.int64)


def burst(rng, n, nb):
    """balanced, but 40 consecutive entries in the first round's middle go to one destination (more than a ring holds)"""
    d = balanced(rng, n, nb)
    d[200:240] = 7
    return d


@pytest.mark.parametrize("nv", (1, 2))
@pytest.mark.parametrize("dist", ("uniform", "one_destination", "list_full", "burst"))
def test_roles_kernel_destination_distributions(kt, table, nv, dist):
    b2e = geometry(nv)
    RS = (kt.const["kPBlock"] // 2) * 4 * nv
    L = kt.const["kP2StragPerBlock"]
    rng = np.random.default_rng({"uniform": 1, "one_destination": 2, "list_full": 3, "burst": 4}[dist] * 10 + nv)
    pd = {"uniform": 3, "one_destination": 1, "list_full": 2, "burst": 3}[dist]
    bucket0, tag_bits = 0, 8
    if dist == "uniform":
        per = buckets_of(rng, (2 * RS + 100, RS - 50, 3 * RS + 1), bucket0, b2e, tag_bits, uniform)
    elif dist == "one_destination":       # ring full, ghosts, then the list: fewer than the list holds
        per = buckets_of(rng, (600, 900), bucket0, b2e, tag_bits, one_destination(3))
    elif dist == "list_full":             # more than the list holds for one destination: the list is full, DIRECT calls follow
        per = buckets_of(rng, (L + 900, 500), bucket0, b2e, tag_bits, one_destination((1 << b2e) - 1))
    else:
        per = buckets_of(rng, (RS + 300, 2 * RS + 5), bucket0, b2e, tag_bits, burst)
    nbk = len(per) - 1
    segs = [granule_segment(rng, per)]
    exp = expected_pairs(segs, bucket0, nbk, b2e, tag_bits)
    r = run_and_check(kt, table, "roles", nv, pd, b2e, tag_bits, segs, ample_cap(exp), bucket0, nbk, ample=dist != "list_full")
    if dist == "one_destination":
        assert r["strag_n"].min() > 0, "a ring took 600 appends of one round without a ghost"
    if dist == "list_full":
        # the first bucket's list is full and the kernel itself called DIRECT for what came after it; the model says the
        # second bucket's cannot be
        assert r["bounds"][0] >= L and r["strag_n"][0] == L and r["n_rec"] > 0
        assert r["bounds"][1] < L and r["strag_n"][1] < L
        assert (r["rec"][:, 0] == (1 << b2e) - 1).all()
    if dist == "burst":
        assert r["bounds"][0] > 0


# ---- capacities --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv", (1, 2))
@pytest.mark.parametrize("capkind", ("passed_by_some", "sixteen"))
def test_roles_kernel_capacities(kt, table, nv, capkind):
    """a capacity that is no multiple of 16 and that some destinations pass (the 332 / 300 pattern of the large-geometry
    test, scaled: a mean of 20 items into regions of 20 -- about half the destinations pass it), and cap = 16"""
    b2e = geometry(nv)
    nb = 1 << b2e
    rng = np.random.default_rng(500 + nv)
    bucket0, tag_bits = 5, 32 - b2e
    per = buckets_of(rng, (20 * nb, 20 * nb + 13), bucket0, b2e, tag_bits, uniform)
    segs = [granule_segment(rng, per)]
    cap = 20 if capkind == "passed_by_some" else 16
    exp = expected_pairs(segs, bucket0, 2, b2e, tag_bits)
    _, n = np.unique(exp >> np.uint64(32), return_counts=True)
    assert (n > cap).sum() > nb // 4 and (capkind == "sixteen" or (n < cap).sum() > nb // 4)
    r = run_and_check(kt, table, "roles", nv, 3, b2e, tag_bits, segs, cap, bucket0, 2)
    assert r["n_rec"] >= int(np.maximum(n - cap, 0).sum()), "more items stayed in regions than the regions hold"


# ---- the kernel whose workgroups share a bucket's regions ----------------------------------------------------------------
@pytest.mark.parametrize("case", ("uniform", "one_destination", "small_cap", "three_segments"))
def test_shared_ring_kernel(kt, table, case):
    """p2_ring_kernel (kG2Blocks workgroups a bucket, granule reservations in shared regions; granule segments only, which
    is all the host gives it): ranges cut among the workgroups at multiples of four items, whole rounds and partial ones"""
    b2e, nb = 10, 1024
    RS = kt.const["kPBlock"] * 8
    G, gran = kt.const["kG2Blocks"], kt.const["kGran"]
    rng = np.random.default_rng(700 + len(case))
    tag_bits = 8 if case != "small_cap" else 32 - b2e
    bucket0 = 0 if case == "uniform" else 5
    if case == "uniform":                 # every workgroup: whole rounds + a partial one; a range of 5; an empty one
        segs = [granule_segment(rng, buckets_of(rng, (G * RS + G * 600 + 1, 5, 0), bucket0, b2e, tag_bits, uniform))]
    elif case == "one_destination":
        segs = [granule_segment(rng, buckets_of(rng, (3000, 41), bucket0, b2e, tag_bits, one_destination(1023)))]
    elif case == "small_cap":
        segs = [granule_segment(rng, buckets_of(rng, (40 * nb, 40 * nb + 3), bucket0, b2e, tag_bits, uniform))]
    else:
        segs = [granule_segment(rng, buckets_of(rng, (RS + 9, 0), bucket0, b2e, tag_bits, uniform)),
                granule_segment(rng, buckets_of(rng, (300, 7), bucket0, b2e, tag_bits, uniform), holes=0.3),
                granule_segment(rng, buckets_of(rng, (2 * RS + 7, 11), bucket0, b2e, tag_bits, uniform))]
    nbk = len(segs[0][1]) // 2 - bucket0 - 1
    exp = expected_pairs(segs, bucket0, nbk, b2e, tag_bits)
    _, n = np.unique(exp >> np.uint64(32), return_counts=True)
    # regions of whole reservations: every workgroup may strand one per destination and asks for the next a round ahead
    cap = gran if case == "small_cap" else (int(n.max()) + 2 * G * gran + gran - 1) // gran * gran
    r = run_and_check(kt, table, "shared", 0, 0, b2e, tag_bits, segs, cap, bucket0, nbk)
    if case == "small_cap":
        assert r["n_rec"] > 0
