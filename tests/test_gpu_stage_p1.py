"""Stage P1 of the partitioned insert path ALONE: p1_ring_kernel over a contract buffer of a few block iterations (16 Ki
positions each), on a small real table's descriptor, through tests/kernels/stage_harness.hip.  Neither the straggler
kernel nor the tile stage runs: the regions, the cursors, the exact counts and the workgroups' straggler lists come back as
the kernel left them, and its DIRECT calls are recorded.

The reference is every k-mer occurrence of the buffer (oracle_lib.extract: windows broken by non-ACGT, the canonical form
if asked for), then in numpy: position = M * key under the table's matrix, bucket = position >> (lsize_l - b1),
item = (position & (2^rest_shift - 1)) << rem_bits | key >> lsize.

What must hold, per bucket:
  * the non-hole entries of its region, plus the entries of the straggler lists times their occurrences, plus the DIRECT
    calls times theirs, are exactly the reference's items of the bucket;
  * tot[b] is the number of items stored in the region;
  * no entry lies beyond the region: whole reservations of kGran entries (items and holes) up to min(cursor, cap) rounded
    down, behind them what was there before the launch -- and behind the last region too;
  * the table's k-mer counter grew by the number of windows, its direct counter by the number of DIRECT calls.

Instantiations (the host's, part_ingest): the byte-table hash decided at run time (NB = 0, CANON = 2), six key bytes
compiled in (NB = 6, CANON = 0 and 1), the xor-shift matrix in registers for positions of at most 32 bits (kHashXSLow).
kHashXS proper (positions of more than 32 bits: tables of 2^33 slots and more) has no small geometry and is not launched."""
import numpy as np
import pytest

import oracle_lib as O
import stage_harness
from stage_harness import HOLE

pytestmark = pytest.mark.gpu

SENT = 0x5EA5EA5E


@pytest.fixture(scope="module")
def kt(gpu):
    return stage_harness.load()


@pytest.fixture(scope="module")
def tables(kt):
    made = {}

    def get(k, lsize, canonical, kind="reference"):
        key = (k, lsize, canonical, kind)
        if key not in made:
            t = kt.capi.Table(k, 1 << lsize, canonical=canonical, matrix_kind=kind)
            made[key] = (t, kt.geom(t), t.matrix())
        return made[key]
    yield get
    for t, _, _ in made.values():
        t.close()


def positions(cols, k, keys):
    c = 2 * k
    pos = np.zeros(len(keys), dtype=np.uint64)
    for j in range(c):
        pos ^= np.where((keys >> np.uint64(j)) & np.uint64(1), cols[c - 1 - j], np.uint64(0)).astype(np.uint64)
    return pos


def reference(g, cols, k, canonical, seq, lo, hi, b1):
    """sorted (bucket << 32 | item) of every k-mer occurrence of seq[lo:hi], and their number"""
    keys = O.extract(bytes(seq[lo:hi]), k, canonical)[:, 0]
    pos = positions(cols, k, keys)
    assert (pos[:300] == O.matrix_times(cols, g["lsize_g"], 2 * k, keys[:300])).all()
    rest_shift = g["lsize_l"] - b1
    b = (pos >> np.uint64(rest_shift)) & np.uint64((1 << b1) - 1)
    item = ((pos & np.uint64((1 << rest_shift) - 1)) << np.uint64(g["rem_bits"])) | (keys >> np.uint64(g["lsize_g"]))
    assert rest_shift + g["rem_bits"] <= 32
    return np.sort((b << np.uint64(32)) | item), len(keys)


def run_and_check(kt, tables, k, lsize, canonical, kind, variant, b1, seq, lo=0, hi=None, cap=None, grid=2):
    t, g, cols = tables(k, lsize, canonical, kind)
    hi = len(seq) if hi is None else hi
    nb, gran, L = 1 << b1, kt.const["kGran"], kt.const["kStragPerBlock"]
    exp, n_mers = reference(g, cols, k, canonical, seq, lo, hi, b1)
    if cap is None:      # the mean with head-room, and what the workgroups may strand: a reservation in hand and one asked for, each
        _, n = np.unique(exp >> np.uint64(32), return_counts=True)
        cap = (int(n.max() if len(n) else 0) + 2 * grid * gran + gran - 1) // gran * gran
    r = kt.p1(t, variant, b1, seq, lo, hi, cap, grid, SENT, rec_cap=max(1 << 12, 2 * len(exp)))
    names = {0: "p1_ring_kernel<uint32_t,false,0,2,RecordDirect>", 1: "p1_ring_kernel<uint32_t,false,6,%d,RecordDirect>" % int(canonical),
             2: "p1_ring_kernel<uint32_t,false,kHashXSLow,2,RecordDirect>"}
    assert r["launched"] == names[variant]
    out, rec = r["out"], r["rec"]
    # nothing beyond a region: whole reservations in front, the sentinel behind them and in the guard
    assert (out[nb] == SENT).all(), "entries behind the last bucket's region"
    reserved = np.minimum(r["gcur"].astype(np.int64), cap) // gran * gran
    col = np.arange(cap)[None, :]
    assert (out[:nb][col >= reserved[:, None]] == SENT).all(), "an entry outside every reservation of its region"
    assert (out[:nb][col < reserved[:, None]] != SENT).all(), "a reservation was handed out and left as it was (neither items nor holes)"
    # tot
    stored = (col < reserved[:, None]) & (out[:nb] != HOLE)
    assert (stored.sum(axis=1) == r["tot"].astype(np.int64)).all()
    # multiset
    rows, cols_ = np.nonzero(stored)
    got = [(rows.astype(np.uint64) << np.uint64(32)) | out[:nb][rows, cols_].astype(np.uint64)]
    assert (r["strag_n"] <= L).all()
    for blk in range(grid):
        e = r["strag"][blk, :int(r["strag_n"][blk])]
        cnt = (e >> np.uint64(56)).astype(np.int64)
        assert (cnt >= 1).all() and (((e >> np.uint64(32)) & np.uint64(0xFFFFFF)) < nb).all()
        got.append(np.repeat(e & np.uint64(0x00FFFFFFFFFFFFFF), cnt))
    assert r["n_rec"] == len(rec) == r["ctr_direct"]
    if len(rec):
        assert (rec[:, 0] < nb).all() and (rec[:, 2] >= 1).all()
        got.append(np.repeat((rec[:, 0] << np.uint64(32)) | rec[:, 1], rec[:, 2].astype(np.int64)))
    got = np.sort(np.concatenate(got))
    assert len(got) == len(exp), "%d k-mers in, %d items out" % (len(exp), len(got))
    assert (got == exp).all()
    assert r["mers"] == n_mers
    r["cap"] = cap
    return r


def reads(rng, n, alphabet="ACGT", every=151):
    s = np.frombuffer(alphabet.encode(), dtype=np.uint8)[rng.integers(0, len(alphabet), n)].copy()
    if every:
        s[every - 1::every] = ord("N")
    return s.tobytes()


# (k, lsize, kind, variant, b1): k = 14 at 2^17 slots takes b1 = 6 (items of 22 bits) and 10; six key bytes need k = 21,
# whose items fit 32 bits from b1 = 10 on
CONFIGS = [(14, 17, "reference", 0, 6), (14, 17, "reference", 0, 10), (14, 17, "xs", 2, 6), (14, 17, "xs", 2, 10), (21, 22, "reference", 1, 10)]


@pytest.mark.parametrize("canonical", (False, True))
@pytest.mark.parametrize("k,lsize,kind,variant,b1", CONFIGS)
def test_uniform_reads_and_block_iteration_edges(kt, tables, k, lsize, kind, variant, b1, canonical):
    """uniform reads of three block iterations and a tail on two workgroups; buffers one short of, at, and one past a block
    iteration; an unaligned lo"""
    T = kt.const["kPTilePos"]
    rng = np.random.default_rng(k * 100 + b1 + canonical)
    seq = reads(rng, 3 * T + 777)
    run_and_check(kt, tables, k, lsize, canonical, kind, variant, b1, seq)
    for n in (T - 1, T, T + 1):
        run_and_check(kt, tables, k, lsize, canonical, kind, variant, b1, seq[:n + 16], hi=n, grid=1)
    run_and_check(kt, tables, k, lsize, canonical, kind, variant, b1, seq, lo=5, hi=T + 333)
    run_and_check(kt, tables, k, lsize, canonical, kind, variant, b1, seq, lo=T - 3, hi=2 * T + 9)


@pytest.mark.parametrize("k,lsize,kind,variant,b1", CONFIGS)
def test_runs_and_n_rich_input(kt, tables, k, lsize, kind, variant, b1):
    """a homopolymer and tandem repeats (runs of one k-mer go on the list with their length; the canonical forms of a tandem
    repeat alternate), sequence with a fifth of its bases N"""
    rng = np.random.default_rng(k + b1)
    seq = (reads(rng, 3000) + b"N" + b"A" * 700 + b"N" + b"AC" * 400 + b"N" + b"ACG" * 300 + b"T" * 33 + reads(rng, 2000) + b"N"
           + reads(rng, 30000, "ACGTN", every=0) + b"G" * 40)
    r = run_and_check(kt, tables, k, lsize, True, kind, variant, b1, seq)
    cnt = np.concatenate([r["strag"][b, :int(r["strag_n"][b])] >> np.uint64(56) for b in range(2)])
    assert (cnt > 1).any(), "no run on the lists: the homopolymer's k-mers went item by item"


def test_regions_too_small_for_the_input(kt, tables):
    """regions of one reservation: what they cannot take goes on the lists, and when a list is full the kernel calls DIRECT"""
    T, L = kt.const["kPTilePos"], kt.const["kStragPerBlock"]
    rng = np.random.default_rng(5)
    seq = reads(rng, 3 * T)
    r = run_and_check(kt, tables, 14, 17, False, "reference", 0, 6, seq, cap=kt.const["kGran"])
    assert (r["strag_n"] == L).any() and r["n_rec"] > 0


def test_the_all_ones_item_goes_on_the_list(kt, tables):
    """k = 21 with 2^10 buckets: items have 32 bits, and a k-mer whose item is all ones would read as a hole in a region"""
    k, lsize, b1 = 21, 22, 10
    t, g, cols = tables(k, lsize, False, "reference")
    rest = g["lsize_l"] - b1
    assert rest + g["rem_bits"] == 32
    low = np.arange(1 << 17, dtype=np.uint64)                # (one candidate in 2^12 has the position's low bits all ones)
    keys = (np.uint64((1 << g["rem_bits"]) - 1) << np.uint64(lsize)) | low
    pos = positions(cols, k, keys)
    hit = keys[(pos & np.uint64((1 << rest) - 1)) == np.uint64((1 << rest) - 1)]
    assert len(hit) > 0
    mer = O.to_str(np.array([hit[0]], dtype=np.uint64), k).encode()
    rng = np.random.default_rng(6)
    seq = reads(rng, 5000) + b"N" + mer + b"N" + reads(rng, 5000)
    r = run_and_check(kt, tables, k, lsize, False, "reference", 1, b1, seq)
    on_lists = np.concatenate([r["strag"][b, :int(r["strag_n"][b])] for b in range(2)])
    assert ((on_lists & np.uint64(0xFFFFFFFF)) == HOLE).sum() == 1
