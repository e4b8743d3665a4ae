"""Stage P1w of the two-word partitioned path ALONE: p1_wide_granule_kernel<RETURNING, false, XS> over a contract buffer,
on a small real table's descriptor, through tests/kernels/stage_harness.hip (jfkt_p1_wide).  P2 and the tile stage do not
run: the bucket regions, the cursors and the exact counts come back as the kernel left them.  This kernel's overflow is
not a template argument: what a region cannot take is claimed in the table itself (wide_item_direct), and the test reads
the table with dump_records.

The reference is plain Python ints: every window of [lo, hi) without a non-ACGT base, its canonical form if asked for, its
position M * key from the columns the table reports (matrix(): column c - 1 - j is the image of key bit j, as
tests/test_gpu_route.py reads it), then make_item_wide restated:
    local = pos mod 2^lsize_l, bucket = local >> (lsize_l - b1), item = (local mod 2^rest_shift) << rem_bits | key >> lsize_g.

What must hold:
  * per bucket, the non-hole entries of its region plus the keys the table holds afterwards (weighted by their counts) are
    the reference's occurrences of the bucket;
  * tot[b] is the number of items stored in region b;
  * a region holds whole reservations -- every entry in front of min(cursor, cap) (cap minus the overflow note where a
    reservation was refused) was written, item or hole -- and nothing behind them; the guard region behind the last
    bucket's is untouched;
  * the table's k-mer counter grew by the number of windows, its direct counter by the sum of the table's counts."""
import collections

import numpy as np
import pytest

import stage_harness
from stage_harness import M64

pytestmark = pytest.mark.gpu

SENT = (0x5EA5EA5E5EA5EA5E << 64) | 0x0123456789ABCDEF
CODE = {65: 0, 67: 1, 71: 2, 84: 3, 97: 0, 99: 1, 103: 2, 116: 3}


@pytest.fixture(scope="module")
def kt(gpu):
    return stage_harness.load()


class Config:
    """one table, one sequence, and the reference of every window of the sequence"""

    def __init__(self, kt, k, lsize, canonical, kind, seq, shard_bits=0):
        self.kt, self.k, self.canonical, self.seq = kt, k, canonical, seq
        self.t = kt.capi.Table(k, 1 << lsize, canonical=canonical, matrix_kind=kind, shard_bits=shard_bits, shard_id=0)
        self.t.set_growth(False)
        self.g = kt.geom(self.t)
        g = self.g
        assert g["key_bits"] == 2 * k and g["tag_full"] == g["tile_bits"] + g["rem_bits"] and g["hash_xs"] == (kind == "xs")
        cols = [int(x) for x in self.t.matrix()]
        c = 2 * k
        # M * key a byte of the key at a time
        self.byte_img = []
        for b in range((c + 7) // 8):
            img = [0] * 256
            for v in range(1, 256):
                low = v & -v
                j = 8 * b + low.bit_length() - 1
                img[v] = img[v ^ low] ^ (cols[c - 1 - j] if j < c else 0)
            self.byte_img.append(img)
        # forward and reverse-complement key of the window ENDING at each position, and the run of valid bases ending there
        mask, top = (1 << c) - 1, 2 * (k - 1)
        fw = rc = run = 0
        self.key_at, self.run_at = [], []
        for ch in seq:
            code = CODE.get(ch)
            if code is None:
                fw = rc = run = 0
            else:
                fw = ((fw << 2) | code) & mask
                rc = (rc >> 2) | ((3 - code) << top)
                run += 1
            self.run_at.append(run)
            self.key_at.append(min(fw, rc) if canonical else fw)
        self.pos_of = {}

    def position(self, key):
        p = self.pos_of.get(key)
        if p is None:
            p, v, b = 0, key, 0
            while v:
                p ^= self.byte_img[b][v & 255]
                v >>= 8; b += 1
            self.pos_of[key] = p
        return p

    def reference(self, lo, hi, b1):
        """Counter of (bucket, item) over the windows of [lo, hi), the map key -> (bucket, item), and the number of windows"""
        g, k = self.g, self.k
        rest_shift = g["lsize_l"] - b1
        occ, of_key, n = collections.Counter(), {}, 0
        for e in range(lo + k - 1, hi):
            if min(self.run_at[e], e - lo + 1) < k:
                continue
            key = self.key_at[e]
            n += 1
            bi = of_key.get(key)
            if bi is None:
                local = self.position(key) & ((1 << g["lsize_l"]) - 1)
                bi = of_key[key] = (local >> rest_shift, ((local & ((1 << rest_shift) - 1)) << g["rem_bits"]) | (key >> g["lsize_g"]))
            occ[bi] += 1
        return occ, of_key, n

    def check(self, b1, lo, hi, grid, cap=None):
        kt, t, g = self.kt, self.t, self.g
        gran, nb = kt.const["kGran"], 1 << b1
        occ, of_key, n_mers = self.reference(lo, hi, b1)
        if cap is None:                                        # regions that cannot overflow: every window in one bucket, a stranded reservation a workgroup
            cap = ((hi - lo) + grid * gran + gran - 1) // gran * gran
        t.clear()
        r = kt.p1_wide(t, b1, self.seq, lo, hi, cap, grid, SENT)
        assert r["launched"] == "p1_wide_granule_kernel<%s,false,%s>" % ("true" if g["returning"] else "false", "true" if g["hash_xs"] else "false")
        out = r["out"]
        sent = (out[..., 0] == np.uint64(SENT & M64)) & (out[..., 1] == np.uint64(SENT >> 64))
        hole = (out[..., 0] == np.uint64(M64)) & (out[..., 1] == np.uint64(M64))
        assert sent[nb].all(), "entries behind the last bucket's region"
        gcur, gshort = r["gcur"].astype(np.int64), r["gshort"].astype(np.int64)
        assert (gcur % gran == 0).all() and (gshort <= cap).all() and (gcur[gshort > 0] > cap).all()
        used = np.where(gshort > 0, cap - gshort, np.minimum(gcur, cap))
        col = np.arange(cap)[None, :]
        assert sent[:nb][col >= used[:, None]].all(), "an entry outside every reservation of its region"
        assert not sent[:nb][col < used[:, None]].any(), "a reservation was handed out and left as it was (neither items nor holes)"
        stored = (col < used[:, None]) & ~hole[:nb]
        assert (stored.sum(axis=1) == r["tot"].astype(np.int64)).all(), "tot is not the number of items stored"
        got = collections.Counter()
        bs, cs = np.nonzero(stored)
        lo_w, hi_w = out[bs, cs, 0].tolist(), out[bs, cs, 1].tolist()
        for b, l, h in zip(bs.tolist(), lo_w, hi_w):
            got[(b, (h << 64) | l)] += 1
        # what the regions could not take is in the table
        t.sync()
        keys, cnts = kt.capi.decode_records(t.dump_records(), self.k, t.info.out_counter_len)
        in_table = 0
        for (l, h), c in zip(keys.tolist(), cnts.tolist()):
            key = (h << 64) | l
            assert key in of_key, "the table holds a key that is no window of the input"
            got[of_key[key]] += c
            in_table += c
        assert r["mers"] == n_mers, "%d windows, the k-mer counter says %d" % (n_mers, r["mers"])
        assert r["ctr_direct"] == in_table, "direct counter %d, the table's counts sum to %d" % (r["ctr_direct"], in_table)
        assert sum(got.values()) == sum(occ.values()), "%d k-mers in, %d items out (%d in the table)" % (sum(occ.values()), sum(got.values()), in_table)
        assert got == occ
        r["cap"], r["in_table"] = cap, in_table
        return r


def sequence(k, seed):
    """uniform bases with an N every 2 k bases in one part, a poly-A stretch, lower case, and plain uniform sequence"""
    rng = np.random.default_rng(seed)
    draw = lambda n: np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].copy()
    a = draw(9000)
    a[2 * k - 1::2 * k] = ord("N")
    b = draw(3000)
    b[::7] |= 0x20
    return a.tobytes() + b"N" + b"A" * 900 + b.tobytes() + b"NN" + draw(28000).tobytes() + b"G" * 40 + b"N" * 20


CONFIGS = [(33, 17, "reference"), (33, 17, "xs"), (40, 17, "reference"), (40, 17, "xs"), (56, 15, "reference"), (56, 15, "xs")]


@pytest.fixture(scope="module")
def configs(kt):
    made = {}

    def get(k, lsize, canonical, kind):
        key = (k, lsize, canonical, kind)
        if key not in made:
            made[key] = Config(kt, k, lsize, canonical, kind, sequence(k, 7 * k + lsize))
        return made[key]
    yield get
    for c in made.values():
        c.t.close()


@pytest.mark.parametrize("canonical", (False, True))
@pytest.mark.parametrize("k,lsize,kind", CONFIGS)
def test_regions_hold_every_window(kt, configs, k, lsize, kind, canonical):
    """ample regions, nothing in the table: 40 000 bases on three workgroups (N's every 2 k bases, a poly-A stretch, lower
    case) at b1 = 1, half of them at b1 = 0; buffers of k - 1, k and 16 384 +- 1 bases from a `lo` that is no multiple of 16;
    b1 = 10 (buckets smaller than a tile: the kernel does not care) on a short range"""
    C = configs(k, lsize, canonical, kind)
    assert C.g["returning"] == (k == 56), "k = 56 at 2^15 slots has the 16-bit count field"
    T = kt.const["kPTilePos"]
    assert T == 16384 and len(C.seq) > 40000 + 13
    r = C.check(1, 0, 40000, 3)
    assert r["in_table"] == 0 and r["mers"] > 30000
    C.check(0, 13, 20013, 3)
    lo = 9000 + 1 + 900 + 3000 + 2 + 5                        # inside the plain uniform part, lo % 16 != 0
    assert lo % 16 and b"N" not in C.seq[lo:lo + T + 1]
    for n, windows in ((k - 1, 0), (k, 1), (T - 1, T - k), (T + 1, T + 2 - k)):
        r = C.check(1, lo, lo + n, 1)
        assert r["mers"] == windows
    r = C.check(10, 8990, 8990 + 2500, 3)
    assert r["in_table"] == 0
    C.check(10, lo, lo + k, 1)


@pytest.mark.parametrize("canonical", (False, True))
@pytest.mark.parametrize("k,lsize,kind", CONFIGS)
def test_regions_of_one_reservation_send_most_items_to_the_table(kt, configs, k, lsize, kind, canonical):
    """cap = kGran: what the regions cannot take is claimed in the table, k-mer by k-mer (the poly-A k-mer a few hundred
    times: one slot, its count); grid 1 and 3, every b1 whose buckets are whole tiles"""
    C = configs(k, lsize, canonical, kind)
    gran = kt.const["kGran"]
    tile_index_bits = C.g["lsize_l"] - C.g["tile_bits"]
    for b1, grid, lo, hi in ((0, 1, 3, 12000), (min(1, tile_index_bits), 3, 8000, 24000), (tile_index_bits, 3, 0, 10000)):
        r = C.check(b1, lo, hi, grid, cap=gran)
        assert r["in_table"] > r["mers"] // 2 and (r["gcur"] > gran).any()


@pytest.mark.parametrize("kind", ("reference", "xs"))
def test_a_shard_takes_the_position_from_the_whole_table_s_matrix(kt, kind):
    """shard 0 of two (shard_bits = 1): the position has lsize_g bits -- the xor-shift hash is evaluated for the whole
    table's width -- and the shard's lsize_l low bits of it place the item; the key's remainder is key >> lsize_g.  2^19 slots:
    the xor-shift hash folds its bits from 17 up into the low ones, so the width it is evaluated for shows in the low bits"""
    k = 40
    C = Config(kt, k, 19, True, kind, sequence(k, 99)[:14000], shard_bits=1)
    try:
        assert C.g["lsize_g"] == C.g["lsize_l"] + 1 == 19
        for b1 in (0, 2):
            r = C.check(b1, 7, 13000, 2)
            assert r["in_table"] == 0
    finally:
        C.t.close()
