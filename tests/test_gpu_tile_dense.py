"""The contract between p2_ring_roles_kernel and the tile kernel: a region written by the loader / storer P2 ends exactly
behind its last item and holds items only (kernels_p1ring.hip.hpp: ring_flush<..., OWNED>), and the flush hands such a
P2 output to the tile kernel's instantiation for hole-free input (kernels_tile.hip.hpp: HOLES = false), which decides
by scalar branches which of a round's rows of 512 items are full, which one is partial and which are empty.

The roles kernel takes buckets of 512 destinations (tables of 2^33 4-byte slots) and of 1024 (2^34): the smallest
geometries that reach it.  Every case asserts from the engine's counters WHICH kernels ran, and the table's content
digest (keys and counts) must equal that of the global-atomic path (set_mode(1)) in a table sized for the input, which the
oracle tests pin.  The inputs walk the per-unit item count through every row case: fewer than one row, several full
rows and a partial one, a second flush into dirty tiles, units of more than one round (9216 items), regions that
overflow (what does not fit is appended behind the exact end or inserted directly)."""
import os

import pytest

pytestmark = pytest.mark.gpu

K, L = 21, 150
_REF = {}


def _big_tables_only():
    if os.environ.get("JFGPU_LIB"):
        pytest.skip("tables of 32 and 64 GB: not under the host emulation")


def _reference(gpu, key, ref_lsize, gen):
    """Digest of the input `gen` writes, counted with global atomics in a table of 2^ref_lsize slots (computed once)."""
    if key not in _REF:
        n_reads = gen[0]
        with gpu.Table(K, 1 << ref_lsize, canonical=True) as ref:
            d = ref.malloc(n_reads * (L + 1) + 16)
            _generate(ref, d, gen)
            ref.set_mode(1)
            ref.count_ascii_dev(d, n_reads * (L + 1)); ref.sync()
            _REF[key] = ref.digest()
            ref.free(d)
    return _REF[key]


def _generate(t, d, gen):
    n_reads, genome, seed = gen
    if genome:
        t.gen_genome_reads_dev(d, 0, n_reads, L, genome, 0.0, seed)
    else:
        t.gen_reads_dev(d, 0, n_reads, L, seed)


def _count_partitioned(gpu, lsize, gen, cuts, reserve_bytes=None):
    """The input through P1 / P2 / T in a table of 2^lsize slots, one flush per cut; returns (digest, counters)."""
    n_reads = gen[0]
    with gpu.Table(K, 1 << lsize, canonical=True) as t:
        assert t.info.slot_bytes == 4
        d = t.malloc(n_reads * (L + 1) + 16)
        _generate(t, d, gen)
        t.set_mode(2)
        t.reserve(reserve_bytes or n_reads * (L + 1))
        t.profile_enable(True); t.profile_reset()
        at = 0
        for cut in list(cuts) + [n_reads]:
            t.count_ascii_dev(d + at * (L + 1), (cut - at) * (L + 1)); t.sync()
            at = cut
        flushes = len(cuts) + 1
        assert t.profile_get(5)[1] >= flushes and t.profile_get(6)[1] >= flushes, "P2 and the tile insert must have run"
        c = t.counters()
        got = t.digest()
        t.free(d)
    assert c["p1_ring"] >= flushes and c["p1_other"] == 0, c
    assert c["p2_roles"] >= flushes and c["p2_sort"] == 0 and c["p2_exact"] == 0 and c["p2_ring"] == 0, c
    return got, c


@pytest.mark.parametrize("lsize", [33, 34])
def test_units_of_less_than_one_row_in_two_flushes(gpu, lsize):
    """143 M k-mers a flush: about 270 items per pair of tiles at 2^33 slots, 135 at 2^34 -- every unit is one partial row.
    The second flush goes into tiles the first left dirty (load_tile).  Launches of 8192 units and more sample themselves:
    the sampling instantiation and the plain one both meet hole-free regions."""
    _big_tables_only()
    gen = (2_200_000, 0, 11)
    want = _reference(gpu, "small", 29, gen)
    assert want[1] == gen[0] * (L - K + 1)
    got, c = _count_partitioned(gpu, lsize, gen, [gen[0] // 2])
    assert c["tile_dense"] >= 2 and c["flushes_plain"] >= 2 and c["flushes_heavy"] == 0, c
    assert c["t_items"] > 0, "the sampling launch did not run"
    assert got == want
    assert c["direct"] < want[1] // 1000


def test_units_of_several_full_rows_and_a_partial_one(gpu):
    """5.8 M uniform reads into 2^33 slots, 4.7 M of them in the first flush: about 1170 items per pair of tiles -- two full rows of 512
    and a partial one, with the row count varying from unit to unit -- then a second flush of 270 items per pair into the
    dirty tiles (1.1 M reads: the smallest batch the single-pass P1 takes)."""
    _big_tables_only()
    gen = (5_800_000, 0, 23)
    want = _reference(gpu, "rows", 31, gen)
    assert want[1] == gen[0] * (L - K + 1)
    got, c = _count_partitioned(gpu, 33, gen, [4_700_000])
    assert c["tile_dense"] >= 2 and c["flushes_heavy"] == 0, c
    assert got == want
    assert c["direct"] < want[1] // 1000


@pytest.mark.parametrize("adapt", ["0", "2"])
def test_units_of_more_than_one_round(gpu, monkeypatch, adapt):
    """Reads without errors from a genome of 1 Mbp, 3000-fold: a pair of tiles holds two of its k-mers on average and
    gets 3000 items for each, so the pairs that hold four or more (one in seven) get 12 000 items and more -- a round of
    9216 (eighteen full rows, no partial one), then a further chunk of full rows and a partial one into the tile as the
    first chunk stored it.  The k-mers are spread over all the destinations, so the rings of P2 take them (a genome of a
    few kbp would send a round's items to a few rings and nearly everything to the straggler lists).  Regions of 16 384
    items; the few pairs with six k-mers and more overflow, and those items are inserted directly.  JFGPU_TILE_ADAPT=0: the
    plain kernel, the hole-free instantiation; 2: the HEAVY kernel, which keeps its hole-aware code, on the same regions."""
    _big_tables_only()
    monkeypatch.setenv("JFGPU_TILE_ADAPT", adapt)
    monkeypatch.setenv("JFGPU_P2_CAP", "16384")
    monkeypatch.setenv("JFGPU_P1_SLACK", "0.3")              # (1000 k-mers a P1 bucket, give or take 30: wider than uniform reads)
    gen = (23_000_000, 1_000_000, 5)
    want = _reference(gpu, "genome", 22, gen)
    assert want[1] == gen[0] * (L - K + 1) and want[0] <= 1_000_000
    got, c = _count_partitioned(gpu, 33, gen, [], reserve_bytes=7_000_000_000)      # (room for 2^19 regions of 16 384 items)
    if adapt == "0":
        assert c["tile_dense"] >= 1 and c["flushes_plain"] >= 1 and c["flushes_heavy"] == 0, c
    else:
        assert c["tile_dense"] == 0 and c["flushes_heavy"] >= 1 and c["flushes_plain"] == 0, c
    assert got == want
    assert c["direct"] < want[1] // 10, c                     # (nearly everything went through the regions)


@pytest.mark.parametrize("cap", [332, 300])
def test_items_appended_behind_a_partial_unit_and_regions_that_overflow(gpu, monkeypatch, cap):
    """Regions too small for some destinations (mean 273 items, standard deviation 16.5).  The storer's cursor stops at a
    multiple of 16 (whole units), a region's further items come through the straggler list and are appended one by one
    behind the exact end -- over the holes a partial last unit stored there -- and what is past the capacity is inserted
    directly.  The tile kernel then reads [begin, end) as items only.
    332: the cursor stops at 320, which one region in 500 passes, and one in 5000 passes 332 -- a few hundred direct
    inserts, far below a thousandth of the input.  300: the cursor stops at 288, which one region in six passes; the
    storers then spend their time on the list, rings run full behind them and their items go on the list too, until it
    is full -- how much ends up inserted directly is not bounded here, the table's content is what is checked."""
    _big_tables_only()
    monkeypatch.setenv("JFGPU_P2_CAP", str(cap))
    gen = (2_200_000, 0, 11)
    want = _reference(gpu, "small", 29, gen)
    got, c = _count_partitioned(gpu, 33, gen, [gen[0] // 2])
    assert c["tile_dense"] >= 2, c
    assert got == want
    assert c["direct"] > 0, c
    if cap == 332:
        assert c["direct"] < want[1] // 1000, c
