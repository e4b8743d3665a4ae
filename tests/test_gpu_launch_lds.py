"""A kernel's dynamic-LDS limit is raised by its launch (jellyfish_amd/csrc/hip_launch.hpp), not by a list in a create function:

  * the limit follows a table that grows: the dump kernel of a table of 2^12 slots asks for little LDS, the same table doubled
    to 2^14 slots (tiles of 2^13) for more than 64 KiB -- dump_tiles_kernel for one-word keys, dump_tiles_words_kernel (whose
    limit the doubling itself used to set) for two-word keys;
  * a process that never creates a table can run the partitioned Bloom insert, whose kernels' limits used to be spread over
    the two create functions."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def distinct_keys(rng, k, n, start):
    """n keys of k bases no two of which are equal, nor equal to a key of an earlier call with a smaller `start`: the low
    word counts up from `start` through an odd multiplier (a bijection of 32 bits), the high bits of a two-word key are random"""
    lo = ((np.arange(start, start + n, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF))
    if k <= 32:
        return lo
    hi = rng.integers(0, 1 << (2 * k - 64), n, dtype=np.uint64)
    return np.stack([lo | (rng.integers(0, 1 << 32, n, dtype=np.uint64) << np.uint64(32)), hi], axis=1)


def sorted_pairs(keys, cnts):
    """(key, count) sorted by key; keys (n,) or (n, 2) little-endian words"""
    keys = np.asarray(keys, dtype=np.uint64).reshape(len(cnts), -1)
    order = np.lexsort(tuple(keys[:, w] for w in range(keys.shape[1])))
    return keys[order], np.asarray(cnts, dtype=np.uint64)[order]


def expected_pairs(added):
    keys = np.concatenate(added).reshape(-1, added[0].reshape(len(added[0]), -1).shape[1])
    uniq, cnts = np.unique(keys, axis=0, return_counts=True)
    return sorted_pairs(uniq, cnts)


def dumped_pairs(capi, t):
    keys, cnts = capi.decode_records(t.dump_records(), t.k, t.info.out_counter_len)
    return sorted_pairs(keys, cnts)


@pytest.mark.parametrize("k,size", [(16, 1 << 12), (40, 1)])
def test_the_dump_limit_follows_a_table_that_grows(gpu, k, size):
    """k = 16 from 2^12 slots; k = 40 from the smallest legal size (tiles of 2^13 slots from the start: the first dump is
    already beyond 64 KiB, the one after the doubling runs on the table grow_swap built)"""
    capi = gpu
    rng = np.random.default_rng(k)
    with capi.Table(k, size, canonical=False) as t:
        t.set_growth(True)
        start = int(t.info.lsize)
        if k == 16:
            assert start == 12 and int(t.info.tile_slots) == 1 << 12
        added = [distinct_keys(rng, k, 3000, 0)]
        t.add_keys(added[0])
        added.append(added[0][:500])                 # (counts of 2 as well)
        t.add_keys(added[1])
        t.sync()
        got, want = dumped_pairs(capi, t), expected_pairs(added)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        target = max(14, start + 1)
        n, step = 3000, max(2000, (1 << start) // 4)
        for _ in range(16):
            if int(t.info.lsize) >= target:
                break
            more = distinct_keys(rng, k, step, n)
            n += step
            added.append(more)
            t.add_keys(more)
            t.sync()
        assert int(t.info.lsize) >= target, "the table did not grow"
        assert int(t.info.tile_slots) == 1 << 13
        got, want = dumped_pairs(capi, t), expected_pairs(added)
        assert len(want[1]) == n
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


BLOOM_ONLY = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from jellyfish_amd import capi
rng = np.random.default_rng(5)
seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 200000)].tobytes()
SEG = 5 * (64 << 10)
for m, nh in ((7, 10), (8 * SEG - 3, 7)):
    bodies = []
    for mode in (2, 1):                       # partitioned, direct (jfgpu_bc_set_mode)
        b = capi.Bloom(31, m, nh, canonical=True)
        b.set_mode(mode)
        b.insert_ascii(seq)
        b.sync()
        bodies.append(b.read().copy())
        b.close()
    assert bodies[0].any(), "nothing was inserted"
    assert np.array_equal(bodies[0], bodies[1]), "m = %d: the partitioned insert and the direct insert disagree" % m
print("bloom only: ok")
"""


def test_a_process_with_only_a_bloom_counter_runs_the_partitioned_insert(gpu):
    """in a fresh child process, no table ever created: a Bloom counter at the smallest geometry tests/test_gpu_stage_bloom_p1.py
    uses (m = 7: one segment), and at its eight segments, takes one buffer through the partitioned insert (mode 2) and holds
    what the direct insert (mode 1) produces from the same buffer"""
    r = subprocess.run([sys.executable, "-c", BLOOM_ONLY, ROOT], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "bloom only: ok" in r.stdout
