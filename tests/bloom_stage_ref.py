"""The reference of the Bloom stage tests (tests/test_gpu_stage_bloom_*.py): the partitioned Bloom insert restated in numpy
on 64-bit integers.  Not a test module.

  h0 = M1 * key, h1 = M2 * key                       (oracle_lib.matrix_times over the counter's two matrices)
  cell_i = (h0 % m + i * (h1 % m)) % m, i < nh       (bloom_counter2's double hashing)
  byte = cell // 5, digit = cell % 5, segment = byte >> 16, bucket = segment >> b2
  item = (segment & (2^b2 - 1)) << 19 | (byte & 0xFFFF) << 3 | digit          (kernels_bloom_part.hip.hpp's header)
  the filter after a multiset of cell updates over a starting filter: per cell min(start + count, 2), five base-3 digits a byte

An update is carried as bucket << 32 | item in one uint64.  check_against_oracle() ties this restatement to jfo_bc_insert
(oracle/jf_oracle.c), once a process."""
import numpy as np

import oracle_lib as O

SEG_BITS, ITEM_LOW = 16, 19
SEG_CELLS = 5 << SEG_BITS
POW3 = np.array([1, 3, 9, 27, 81], dtype=np.int64)
U = np.uint64


def hashes(bloom, kmers):
    k = bloom.k
    return O.matrix_times(bloom.matrix1, 64, 2 * k, kmers), O.matrix_times(bloom.matrix2, 64, 2 * k, kmers)


def cells_of_hashes(h0, h1, m, nh):
    """(n, nh) cells; i * (h1 % m) stays below 2^63 for every filter here (asserted)"""
    assert nh * m < (1 << 62)
    a, inc = h0 % U(m), h1 % U(m)
    i = np.arange(nh, dtype=np.uint64)[None, :]
    return (a[:, None] + i * inc[:, None]) % U(m)


def cells_of(bloom, seq, lo, hi, canonical):
    """the cells of every k-mer occurrence of seq[lo:hi], flat, and the number of windows"""
    kmers = O.extract(bytes(seq[lo:hi]), bloom.k, canonical)
    if len(kmers) == 0:
        return np.zeros(0, dtype=np.uint64), 0
    h0, h1 = hashes(bloom, kmers)
    return cells_of_hashes(h0, h1, bloom.m, bloom.nb_hashes).reshape(-1), len(kmers)


def updates_of_cells(cells, b2):
    """bucket << 32 | item of every cell"""
    cells = np.asarray(cells, dtype=np.uint64)
    byte, dig = cells // U(5), cells % U(5)
    seg = byte >> U(SEG_BITS)
    item = ((seg & U((1 << b2) - 1)) << U(ITEM_LOW)) | ((byte & U(0xFFFF)) << U(3)) | dig
    return ((seg >> U(b2)) << U(32)) | item


def cells_of_updates(upd, b2):
    upd = np.asarray(upd, dtype=np.uint64)
    item = upd & U(0xFFFFFFFF)
    seg = ((upd >> U(32)) << U(b2)) | (item >> U(ITEM_LOW))
    return ((seg << U(SEG_BITS)) | ((item >> U(3)) & U(0xFFFF))) * U(5) + (item & U(7))


def expected_filter(start, cells):
    """start (bytes, each < 243) after the multiset of cell updates: per cell min(start + count, 2); touches only the bytes hit"""
    out = np.array(start, dtype=np.uint8, copy=True)
    if len(cells) == 0:
        return out
    uc, cnt = np.unique(np.asarray(cells, dtype=np.uint64), return_counts=True)
    byte, dig = (uc // U(5)).astype(np.int64), (uc % U(5)).astype(np.int64)
    assert byte.max() < len(out)
    old = (out[byte].astype(np.int64) // POW3[dig]) % 3
    delta = (np.minimum(old + cnt, 2) - old) * POW3[dig]
    ub, inv = np.unique(byte, return_inverse=True)
    out[ub] = (out[ub].astype(np.int64) + np.bincount(inv, weights=delta).astype(np.int64)).astype(np.uint8)
    return out


def multiset_minus(whole, part, what="entries"):
    """whole - part as sorted multisets of uint64; part must be contained in whole"""
    uw, cw = np.unique(np.asarray(whole, dtype=np.uint64), return_counts=True)
    if len(part):
        up, cp = np.unique(np.asarray(part, dtype=np.uint64), return_counts=True)
        at = np.searchsorted(uw, up)
        assert (at < len(uw)).all() and (uw[np.minimum(at, len(uw) - 1)] == up).all(), "%s that the reference does not have" % what
        cw[at] -= cp
        assert (cw >= 0).all(), "%s more often than the reference has them" % what
    return np.repeat(uw, cw)


def saturated_share(cells):
    """the share of a multiset's updates that fall on cells which the multiset alone takes beyond 2"""
    if len(cells) == 0:
        return 0.0
    _, cnt = np.unique(cells, return_counts=True)
    return float(cnt[cnt > 2].sum()) / len(cells)


def assert_saturation_cannot_hide(cells):
    """the condition of the overflow shapes: at most 1 % of the reference's updates fall on cells it saturates by itself, so a
    dropped or doubled update among those that went straight to the filter changes its bytes"""
    share = saturated_share(cells)
    assert share <= 0.01, "%.2f %% of the updates fall on cells the input alone takes beyond 2" % (100 * share)


_checked = False


def check_against_oracle(bloom, seq, canonical):
    """once: expected_filter(cells_of(...)) equals the oracle's bloom_counter2 restatement fed the same hashes"""
    global _checked
    if _checked:
        return
    kmers = O.extract(bytes(seq), bloom.k, canonical)
    h0, h1 = hashes(bloom, kmers)
    data = np.zeros(bloom.nb_bytes, dtype=np.uint8)
    L = O.lib()
    for x, y in zip(h0.tolist(), h1.tolist()):
        L.jfo_bc_insert(data.ctypes.data, bloom.m, bloom.nb_hashes, x, y)
    mine = expected_filter(np.zeros(bloom.nb_bytes, dtype=np.uint8), cells_of_hashes(h0, h1, bloom.m, bloom.nb_hashes).reshape(-1))
    assert (mine == data).all(), "the numpy restatement and jfo_bc_insert disagree"
    _checked = True
