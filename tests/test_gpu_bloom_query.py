"""jfgpu_bc_query_ascii(_dev) on the GPU (-m gpu): check() of every k-mer of a contract buffer against a Bloom counter in
one kernel (bloom_query_ascii_kernel, jellyfish_amd/csrc/kernels_bloom_query.hip.hpp), for the three key views -- what
`query -s` asks of a bloomcounter database (sub_commands/query_main.cc:44-51, :99-104).

The expected answer is built from the counter's own bytes (Bloom.read(), or the body of a reference file) through
tests/oracle_lib.py alone: the end positions of the windows are those whose last k bytes are all in ACGTacgt; O.extract gives
the keys there, canonical and as the text has them (their difference is the reverse-complement bit); O.matrix_times with the
counter's two matrices and jfo_bc_check (bloom_counter2.hpp:109-142 restated) give check().  vals and flags are compared
exactly, entry by entry, over all n."""
import json
import os
import random

import numpy as np
import pytest

import oracle_lib as O
from test_gpu_bloom_nword import oracle_check
from test_gpu_query import FOUND, MER, REVCOMP, TILE, check, end_positions, palindrome, revcomp, rnd_seq
from test_oracle import read_bc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def bloom_expected(seq, k, canonical, data, m, nh, m1, m2):
    """(vals, flags) that a counter of m cells and nh hashes holding the bytes `data` under the matrices m1, m2 must answer."""
    n = len(seq)
    vals = np.zeros(n, dtype=np.uint64)
    flags = np.zeros(n, dtype=np.uint8)
    ends = end_positions(seq, k)
    keys = np.ascontiguousarray(O.extract(seq, k, canonical))
    text = np.ascontiguousarray(O.extract(seq, k, False))
    assert len(keys) == len(ends) == len(text)
    if not len(ends):
        return vals, flags
    data = np.ascontiguousarray(data, dtype=np.uint8)
    chk = oracle_check(data, m, nh, O.matrix_times(m1, 64, 2 * k, keys).tolist(), O.matrix_times(m2, 64, 2 * k, keys).tolist())
    rc = (keys != text).any(axis=1) if canonical else np.zeros(len(ends), dtype=bool)
    vals[ends] = chk
    flags[ends] = MER | np.where(chk != 0, FOUND, 0).astype(np.uint8) | np.where(rc, REVCOMP, 0).astype(np.uint8)
    return vals, flags


def expected_of(b, seq, canonical, data=None):
    return bloom_expected(seq, b.k, canonical, b.read() if data is None else data, b.m, b.nb_hashes, b.matrix1, b.matrix2)


# ---- every key view and its edges ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", [True, False], ids=["C", "fw"])
@pytest.mark.parametrize("k", [1, 12, 21, 31, 32, 33, 40, 63, 64, 65, 96, 97, 128])
def test_every_key_view_against_the_oracle(gpu, k, canonical):
    rng = random.Random(2000 * k + canonical)
    twice = rnd_seq(rng, 1500 + k)                                        # inserted twice
    once = rnd_seq(rng, 700) + b"A" * (k + 20) + rnd_seq(rng, 800 + k, "ACGTacgt")     # once: a homopolymer run, lower case
    inserted = once + b"N" + twice
    n_inserted = len(end_positions(inserted, k)) + len(end_positions(twice, k))
    parts = [once[100:], twice[:750 + k], revcomp(twice[700:]), rnd_seq(rng, 1600 + k), b"n", once[:k + 3]]
    if k % 2 == 0:
        parts += [palindrome(rng, k), palindrome(rng, k)]
    query = b"N".join(parts)
    with gpu.Bloom(k, gpu.opt_m(0.001, n_inserted), gpu.opt_k(0.001), canonical=canonical, seed=k + 1) as b:
        b.insert_ascii(inserted)
        b.insert_ascii(twice)
        fed = b.sync()
        assert fed == n_inserted
        want = expected_of(b, query, canonical)
        check(b.query_ascii(query), want, "k = %d" % k)
        assert b.sync() == fed                                            # (the tally is the insert's: a query leaves it alone)
        mers = int((want[1] & MER != 0).sum())
        assert mers > 4500
        if k > 1:                                                         # no constant answer can pass
            for answer in (0, 1, 2):
                assert 10 * int(((want[0] == answer) & (want[1] & MER != 0)).sum()) >= mers, (answer, mers)
            assert ((want[1] & FOUND != 0) == (want[0] != 0)).all()
        if canonical and k > 1:
            assert (want[1] & REVCOMP != 0).sum() > 500
        if not canonical:
            assert not (want[1] & REVCOMP).any()
        if k % 2 == 0 and canonical:                                      # a palindrome is its own reverse complement
            assert want[1][len(query) - 1] & (MER | REVCOMP) == MER


@pytest.mark.parametrize("k", [21, 40, 100])
def test_a_counter_of_1009_cells(gpu, k):
    """The reduction modulo a small m: h % m leaves nearly all of the hash's bits to the reciprocal's correction steps."""
    rng = random.Random(k)
    text = rnd_seq(rng, 60 + k)
    query = text[:40 + k] + b"N" + text[10:30 + k] + b"N" + rnd_seq(rng, 3000)
    with gpu.Bloom(k, 1009, 3, canonical=True, seed=5) as b:
        b.insert_ascii(text)
        b.insert_ascii(text[:30 + k])
        want = expected_of(b, query, True)
        check(b.query_ascii(query), want, "m = 1009, k = %d" % k)
        assert set(want[0][want[1] & MER != 0].tolist()) == {0, 1, 2}


# ---- the reference's files -------------------------------------------------------------------------------------------------
def golden_cases():
    cases = json.load(open(os.path.join(GOLD, "manifest.json")))["bloom"] + json.load(open(os.path.join(GOLD, "bloom_nword.json")))["bloom"]
    assert sorted(c["ref_bc"] for c in cases) == ["bc_k100C.ref.bc", "bc_k21C.ref.bc", "bc_k31.ref.bc", "bc_k65.ref.bc"]
    return cases


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_reference_files(gpu, case):
    """The body `jellyfish bc` wrote, loaded under its header's matrices, answers for the file's own input what the oracle
    reads out of that body."""
    header, body = read_bc(os.path.join(GOLD, case["ref_bc"]))
    k, can = case["k"], case["canonical"]
    m1 = np.array(header["matrix1"]["columns"], dtype=np.uint64)
    m2 = np.array(header["matrix2"]["columns"], dtype=np.uint64)
    seq = O.parse_file(open(os.path.join(GOLD, case["input"]), "rb").read())
    with gpu.Bloom(k, header["size"], header["nb_hashes"], canonical=can, matrix1=m1, matrix2=m2) as b:
        assert b.nb_bytes == len(body)
        b.load(body)
        want = expected_of(b, seq, can, data=body)
        check(b.query_ascii(seq), want, case["name"])
        answers = want[0][want[1] & MER != 0]
        assert len(answers) > 3000 and (answers >= 1).all()               # (its own input: everything was inserted)
        assert 10 * (answers == 2).sum() > len(answers) and 10 * (answers == 1).sum() > len(answers)
        other = rnd_seq(random.Random(k), 2000)                           # and for sequence it never saw
        check(b.query_ascii(other), expected_of(b, other, can, data=body), case["name"] + ", random sequence")


# ---- tile edges: halo staging and window reset across lanes and tiles, for each view's halo (2, 4 and 8 words) -------------
@pytest.fixture(scope="module")
def edge_text():
    return rnd_seq(random.Random(6), 3 * TILE + 7 + 300)


@pytest.mark.parametrize("k", [21, 40, 100])
def test_tile_edges(gpu, edge_text, k):
    with gpu.Bloom(k, gpu.opt_m(0.001, 2 * len(edge_text)), gpu.opt_k(0.001), canonical=True, seed=9) as b:
        b.insert_ascii(edge_text[:2 * TILE + 50])
        b.insert_ascii(edge_text[TILE - 300:TILE + 300])
        data = b.read()
        exp = lambda q: expected_of(b, q, True, data=data)
        for n in (0, 1, k - 1, k, k + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 7):
            q = edge_text[:n]
            check(b.query_ascii(q), exp(q), "length %d" % n)
        base = bytearray(edge_text[:TILE + 200])
        for off in (15, 16, 17, TILE - 1, TILE, TILE + 1):
            for what, put in (("N", b"N"), ("lower case", bytes(base[off:off + 2 * k + 5]).lower()), ("IUPAC", b"R")):
                q = bytearray(base)
                q[off:off + len(put)] = put
                q = bytes(q)
                want = exp(q)
                check(b.query_ascii(q), want, "%s at %d" % (what, off))
                if what == "lower case":                                  # the same answers as in upper case
                    check(want, exp(bytes(base)), "oracle, lower case at %d" % off)
        # a run of bases that ends exactly at the tile's last position, the next run starts with the next tile
        q = edge_text[:TILE - 1 - 2 * k] + b"N" + edge_text[500:500 + 2 * k] + edge_text[700:700 + 3 * k]
        assert q[TILE - 1 - 2 * k] == ord("N") and len(q) > TILE + k
        want = exp(q)
        check(b.query_ascii(q), want, "runs meeting at the tile edge")
        q = q[:TILE] + b"N" + q[TILE + 1:]                                # ... and the second run is cut off from it
        want2 = exp(q)
        assert (want2[1][TILE:TILE + k] == 0).all() and (want[1][TILE:TILE + k] != 0).all()
        check(b.query_ascii(q), want2, "a reset on the tile's first position")
        q = q[:TILE - 1] + b"N" + edge_text[TILE:TILE + 3 * k]            # ... or the reset is the tile's last position and a run starts the next tile
        check(b.query_ascii(q), exp(q), "a run that starts with the tile")


# ---- device form: unaligned sequence pointer, guards behind the outputs, no flags ------------------------------------------
@pytest.mark.parametrize("k", [21, 40, 100])
def test_unaligned_device_buffers_and_guards(gpu, k):
    rng = random.Random(78 + k)
    text = rnd_seq(rng, 6000, "ACGTN" if k == 21 else "ACGT")
    with gpu.Bloom(k, gpu.opt_m(0.001, 8000), gpu.opt_k(0.001), canonical=True, seed=3) as b, gpu.Table(21, 1 << 12) as mem:
        b.insert_ascii(text[:4000])
        b.insert_ascii(text[1000:2500])
        fed = b.sync()
        data = b.read()
        pad = 32
        d_seq = mem.malloc(len(text) + 4 * pad)
        d_vals = mem.malloc(8 * (len(text) + 2))
        d_flags = mem.malloc(len(text) + 32)
        try:
            for shift, n in ((0, TILE + 48), (1, 5000), (7, TILE + 9), (15, 4999), (0, 4993)):
                q = text[200:200 + n]
                # bases before and after the buffer: a kernel reading outside [0, n) would see windows that are not there
                mem.h2d(d_seq, np.frombuffer(b"ACGT" * (pad // 4) + text[200 - shift:200] + q + b"ACGT" * (pad // 2), dtype=np.uint8))
                want = expected_of(b, q, True, data=data)
                for with_flags in (True, False):
                    mem.h2d(d_vals, np.full(n + 2, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64))
                    mem.h2d(d_flags, np.full(n + 32, 0xEE, dtype=np.uint8))
                    b.query_ascii_dev(d_seq + pad + shift, n, d_vals, d_flags if with_flags else None)
                    assert b.sync() == fed                                # waits for the counter's stream; the tally is unchanged
                    gv = mem.d2h(d_vals, 8 * (n + 2)).view(np.uint64)
                    gf = mem.d2h(d_flags, n + 32)
                    assert (gv[n:] == 0xA5A5A5A5A5A5A5A5).all() and (gf[n:] == 0xEE).all(), "written beyond n"
                    if not with_flags:                                    # flags == NULL: the same answers, and nothing written for the flags
                        assert (gf == 0xEE).all()
                        gf = want[1]
                    check((gv[:n].copy(), gf[:n].copy()), want, "pointer + %d, n = %d, flags %s" % (shift, n, with_flags))
            assert (b.read() == data).all()                               # the counter is only read
        finally:
            mem.free(d_seq); mem.free(d_vals); mem.free(d_flags)


# ---- pending partitioned increments ------------------------------------------------------------------------------------------
def test_query_sees_pending_partitioned_increments(gpu):
    rng = random.Random(42)
    k = 21
    text = b"N".join(rnd_seq(rng, 4000) for _ in range(10))
    q = text[1000:5000] + b"N" + rnd_seq(rng, 2000)
    with gpu.Bloom(k, gpu.opt_m(0.001, 50000), gpu.opt_k(0.001), canonical=True, seed=11) as b, gpu.Table(21, 1 << 12) as mem:
        b.set_mode(2)
        b.profile_enable()
        d_seq = mem.malloc(len(text) + 16)
        try:
            mem.h2d(d_seq, np.frombuffer(text, dtype=np.uint8))
            b.insert_ascii_dev(d_seq, len(text))                          # no sync: the cell updates are pending in the workspace
            got = b.query_ascii(q)
            assert b.profile_get(1)[1] > 0, "the partitioned path did not run"
            want = expected_of(b, q, True)
            check(got, want, "after an un-synced partitioned insert")
            found = int((want[1] & FOUND != 0).sum())
            assert found >= 3900 and int((want[1] & MER != 0).sum()) - found > 1500
        finally:
            mem.free(d_seq)


# ---- errors ---------------------------------------------------------------------------------------------------------------
def test_errors(gpu):
    lib = gpu.load()
    seq = np.frombuffer(b"ACGTACGTACGTACGTACGTACGTACGT", dtype=np.uint8)
    vals, flags = np.zeros(len(seq), dtype=np.uint64), np.zeros(len(seq), dtype=np.uint8)
    with gpu.Bloom(21, 10000, 3) as b:
        for fn in (lib.jfgpu_bc_query_ascii, lib.jfgpu_bc_query_ascii_dev):
            assert fn(b._h, None, 0, None, None) == gpu.OK                           # nothing asked
            assert fn(b._h, seq.ctypes.data, 0, None, None) == gpu.OK
            assert fn(b._h, None, len(seq), vals.ctypes.data, flags.ctypes.data) == gpu.E_INVALID
            assert fn(b._h, seq.ctypes.data, len(seq), None, flags.ctypes.data) == gpu.E_INVALID
            assert fn(None, seq.ctypes.data, len(seq), vals.ctypes.data, flags.ctypes.data) == gpu.E_INVALID
        v, f = b.query_ascii(b"")
        assert len(v) == 0 and len(f) == 0
    with gpu.Bloom(21, 10000, 3, one_pass_filter=True) as b:
        for fn in (lib.jfgpu_bc_query_ascii, lib.jfgpu_bc_query_ascii_dev):
            assert fn(b._h, seq.ctypes.data, len(seq), vals.ctypes.data, flags.ctypes.data) == gpu.E_UNSUPPORTED
            assert b"one-pass" in lib.jfgpu_last_error()
