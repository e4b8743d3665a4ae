"""The partitioned Bloom insert for mers of 33 to 128 bases, end to end through the C ABI (-m gpu): jfgpu_bc_set_mode(b, 2)
is accepted for keys of two, three and four words, P1b is p1_bloom_keys_kernel (kernels_bloom_part_keys.hip.hpp), and from
P2 onwards the path is the one-word keys' own.  Mode 2 leaves the bytes mode 1 leaves, which are the oracle's
(jfo_bc_insert, bloom_counter2.hpp:56-107 restated) and the reference's files'; every call that reads the counter sees the
updates that are still pending."""
import json
import os
import random

import numpy as np
import pytest

import oracle_lib as O
from test_gpu_bloom_nword import input_kmers, oracle_check, random_input, rows, table_map
from test_gpu_bloom_query import bloom_expected
from test_gpu_query import check
from test_oracle import read_bc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CASES = json.load(open(os.path.join(GOLD, "bloom_nword.json")))["bloom"]

SMALL, TWO_LEVEL = 14 * 150000, 14 * 30_000_000           # one level (seven segments); 1282 segments: P2 is on the path


@pytest.mark.parametrize("k", [33, 63, 64, 65, 100, 128])
def test_set_mode_2_is_accepted(gpu, k):
    """(the parent answers E_UNSUPPORTED for every one of these)"""
    with gpu.Bloom(k, SMALL, 10, canonical=True, seed=9) as b:
        b.set_mode(2)
        b.set_mode(0)
        b.set_mode(1)
        b.set_mode(2)


def test_set_mode_2_is_still_refused_without_a_geometry(gpu):
    """a one-pass filter (kind 1) has no segment geometry, whatever the key's width"""
    with gpu.Bloom(100, 100000, 7, canonical=True, one_pass_filter=True) as bf:
        with pytest.raises(gpu.JfgpuError) as e:
            bf.set_mode(2)
        assert e.value.code == gpu.E_UNSUPPORTED


@pytest.fixture(scope="module")
def batches():
    rng = random.Random(17)
    seq = ("".join(rng.choice("ACGT") for _ in range(90000)) + "N" + "".join(rng.choice("ACGTacgtN") for _ in range(30000))).encode()
    return seq + seq[:50000] + seq[:20000]                      # parts of it two and three times: cells saturate


_ORACLE = {}


def oracle_bytes(seq, k, m1, m2, n_cells, nh):
    """the jfo_bc_insert loop over every k-mer of seq, once per (input, k, matrices)"""
    at = (hash(seq), k, n_cells, nh, m1.tobytes(), m2.tobytes())
    if at not in _ORACLE:
        kmers = O.extract(seq, k, True)
        h0, h1 = O.matrix_times(m1, 64, 2 * k, kmers), O.matrix_times(m2, 64, 2 * k, kmers)
        data = np.zeros(n_cells // 5 + (n_cells % 5 != 0), dtype=np.uint8)
        L = O.lib()
        for x, y in zip(h0.tolist(), h1.tolist()):
            L.jfo_bc_insert(data.ctypes.data, n_cells, nh, x, y)
        _ORACLE[at] = data
    return _ORACLE[at]


@pytest.mark.parametrize("k,n_cells,env", [(33, SMALL, None), (63, SMALL, None), (64, SMALL, None), (65, SMALL, None), (100, SMALL, None), (128, SMALL, None),
                                           (63, TWO_LEVEL, None), (65, TWO_LEVEL, None), (128, TWO_LEVEL, None),
                                           (100, TWO_LEVEL, "share4"), (64, TWO_LEVEL, "single2")],
                         ids=lambda v: {SMALL: "small", TWO_LEVEL: "twolevel", None: "plain"}.get(v, str(v)))
def test_partitioned_insert_equals_direct_and_oracle(gpu, monkeypatch, batches, k, n_cells, env):
    """tests/test_gpu_bloom.py's test of the same name on keys of two to four words: several batches per flush, saturation
    at 2, a flush in the middle (check on encoded keys), inserts after it; with more than 1024 segments P2 is on the path;
    share4: P2 and the segment kernel go through the P1b buckets in four groups that share one output buffer; single2: the
    single-pass P2 forced on."""
    monkeypatch.setenv("JFGPU_P2_SINGLE", "2" if env == "single2" else "0")
    if env == "share4":
        monkeypatch.setenv("JFGPU_FLUSH_SHARE", "4")
    two_level = n_cells == TWO_LEVEL
    seq, nh = batches, 10
    windows = len(O.extract(seq, k, True))
    out = {}
    for mode in (1, 2):
        with gpu.Bloom(k, n_cells, nh, canonical=True, seed=9) as b:
            b.set_mode(mode)
            b.profile_enable(True)
            third = len(seq) // 3
            b.insert_ascii(seq[:third])
            b.insert_ascii(seq[third - (k - 1): 2 * third])
            kmers = O.extract(seq[:third], k, True)
            assert (b.keys(np.ascontiguousarray(kmers[::501])) >= 1).all()          # flushes what is pending
            b.insert_ascii(seq[2 * third - (k - 1):])
            assert b.sync() == windows
            out[mode] = b.read()
            used = [b.profile_get(i)[1] for i in range(4)]
            if mode == 2:
                assert used[1] > 0 and used[3] > 0 and (used[2] > 0) == two_level, used
            else:
                assert used[1] == 0 and used[0] > 0
            m1, m2 = b.matrix1, b.matrix2
    assert (out[1] == out[2]).all()
    if not two_level:
        assert (out[2] == oracle_bytes(seq, k, m1, m2, n_cells, nh)).all()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_reference_files_in_mode_2(gpu, case):
    """The bodies of bc_k100C.ref.bc and bc_k65.ref.bc under the files' own matrices: a single segment, (0, 0)."""
    header, body = read_bc(os.path.join(GOLD, case["ref_bc"]))
    k, can = case["k"], case["canonical"]
    m1 = np.array(header["matrix1"]["columns"], dtype=np.uint64)
    m2 = np.array(header["matrix2"]["columns"], dtype=np.uint64)
    seq = O.parse_file(open(os.path.join(GOLD, case["input"]), "rb").read())
    with gpu.Bloom(k, header["size"], header["nb_hashes"], canonical=can, matrix1=m1, matrix2=m2) as b:
        assert b.nb_bytes == len(body) <= 1 << 16
        b.set_mode(2)
        b.profile_enable(True)
        b.insert_ascii(seq)
        assert b.sync() == len(O.extract(seq, k, can))
        assert (b.read() == body).all()
        assert b.profile_get(1)[1] > 0 and b.profile_get(3)[1] > 0 and b.profile_get(0)[1] == 0


@pytest.mark.parametrize("k", [100, 128])
def test_attach_sees_pending_updates(gpu, k):
    """attach_bloom to a four-word table straight after an un-synced mode-2 insert: the table admits exactly what
    jfo_bc_check > 1 admits on the bytes read back afterwards, which are the oracle's."""
    seq, kmers = random_input(k), input_kmers(k, True)
    m, nh = gpu.opt_m(0.001, len(kmers)), gpu.opt_k(0.001)
    uniq, first_at, cnt = np.unique(kmers, axis=0, return_index=True, return_counts=True)
    with gpu.Bloom(k, m, nh, canonical=True, seed=5 + k) as b, gpu.Table(k, 1 << 16, canonical=True) as t:
        b.set_mode(2)
        b.profile_enable(True)
        b.insert_ascii(seq)
        assert b.profile_get(1)[1] > 0 and b.profile_get(3)[1] == 0, "nothing is pending: the case does not test the flush"
        t.attach_bloom(b)
        assert b.profile_get(3)[1] > 0
        t.count_ascii(seq)
        t.sync()
        got = table_map(gpu, t, k)
        t.attach_bloom(None)
        data = b.read()
        h0 = O.matrix_times(b.matrix1, 64, 2 * k, kmers).tolist()
        h1 = O.matrix_times(b.matrix2, 64, 2 * k, kmers).tolist()
        assert (data == oracle_bytes(seq, k, b.matrix1, b.matrix2, m, nh)).all()
        adm = oracle_check(data, m, nh, [h0[i] for i in first_at.tolist()], [h1[i] for i in first_at.tolist()]) > 1
        exp = {key: c for key, c, a in zip(rows(uniq), cnt.tolist(), adm.tolist()) if a}
        assert 5000 < len(exp) < len(uniq)
        assert got == exp


@pytest.mark.parametrize("k", [63, 100])
def test_query_ascii_sees_pending_updates(gpu, k):
    """query_ascii after an un-synced mode-2 insert answers from the oracle's bytes (the query: bases fed twice, bases fed once,
    bases never fed)"""
    seq = random_input(k)
    n = len(input_kmers(k, True))
    m, nh = gpu.opt_m(0.001, n), gpu.opt_k(0.001)
    query = seq[8000:12000] + b"N" + "".join(random.Random(k).choice("ACGT") for _ in range(3000)).encode()
    with gpu.Bloom(k, m, nh, canonical=True, seed=5 + k) as b:
        b.set_mode(2)
        b.profile_enable(True)
        b.insert_ascii(seq)
        assert b.profile_get(3)[1] == 0
        got = b.query_ascii(query)
        assert b.profile_get(3)[1] > 0
        want = bloom_expected(query, k, True, oracle_bytes(seq, k, b.matrix1, b.matrix2, m, nh), m, nh, b.matrix1, b.matrix2)
        check(got, want, "k = %d" % k)
        assert set(want[0].tolist()) == {0, 1, 2}


@pytest.mark.parametrize("k", [63, 100])
def test_auto_takes_the_partitioned_path_from_1_mib(gpu, k):
    """Mode 0: bloom_keys_auto_partitioned (bloom_partition.inl) as profiles/bloom_keys_part_rate.txt left it -- a batch of
    1 MiB of sequence and more is routed (stage 1 launches), a smaller one takes the direct kernel; the bytes are mode 1's."""
    small = random_input(k)
    big = small * 27                                            # 1.08 MB
    assert len(small) < (1 << 20) <= len(big)
    with gpu.Bloom(k, 64 * 5 * 65536, 10, canonical=True, seed=9) as b, gpu.Bloom(k, 64 * 5 * 65536, 10, canonical=True, seed=9) as d:
        b.profile_enable(True)
        b.insert_ascii(small)
        b.sync()
        used = [b.profile_get(i)[1] for i in range(4)]
        assert used[0] > 0 and used[1] == 0 and used[3] == 0, used
        b.profile_reset()
        b.insert_ascii(big)
        b.sync()
        used = [b.profile_get(i)[1] for i in range(4)]
        assert used[1] > 0 and used[3] > 0, used
        d.set_mode(1)
        d.insert_ascii(small)
        d.insert_ascii(big)
        assert d.sync() == b.sync()
        assert (b.read() == d.read()).all()
