"""Bloom counters and one-pass Bloom filters for mers of 65 to 128 bases on the GPU (-m gpu): `bc`, `count --bc` and
`count --bf-size` over keys of three and four words (kernels_nword.hip.hpp: bloom_insert_ascii_nword_kernel,
bloom_keys_nword_kernel, the filter in count_ascii_nword_kernel), byte-exact against the reference's files and against the
oracle's restatement of bloom_counter2.hpp:56-142.

The fixtures tests/golden/bc_k100C.* and bc_k65.* (listed in bloom_nword.json) are the reference's own output on
reads150_dup.fa, produced the way oracle/gen_golden.py produces bc_k21C.* and bc_k31.*, from tests/golden with
SOURCE_DATE_EPOCH=0:

    ref_jf bc [-C] -m K -s 9000 -f 0.001 -t 2 -o bc_kK[C].ref.bc reads150_dup.fa
    ref_jf count [-C] -m K -s 64k -t 2 --bc bc_kK[C].ref.bc -o f.jf reads150_dup.fa
    ref_jf dump -c f.jf | sort > bc_kK[C].filtered.dump

with (K, -C) = (100, yes) and (65, no).  In the two headers the `exe_path` entry, which names where the reference binary
lay when it ran, is shortened to `oracle/_ref/ref_jf` and the header padded with NUL bytes to its old length; nothing else
of the files is touched."""
import functools
import json
import os
import random
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from test_oracle import read_bc
from test_gpu_route import route

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CASES = json.load(open(os.path.join(GOLD, "bloom_nword.json")))["bloom"]
CLI = os.environ.get("JFGPU_CLI") or os.path.join(ROOT, "bin", "jellyfish-amd")


def rows(a):
    return [tuple(r) for r in np.asarray(a).reshape(len(a), -1).tolist()]


def table_map(gpu, t, k):
    kk, cc = gpu.decode_records(t.dump_records(chunk_records=1 << 16), k, t.info.out_counter_len)
    return dict(zip(rows(kk), cc.tolist()))


_HASHES = {}


def hashes(b, k, canonical):
    """(h0, h1) of every k-mer of random_input(k), in order, under the counter's two 64 x 2k matrices, by the oracle's own
    product -- computed once per matrix pair (the counters of a k are seeded alike)."""
    at = (k, canonical, b.matrix1.tobytes(), b.matrix2.tobytes())
    if at not in _HASHES:
        kmers = input_kmers(k, canonical)
        _HASHES[at] = (O.matrix_times(b.matrix1, 64, 2 * k, kmers).tolist(), O.matrix_times(b.matrix2, 64, 2 * k, kmers).tolist())
    return _HASHES[at]


def oracle_check(data, m, nh, h0, h1):
    L = O.lib()
    return np.array([L.jfo_bc_check(data.ctypes.data, m, nh, x, y) for x, y in zip(h0, h1)], dtype=np.uint8)


# ---- 1. the reference's files --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_nword_bloom_bytes_identical_to_reference(gpu, case):
    """The counter fed reads150_dup.fa under the file's own matrices holds the body `jellyfish bc` wrote; a table of
    four-word slots with it attached dumps the reference's `count --bc` dump."""
    header, body = read_bc(os.path.join(GOLD, case["ref_bc"]))
    k, can = case["k"], case["canonical"]
    assert header["key_len"] == 2 * k and len(header["matrix1"]["columns"]) == 2 * k
    m1 = np.array(header["matrix1"]["columns"], dtype=np.uint64)
    m2 = np.array(header["matrix2"]["columns"], dtype=np.uint64)
    seq = O.parse_file(open(os.path.join(GOLD, case["input"]), "rb").read())
    windows = len(O.extract(seq, k, can))
    with gpu.Bloom(k, header["size"], header["nb_hashes"], canonical=can, matrix1=m1, matrix2=m2) as b:
        assert b.nb_bytes == len(body)
        b.insert_ascii(seq)
        assert b.sync() == windows
        assert (b.read() == body).all()
        keys, cnt = O.count(seq, k, can)
        assert keys.shape[1] == (2 * k + 63) // 64
        chk = b.keys(keys)
        assert ((chk == 2) | (cnt < 2)).all() and (chk >= 1).all()
        golden = open(os.path.join(GOLD, case["name"] + ".filtered.dump")).read().splitlines()
        assert len(golden) == case["kept"]
        with gpu.Table(k, 1 << 16, canonical=can) as t:
            t.attach_bloom(b)
            t.count_ascii(seq)
            t.sync()
            got = sorted("%s %d" % (O.to_str(np.array(key, dtype=np.uint64), k), c) for key, c in table_map(gpu, t, k).items())
            assert got == golden
            assert t.stats().mers_fed == windows                  # every window counts as fed, admitted or not
            t.attach_bloom(None)


# ---- 2. random input against the plain-C oracle ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def random_input(k):
    """About 40 000 bases (ten tiles of 4096 positions: windows straddle tiles and the eight-word halo): random ACGT with
    lower-case stretches, an N roughly every 700 bases, one N placed k - 1 bases after another (a run that yields
    nothing), one run of A of length k + 1 (its k-mer twice in a row) and the first 10 000 bases once more."""
    rng = random.Random(1000 + k)
    s = [rng.choice("ACGT") for _ in range(30000)]
    for _ in range(12):
        a = rng.randrange(0, 29000)
        for i in range(a, a + rng.randrange(1, 400)):
            s[i] = s[i].lower()
    at = 0
    while True:
        at += rng.randrange(500, 900)
        if at >= len(s):
            break
        s[at] = "N"
    s[12000] = "N"
    s[12000 + k] = "N"                                          # k - 1 bases between the two
    for i in range(12001, 12000 + k):
        s[i] = rng.choice("ACGT")
    poly = "C" + "A" * (k + 1) + "C"
    seq = ("".join(s[:20000]) + poly + "".join(s[20000:])).encode()
    return seq + seq[:10000]


@functools.lru_cache(maxsize=None)
def input_kmers(k, canonical):
    return np.ascontiguousarray(O.extract(random_input(k), k, canonical))


def disjoint_sample(kmers, h0, h1, m, nh, want):
    """Distinct k-mers no two of which share a cell: what one batch of inserts returns for them does not depend on the
    order the device applies them in."""
    taken, pick, seen = set(), [], set()
    for i in range(0, len(kmers), 101):
        key = tuple(kmers[i].tolist())
        cells = {(h0[i] % m + j * (h1[i] % m)) % m for j in range(nh)}
        if key in seen or cells & taken:
            continue
        seen.add(key); taken |= cells; pick.append(i)
        if len(pick) == want:
            break
    return pick


@pytest.mark.parametrize("tiny", [False, True], ids=["opt_m", "m1009"])
@pytest.mark.parametrize("canonical", [True, False], ids=["C", "fw"])
@pytest.mark.parametrize("k", [65, 96, 97, 128])
def test_nword_bloom_against_oracle_on_random_input(gpu, k, canonical, tiny):
    """Key words 3 | 4 at both ends of each (65, 96 | 97, 128).  m = 1009 with ten hashes: every cell saturates and many
    lanes bump the same word; 1009 is no multiple of 5, so the last byte holds four cells."""
    seq, kmers = random_input(k), input_kmers(k, canonical)
    n = len(kmers)
    assert n > 30000 and kmers.shape[1] == (2 * k + 63) // 64
    m, nh = (1009, 10) if tiny else (gpu.opt_m(0.001, n), gpu.opt_k(0.001))
    L = O.lib()
    with gpu.Bloom(k, m, nh, canonical=canonical, seed=5 + k) as b:
        b.insert_ascii(seq)
        assert b.sync() == n
        got = b.read()
        h0, h1 = hashes(b, k, canonical)
        data = np.zeros(b.nb_bytes, dtype=np.uint8)
        for x, y in zip(h0, h1):
            L.jfo_bc_insert(data.ctypes.data, m, nh, x, y)
        assert (got == data).all()
        assert got.max() <= 242
        poly = O.count(b"A" * k, k, canonical)[0]
        assert b.keys(poly).tolist() == [2]                      # seen twice in a row, and nowhere else
        pick = disjoint_sample(kmers, h0, h1, m, nh, 1 if tiny else 300)
        sample = np.ascontiguousarray(kmers[pick])
        want = oracle_check(data, m, nh, [h0[i] for i in pick], [h1[i] for i in pick])
        assert (b.keys(sample) == want).all()
        if not tiny:
            assert (want == 1).any() and (want == 2).any()
        with gpu.Bloom(k, m, nh, canonical=canonical, matrix1=b.matrix1, matrix2=b.matrix2) as c:
            c.load(got)
            assert (c.read() == got).all()
            assert (c.keys(sample) == want).all()
            assert (c.keys(sample, insert=True) == want).all()    # insert returns the previous minimum
            assert (c.keys(sample) == np.minimum(want + 1, 2)).all()


# ---- 3. count --bc on tables of three- and four-word keys -----------------------------------------------------------------
@pytest.mark.parametrize("k,size", [(65, 1 << 16), (65, 1 << 12), (100, 1 << 16), (128, 1 << 16)], ids=["65", "65-grows", "100", "128"])
def test_count_bc_on_nword_tables(gpu, k, size):
    """The table holds exactly the k-mers whose check() on the counter's bytes is > 1 (jfo_bc_check reads the bytes, not
    the kernels), each with its true multiplicity; the input goes in in two calls that overlap by k - 1 bases.  A size
    hint of 2^12 slots: the table doubles with the filter attached, and the larger table goes on asking it."""
    seq, kmers = random_input(k), input_kmers(k, True)
    m, nh = gpu.opt_m(0.001, len(kmers)), gpu.opt_k(0.001)
    uniq, first_at, cnt = np.unique(kmers, axis=0, return_index=True, return_counts=True)
    with gpu.Bloom(k, m, nh, canonical=True, seed=5 + k) as b:
        b.insert_ascii(seq)
        b.sync()
        data = b.read()
        h0, h1 = hashes(b, k, True)
        adm = oracle_check(data, m, nh, [h0[i] for i in first_at.tolist()], [h1[i] for i in first_at.tolist()]) > 1
        exp = {key: c for key, c, a in zip(rows(uniq), cnt.tolist(), adm.tolist()) if a}
        assert 5000 < len(exp) < len(uniq) and all(key in exp for key, c in zip(rows(uniq), cnt.tolist()) if c >= 2)
        with gpu.Table(k, size, canonical=True) as t:
            first = int(t.info.lsize)
            t.attach_bloom(b)
            cut = 17001
            t.count_ascii(seq[:cut])
            t.count_ascii(seq[cut - (k - 1):])
            t.sync()
            assert table_map(gpu, t, k) == exp
            assert t.stats().mers_fed == len(kmers)
            if size == 1 << 12:
                assert int(t.refresh_info().lsize) > first == 12
            t.attach_bloom(None)
            t.count_ascii(seq[:cut])                              # detached: everything is counted again
            t.sync()
            assert len(table_map(gpu, t, k)) > len(exp)


# ---- 4. count --bf-size ----------------------------------------------------------------------------------------------------
def test_one_pass_bloom_filter_on_nword_keys(gpu):
    """tests/test_gpu_bloom.py::test_one_pass_bloom_filter at k = 100: the first sighting of a k-mer only marks it, later
    ones are counted.  The repeated part is fed with a once-only part and then again alone, so every repeated k-mer is
    counted once per sighting of the second feed, plus those of the first feed that were false positives; k-mers seen once
    are absent but for false positives.  The caps are that test's: three times the filter's nominal rate of 0.01.  (A
    simulation of the filter at these sizes -- 44 802 k-mers, 448 020 bits, seven hashes -- gives 3 to 7 false positives
    among the 29 901 repeated k-mers and 49 to 57 among the 14 901 others: caps 897 and 447.)"""
    k = 100
    rng = random.Random(k * 7)
    twice = "".join(rng.choice("ACGT") for _ in range(30000)).encode()
    once = "".join(rng.choice("ACGT") for _ in range(15000)).encode()
    rep = set(rows(O.count(twice, k, True)[0]))
    single = set(rows(O.count(once, k, True)[0])) - rep
    n = len(rep) + len(single)
    with gpu.Bloom(k, gpu.opt_m(0.01, n), gpu.opt_k(0.01), canonical=True, one_pass_filter=True) as bf, \
            gpu.Table(k, 1 << 17, canonical=True) as t:
        assert bf.nb_bytes == (gpu.opt_m(0.01, n) + 7) // 8 and bf.nb_hashes == 7
        t.attach_bloom(bf)
        t.count_ascii(twice + b"N" + once)
        t.sync()
        t.count_ascii(twice)
        t.sync()
        got = table_map(gpu, t, k)
        t.attach_bloom(None)
    mult = {}
    kt_all = rows(O.extract(twice, k, True))
    for key in kt_all:
        mult[key] = mult.get(key, 0) + 1
    assert all(mult[key] <= got.get(key, 0) <= 2 * mult[key] for key in rep)
    extra = sum(got[key] - mult[key] for key in rep)
    fp_single = sum(1 for key in single if key in got)
    assert extra <= 0.03 * len(kt_all) and fp_single <= 0.03 * len(single)
    assert set(got) <= rep | single


# ---- 5. refusals that stay -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [65, 100])
def test_routing_refuses_an_nword_table_with_a_filter(gpu, k):
    """The routing kernels of keys of three and four words take no filter: a table with a counter attached is refused
    (with the mer length in the message) instead of being routed unfiltered; without the filter the same call routes."""
    seq = random_input(k)[:6000]
    with gpu.Bloom(k, gpu.opt_m(0.01, 6000), gpu.opt_k(0.01), canonical=True, seed=3) as b, \
            gpu.Table(k, 1 << 16, canonical=True, shard_bits=1, shard_id=0) as t:
        t.attach_bloom(b)
        try:
            with pytest.raises(gpu.JfgpuError) as e:
                route(t, seq, 0)
            assert e.value.code == gpu.E_UNSUPPORTED and ("mer length %d" % k) in e.value.msg
        finally:
            t.attach_bloom(None)
        counts, _ = route(t, seq, 0)
        assert int(counts.sum()) == len(O.extract(seq, k, True))


def test_mer_length_129_is_refused(gpu):
    for one_pass in (False, True):
        with pytest.raises(gpu.JfgpuError) as e:
            gpu.Bloom(129, 1000, 3, one_pass_filter=one_pass)
        assert e.value.code == gpu.E_UNSUPPORTED and "128" in e.value.msg


# ---- 6. the command line ---------------------------------------------------------------------------------------------------
def dump_lines(path):
    return sorted(subprocess.check_output([CLI, "dump", "-c", path]).decode().splitlines())


def test_cli_bc_and_count_bc_at_k100(gpu, tmp_path):
    """`bc -m 100 -C` writes the reference's file (size, nb_hashes, both 64 x 200 matrices, body); `count --bc` on the
    reference's file gives the reference's dump; `query` reads the engine's file; the reference loads it."""
    case = [c for c in CASES if c["k"] == 100][0]
    inp = os.path.join(GOLD, case["input"])
    ref_bc = os.path.join(GOLD, case["ref_bc"])
    golden = open(os.path.join(GOLD, case["name"] + ".filtered.dump")).read().splitlines()
    mine = str(tmp_path / "mine.bc")
    subprocess.check_call([CLI, "bc", "-m", "100", "-C", "-s", "9000", "-f", "0.001", "-o", mine, inp])
    h_ref, body_ref = read_bc(ref_bc)
    h, body = read_bc(mine)
    assert h["format"] == "bloomcounter" and h["key_len"] == 200 and h["canonical"] is True
    assert (h["size"], h["nb_hashes"]) == (h_ref["size"], h_ref["nb_hashes"])
    for mx in ("matrix1", "matrix2"):
        assert h[mx]["r"] == 64 and h[mx]["c"] == 200 and len(h[mx]["columns"]) == 200
        assert h[mx]["columns"] == h_ref[mx]["columns"]
    assert len(body) == len(body_ref) and (body == body_ref).all()
    out = str(tmp_path / "f.jf")
    subprocess.check_call([CLI, "count", "-m", "100", "-C", "-s", "64k", "--bc", ref_bc, "-o", out, inp])
    assert dump_lines(out) == golden
    picks = [l.split()[0] for l in golden[::200]]
    ans = subprocess.check_output([CLI, "query", mine] + picks).decode().splitlines()
    assert ans == ["%s 2" % p for p in picks]
    if O.have_ref():
        out2 = str(tmp_path / "f2.jf")
        subprocess.check_call([O.REF_JF, "count", "-m", "100", "-C", "-s", "64k", "--bc", mine, "-o", out2, inp])
        assert sorted(subprocess.check_output([O.REF_JF, "dump", "-c", out2]).decode().splitlines()) == golden


def test_cli_count_bf_size_at_k65(gpu, tmp_path):
    """`count -m 65 --bf-size 10k` over two files, the second one a repeat of half of the first (a file is fed after the
    one before it): what was seen once is dropped, up to the caps of the one-pass test above."""
    k = 65
    rng = random.Random(65)
    reads = ["".join(rng.choice("ACGT") for _ in range(150)) for _ in range(60)]
    a, b = tmp_path / "a.fa", tmp_path / "b.fa"
    a.write_text("".join(">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)))
    b.write_text("".join(">s%d\n%s\n" % (i, r) for i, r in enumerate(reads[:30])))
    out = str(tmp_path / "f.jf")
    subprocess.check_call([CLI, "count", "-m", str(k), "-s", "64k", "--bf-size", "10k", "-o", out, str(a), str(b)])
    got = dict((l.split()[0], int(l.split()[1])) for l in dump_lines(out))
    rep = {O.to_str(np.array(key, dtype=np.uint64), k) for key in rows(O.count("N".join(reads[:30]).encode(), k, False)[0])}
    single = {O.to_str(np.array(key, dtype=np.uint64), k) for key in rows(O.count("N".join(reads[30:]).encode(), k, False)[0])} - rep
    assert len(rep) == 30 * 86 and len(single) == 30 * 86
    assert all(1 <= got.get(key, 0) <= 2 for key in rep)
    assert sum(got[key] - 1 for key in rep) <= 0.03 * len(rep)
    assert sum(1 for key in single if key in got) <= 0.03 * len(single)
    assert set(got) <= rep | single


def test_cli_bc_gpus_is_refused_by_mer_length(gpu, tmp_path):
    r = subprocess.run([CLI, "bc", "-m", "100", "-s", "9000", "-o", str(tmp_path / "o.bc"), "--gpus", "2",
                        os.path.join(GOLD, "reads150_dup.fa")], capture_output=True, timeout=300)
    assert r.returncode != 0 and b"mer length 100" in r.stderr, r.stderr
