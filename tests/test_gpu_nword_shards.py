"""Hash-prefix shards of tables of keys of three and four words, 65 <= k <= 128 (-m gpu).

Every rank routes the 256-bit k-mers of its input by owner (route_count / route_scatter_kernel<NTable>), a message carries
ceil(2k / 64) words per k-mer (3 for k <= 96, 4 above), receivers insert with the four-word claim (add_keys_kernel<NTable>)
or, in the UPDATE pass of `count --if`, count what is present (update_keys_kernel<NTable, true>).  Shards grow together
(reshard_kernel<NTable>, add_pairs_kernel<NTable>), and a step is cut into pieces whose send buffers stay under a byte budget
(JFGPU_COMM_PIECE_BYTES).  What the shards hold is what one table holds."""
import hashlib
import json
import os
import random
import subprocess

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CLI = os.environ.get("JFGPU_CLI") or os.path.join(ROOT, "bin", "jellyfish-amd")


def rnd_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n)).encode()


def oracle_map(seq, k, canonical):
    keys, cnt = O.count(seq, k, canonical)
    return {tuple(r): c for r, c in zip(keys.tolist(), cnt.tolist())}


def table_map(capi, t):
    keys, cnts = capi.decode_records(t.dump_records(chunk_records=1 << 16), t.k, t.info.out_counter_len)
    keys = np.asarray(keys).reshape(len(cnts), -1)
    assert len({tuple(r) for r in keys.tolist()}) == len(keys)
    return {tuple(r): c for r, c in zip(keys.tolist(), cnts.tolist())}


def feed_local(comm, shards, steps, bufs):
    for step in steps:
        ptrs, ns = [], []
        for r, seq in enumerate(step):
            d = shards[r].malloc(len(seq) + 64)
            if seq:
                shards[r].h2d(d, np.frombuffer(seq, dtype=np.uint8))
            bufs.append((shards[r], d)); ptrs.append(d); ns.append(len(seq))
        comm.local_step(shards, ptrs, ns)


def test_the_parent_refusal_is_gone(gpu):
    """A shard of a table of 100-mers can be created (the engine used to answer `jfgpu error 6: sharded tables with mer
    length > 64 are not built yet`); it holds at least one tile of 2^11 slots and its slot array is four words a slot."""
    with gpu.Table(100, 1 << 16, shard_bits=1, shard_id=0) as t:
        assert t.info.slot_bytes == 32 and t.info.shard_bits == 1 and t.info.lsize == 16
    with gpu.Table(100, 1 << 4, shard_bits=3, shard_id=5) as t:
        assert t.info.lsize >= 11 + 3


# (k, canonical, world, JFGPU_COMM_MAX_MSG, JFGPU_COMM_PIECE_BYTES)
CASES = [(k, can, w, None, None) for (k, can) in ((65, True), (96, False), (100, True), (120, False)) for w in (1, 2, 4, 8)]
CASES += [(100, True, 4, "997", None), (65, True, 2, None, "24000"), (100, True, 4, None, "30000")]


@pytest.mark.parametrize("k,canonical,world,max_msg,piece", CASES)
def test_sharded_nword_keys_equal_single_table(gpu, monkeypatch, k, canonical, world, max_msg, piece):
    """The shards' dumps concatenated in rank order are byte-identical to the dump of one table of the same lsize under the
    same matrix; sent == received == every k-mer of the input; stats sum to the oracle's; a key added to a shard that does
    not own it is refused by every shard but its owner.  JFGPU_COMM_MAX_MSG=997: messages go in rounds.
    JFGPU_COMM_PIECE_BYTES small: every step with input is cut into several pieces (more routing passes than steps)."""
    if max_msg:
        monkeypatch.setenv("JFGPU_COMM_MAX_MSG", max_msg)
    if piece:
        monkeypatch.setenv("JFGPU_COMM_PIECE_BYTES", piece)
    rng = random.Random(k * 13 + world * 3 + (7 if piece else 0) + (5 if max_msg else 0))
    L = 48000 // world
    steps = [[rnd_seq(rng, rng.choice([0, 70, L // 2, L]), "ACGTN") for _ in range(world)] for _step in range(3)]
    steps[1][0] = b""                                           # an empty rank
    steps[0][world - 1] = steps[0][world - 1] + b"N" + rnd_seq(rng, 30000, "ACGT")      # one rank with 30 kb more
    whole_seq = b"N".join(b"N".join(step) for step in steps)
    keys, cnt = O.count(whole_seq, k, canonical)
    assert len(keys) > 1000
    with gpu.Table(k, 1 << 18, canonical=canonical) as single:
        single.set_growth(False)
        single.count_ascii(whole_seq); single.sync()
        whole = single.dump_records()
        cols = single.matrix()
        lsize_g = single.info.lsize
    assert lsize_g == 18 and (1 << lsize_g) <= (1 << 20)
    sb = world.bit_length() - 1
    shards = [gpu.Table(k, 1 << lsize_g, canonical=canonical, shard_bits=sb, shard_id=r, matrix_columns=cols) for r in range(world)]
    comm = gpu.Comm(world, local=True)
    try:
        assert all(t.info.lsize == lsize_g and t.info.slot_bytes == 32 for t in shards)
        for t in shards:
            t.profile_enable(True)
        bufs = []
        feed_local(comm, shards, steps, bufs)
        sent, received = comm.finish()
        assert sent == received == int(cnt.sum())
        routes = [shards[r].profile_get(2)[1] // 2 for r in range(world)]          # (two routing passes per piece)
        with_input = [sum(1 for step in steps if len(step[r]) >= k) for r in range(world)]
        assert all(p >= s for p, s in zip(routes, with_input)), (routes, with_input)
        if piece:                                               # pieces of at most P bytes that overlap by k - 1
            P = int(piece) // (8 * ((2 * k + 63) // 64))
            least = [sum(-(-(len(step[r]) - (k - 1)) // (P - (k - 1))) for step in steps if len(step[r]) >= k) for r in range(world)]
            assert all(p >= m for p, m in zip(routes, least)) and max(routes) > 3 * max(with_input), (routes, least)
        for t in shards:
            t.sync()
        parts = [t.dump_records() for t in shards]
        assert (np.concatenate(parts) == whole).all()
        assert sum(t.stats().total for t in shards) == int(cnt.sum())
        assert sum(t.stats().distinct for t in shards) == len(keys)
        foreign = np.ascontiguousarray(keys[:1], dtype=np.uint64)
        refused = 0
        for t in shards:
            try:
                t.add_keys(foreign)
                t.sync()
            except gpu.JfgpuError as e:
                assert "does not own" in e.msg
                refused += 1
        assert refused == world - 1
        for t, d in bufs:
            t.free(d)
    finally:
        comm.close()
        for t in shards:
            t.close()


@pytest.mark.parametrize("k,world", [(100, 2), (65, 2), (65, 4), (100, 4)])
def test_nword_shards_grow_together(gpu, k, world):
    """Shards created at the minimum size double together (comm_grow: reshard_kernel<NTable>, pairs of kw key words and a
    count through the key path's exchange, add_pairs_kernel<NTable>): every shard ends at the same lsize, at least two
    doublings above where it started, under one matrix; every key sits on the shard its position names; no key is on two
    shards; the union is the oracle's map."""
    rng = random.Random(k * 11 + world)
    steps = [[rnd_seq(rng, rng.choice([20000, 50000, 80000]), "ACGT") + b"N" + rnd_seq(rng, 300, "ACGTN") for _ in range(world)] for _step in range(4)]
    whole_seq = b"N".join(b"N".join(step) for step in steps)
    keys, cnt = O.count(whole_seq, k, True)
    exp = oracle_map(whole_seq, k, True)
    sb = world.bit_length() - 1
    shards = [gpu.Table(k, 1, shard_bits=sb, shard_id=r) for r in range(world)]
    comm = gpu.Comm(world, local=True)
    try:
        lsize0 = shards[0].info.lsize
        bufs = []
        feed_local(comm, shards, steps, bufs)
        sent, received = comm.finish()
        assert sent == received == int(cnt.sum())
        got = {}
        for r, t in enumerate(shards):
            t.sync()
            assert t.info.lsize >= lsize0 + 2 and t.info.lsize == shards[0].info.lsize, "the shards must have doubled, and together"
            part = table_map(gpu, t)
            sub = np.array(list(part.keys()), dtype=np.uint64).reshape(-1, (2 * k + 63) // 64)
            if sb and len(sub):
                pos = O.matrix_times(t.matrix(), t.info.lsize, 2 * k, sub)
                assert ((pos >> np.uint64(t.info.lsize - sb)) == r).all()
            assert not (set(part) & set(got))
            got.update(part)
        assert got == exp
        assert len({tuple(t.matrix().tolist()) for t in shards}) == 1
        assert sum(t.stats().total for t in shards) == int(cnt.sum())
        for t, d in bufs:
            t.free(d)
    finally:
        comm.close()
        for t in shards:
            t.close()


def test_prime_and_update_over_nword_shards(gpu):
    """The two passes of `count --if` over shards of 100-mers: PRIME with one sequence set (count 0), UPDATE with reads that
    overlap it in part (counted only if present, update_keys_kernel<NTable, true>).  The result equals one table run through the
    same two operations, keys primed with count 0 included, and the oracle."""
    rng = random.Random(100)
    k, world = 100, 2
    wanted = [rnd_seq(rng, 6000) for _ in range(world)]
    reads = [wanted[r][1000:4000] + b"N" + rnd_seq(rng, 5000) + b"N" + wanted[(r + 1) % world][500:2500] for r in range(world)]
    exp_w = oracle_map(b"N".join(wanted), k, True)
    exp_r = oracle_map(b"N".join(reads), k, True)
    exp = {key: exp_r.get(key, 0) for key in exp_w}
    with gpu.Table(k, 1 << 16) as single:
        single.set_operation(1); single.count_ascii(b"N".join(wanted)); single.sync()
        single.set_operation(2); single.count_ascii(b"N".join(reads)); single.sync()
        one = table_map(gpu, single)
        cols = single.matrix()
        lsize_g = single.info.lsize
    assert one == exp and sum(exp.values()) > 1000 and any(v == 0 for v in exp.values())
    shards = [gpu.Table(k, 1 << lsize_g, shard_bits=1, shard_id=r, matrix_columns=cols) for r in range(world)]
    comm = gpu.Comm(world, local=True)
    try:
        bufs = []
        for t in shards:
            t.set_operation(1)
        feed_local(comm, shards, [wanted], bufs)
        comm.finish()
        for t in shards:
            t.sync()
        assert sum(t.stats().distinct for t in shards) == len(exp_w) and sum(t.stats().total for t in shards) == 0
        for t in shards:
            t.set_operation(2)
        feed_local(comm, shards, [reads], bufs)
        comm.finish()
        got = {}
        for t in shards:
            t.sync()
            part = table_map(gpu, t)
            assert not (set(part) & set(got))
            got.update(part)
        assert got == one
        for t, d in bufs:
            t.free(d)
    finally:
        comm.close()
        for t in shards:
            t.close()


# ---- the command line: rank processes on one device (ipc transport) ---------------------------------------------------

@pytest.fixture(scope="module")
def cli(gpu):
    if not os.environ.get("JFGPU_CLI"):
        subprocess.check_call(["make", "-s", "cli"], cwd=ROOT)
    return CLI


def _body(path):
    d = open(path, "rb").read()
    return d[9 + int(d[:9]):]


def _ipc_env(**extra):
    env = dict(os.environ, JFGPU_COMM_TRANSPORT="ipc", JFGPU_PARSE_CHUNK="150000",
               HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    env.pop("JFGPU_COMM_PIECE_BYTES", None)
    env.update(extra)
    return env


def _reads(path, rng, n, length=150):
    with open(path, "wb") as f:
        for r in range(n):
            f.write((">r%d\n%s\n" % (r, "".join(rng.choice("ACGT") for _ in range(length)))).encode())


@pytest.mark.parametrize("k,world", [(100, 2), (100, 4), (65, 2)])
def test_count_gpus_n_nword_as_rank_processes(cli, tmp_path, k, world):
    """`count -m 100 -C --gpus 2 / 4` and `-m 65 --gpus 2` (three-word keys) on 6000 random 150 bp reads as rank processes
    on one device: file body, --digest and stats equal the single-process run's."""
    rng = random.Random(31 + k + world)
    fa = tmp_path / "reads.fa"
    _reads(fa, rng, 6000)
    ref, out = str(tmp_path / "ref.jf"), str(tmp_path / "gN.jf")
    dg0, dg1 = str(tmp_path / "d0.txt"), str(tmp_path / "d1.txt")
    subprocess.check_call([cli, "count", "-m", str(k), "-C", "-s", "2M", "-o", ref, "--digest", dg0, str(fa)])
    subprocess.check_call([cli, "count", "-m", str(k), "-C", "-s", "2M", "-o", out, "--digest", dg1, "--gpus", str(world), str(fa)], env=_ipc_env(), timeout=900)
    assert open(dg0).read() == open(dg1).read()
    assert _body(out) == _body(ref) and len(_body(ref)) > 0
    assert subprocess.check_output([cli, "stats", out]) == subprocess.check_output([cli, "stats", ref])


def test_count_gpus_2_nword_grows_from_a_tiny_size_hint(cli, tmp_path):
    """`-s 2k --gpus 2 -m 100`: the shards grow together; `dump -c` equals the single-process run's, and the reference's
    reader finds the file in order."""
    rng = random.Random(77)
    fa = tmp_path / "reads.fa"
    _reads(fa, rng, 3000)
    ref, out = str(tmp_path / "ref.jf"), str(tmp_path / "g2.jf")
    subprocess.check_call([cli, "count", "-m", "100", "-C", "-s", "2k", "-o", ref, str(fa)])
    subprocess.check_call([cli, "count", "-m", "100", "-C", "-s", "2k", "-o", out, "--gpus", "2", str(fa)], env=_ipc_env(JFGPU_PARSE_CHUNK="100000"), timeout=900)
    want = sorted(subprocess.check_output([cli, "dump", "-c", ref]).decode().splitlines())
    got = subprocess.check_output([cli, "dump", "-c", out]).decode().splitlines()
    assert sorted(got) == want and len(want) > 100000
    assert subprocess.check_output([cli, "stats", out]) == subprocess.check_output([cli, "stats", ref])
    if O.have_ref():
        assert subprocess.check_output([O.REF_JF, "dump", "--check-order", out]).decode().startswith("ORDER OK %d" % len(want))


def test_large_key_golden_k100_over_two_shards(cli, tmp_path):
    """tests/large_key.sh under --gpus 2: the first 10001 lines of the reference generator's seq1m_0.fa, -m 100 with -s 2M
    and -s 2k (the shards grow); the sorted k-mer list has the reference's golden md5."""
    if not os.access(O.REF_GEN, os.X_OK):
        pytest.skip("oracle/_ref not built")
    g = json.load(open(os.path.join(GOLD, "manifest.json")))["reference_md5"]
    d = str(tmp_path)
    subprocess.check_call([O.REF_GEN, "-o", "seq1m"] + g["seq1m"], cwd=d)
    with open(os.path.join(d, "head.fa"), "wb") as f:
        f.write(b"".join(open(os.path.join(d, "seq1m_0.fa"), "rb").readlines()[:10001]))
    for name, size in (("m100_2M.jf", "2M"), ("m100_2k.jf", "2k")):
        subprocess.check_call([cli, "count", "-t", "4", "-o", name, "-m", "100", "-s", size, "--gpus", "2", "head.fa"], cwd=d, env=_ipc_env(), timeout=900)
        out = subprocess.check_output([cli, "dump", "-c", name], cwd=d)
        md5 = hashlib.md5(b"".join(sorted(l.split(b" ")[0] + b"\n" for l in out.splitlines()))).hexdigest()
        assert md5 == g["large_key_m100.ordered"], name


def test_count_gpus_2_nword_if_and_text(cli, tmp_path):
    """`--if` and `--text` at k = 100 with --gpus 2 equal their single-process files."""
    rng = random.Random(5)
    fa, iff = tmp_path / "reads.fa", tmp_path / "if.fa"
    _reads(fa, rng, 3000)
    lines = open(fa).read().splitlines()
    with open(iff, "w") as f:
        for i in range(0, 2000, 2):                              # half the reads as the --if set, and some that are not in the reads
            f.write(lines[i] + "\n" + lines[i + 1] + "\n")
        f.write(">x\n" + "".join(rng.choice("ACGT") for _ in range(5000)) + "\n")
    for extra, tag in ((["--if", str(iff)], "if"), (["--text"], "txt")):
        ref, out = str(tmp_path / (tag + "_ref.jf")), str(tmp_path / (tag + "_g2.jf"))
        subprocess.check_call([cli, "count", "-m", "100", "-C", "-s", "1M", "-o", ref] + extra + [str(fa)])
        subprocess.check_call([cli, "count", "-m", "100", "-C", "-s", "1M", "-o", out, "--gpus", "2"] + extra + [str(fa)], env=_ipc_env(JFGPU_PARSE_CHUNK="100000"), timeout=900)
        if tag == "if":
            want = sorted(subprocess.check_output([cli, "dump", "-c", ref]).decode().splitlines())
            got = sorted(subprocess.check_output([cli, "dump", "-c", out]).decode().splitlines())
            assert got == want and any(l.endswith(" 0") for l in want) and any(not l.endswith(" 0") for l in want)
            assert _body(out) == _body(ref)
        else:
            assert _body(out) == _body(ref) and len(_body(ref)) > 100000


@pytest.mark.parametrize("feed", ["-g", "--host-parse", "--sam"])
def test_count_gpus_2_nword_other_feeds(cli, tmp_path, feed):
    """`-g` (generator commands), `--host-parse` and `--sam` (a BGZF BAM) at k = 100 with --gpus 2 equal their
    single-process files."""
    import sam_fixtures as S
    rng = random.Random(21)
    fa = tmp_path / "reads.fa"
    _reads(fa, rng, 3000)
    if feed == "-g":
        gen = tmp_path / "gen.txt"
        gen.write_text("cat %s\ncat %s\n" % (fa, fa))
        args = ["-g", str(gen)]
    elif feed == "--sam":
        bam = tmp_path / "reads.bam"
        bam.write_bytes(S.bgzf(S.bam_stream(S.random_records(3000, 21))))
        args = ["--sam", str(bam)]
    else:
        args = ["--host-parse", str(fa)]
    ref, out = str(tmp_path / "ref.jf"), str(tmp_path / "g2.jf")
    subprocess.check_call([cli, "count", "-m", "100", "-C", "-s", "1M", "-o", ref] + args)
    subprocess.check_call([cli, "count", "-m", "100", "-C", "-s", "1M", "-o", out, "--gpus", "2"] + args, env=_ipc_env(JFGPU_PARSE_CHUNK="100000"), timeout=900)
    assert _body(out) == _body(ref) and len(_body(ref)) > 100000


def test_count_gpus_2_nword_default_parse_chunk_goes_in_pieces(cli, tmp_path):
    """Without JFGPU_PARSE_CHUNK the parser hands over its default chunk; a file of a few MB larger than one piece (budget
    override small) goes through in pieces and equals the single-process file."""
    rng = random.Random(9)
    fa = tmp_path / "reads.fa"
    _reads(fa, rng, 20000)
    assert os.path.getsize(fa) > 3_000_000
    ref, out = str(tmp_path / "ref.jf"), str(tmp_path / "g2.jf")
    subprocess.check_call([cli, "count", "-m", "100", "-C", "-s", "8M", "-o", ref, str(fa)])
    env = _ipc_env(JFGPU_COMM_PIECE_BYTES=str(1 << 24))           # 16 MiB send buffers: pieces of 512 KiB of input
    env.pop("JFGPU_PARSE_CHUNK", None)
    subprocess.check_call([cli, "count", "-m", "100", "-C", "-s", "8M", "-o", out, "--gpus", "2", str(fa)], env=env, timeout=900)
    assert _body(out) == _body(ref) and len(_body(ref)) > 0


def test_count_gpus_1_nword_through_rccl_to_itself(cli, tmp_path):
    """`count --gpus 1 -m 100` with JFGPU_COMM_SELF_RCCL=1 (ncclSend / ncclRecv to itself) equals the plain run."""
    rng = random.Random(12)
    fa = tmp_path / "reads.fa"
    _reads(fa, rng, 4000)
    ref, out = str(tmp_path / "ref.jf"), str(tmp_path / "g1.jf")
    dg0, dg1 = str(tmp_path / "d0.txt"), str(tmp_path / "d1.txt")
    subprocess.check_call([cli, "count", "-m", "100", "-C", "-s", "2M", "-o", ref, "--digest", dg0, str(fa)])
    env = dict(os.environ, JFGPU_COMM_SELF_RCCL="1", JFGPU_PARSE_CHUNK="200000")
    env.pop("JFGPU_COMM_TRANSPORT", None)
    subprocess.check_call([cli, "count", "-m", "100", "-C", "-s", "2M", "-o", out, "--digest", dg1, "--gpus", "1", str(fa)], env=env, timeout=600)
    assert open(dg0).read() == open(dg1).read()
    assert _body(out) == _body(ref)


@pytest.mark.parametrize("flag", [["--bc", "x.bc"], ["--bf-size", "1M"]])
def test_count_gpus_nword_bloom_options_are_refused_by_mer_length(cli, tmp_path, flag):
    """--bc and --bf-size with -m 100 --gpus 2: there is no four-word Bloom counter; the message names the mer length."""
    fa = tmp_path / "reads.fa"
    _reads(fa, random.Random(1), 10)
    r = subprocess.run([cli, "count", "-m", "100", "-s", "1M", "-o", str(tmp_path / "o.jf"), "--gpus", "2"] + flag + [str(fa)],
                       capture_output=True, env=_ipc_env(), timeout=300)
    assert r.returncode != 0 and b"mer length 100" in r.stderr, r.stderr
