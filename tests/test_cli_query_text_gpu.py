"""`jellyfish-amd query -s` with its lines built on the device (-m gpu): a binary/sorted database is looked up and formatted
by jfgpu_query_text, a bloomcounter database is loaded into a device counter and answered by jfgpu_bc_query_text
(sub_commands/query_main.cc:44-51, :99-104).  The output is the host path's byte for byte -- under the default, with
JFGPU_QUERY_FORMAT_HOST=1 (device look-up, host lines) and with JFGPU_QUERY_HOST=1 (everything on the host), to stdout and
to -o FILE -- and JFGPU_QUERY_TRACE says which database kind was answered and who built the lines."""
import os
import random
import subprocess

import pytest

from test_cli_query_gpu import CLI, ROOT, make_db, make_query

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def cli(gpu):
    if not os.environ.get("JFGPU_CLI"):
        subprocess.check_call(["make", "-s", "cli"], cwd=ROOT)
    return CLI


def run_query(cli, db, q, out_file=None, **env):
    cmd = [cli, "query", db, "-s", q] + (["-o", out_file] if out_file else [])
    r = subprocess.run(cmd, env=dict(os.environ, JFGPU_QUERY_TRACE="1", **env), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    trace = [l for l in r.stderr.decode().splitlines() if l.startswith("query: ")]
    assert len(trace) == 1, r.stderr.decode()
    if out_file:
        assert r.stdout == b""
        return open(out_file, "rb").read(), trace[0]
    return r.stdout, trace[0]


def three_ways(cli, tmp_path, db, q, k, kind, mers):
    """The output under the default, JFGPU_QUERY_FORMAT_HOST=1 and JFGPU_QUERY_HOST=1, to stdout and to a file: one text."""
    host, host_trace = run_query(cli, db, q, JFGPU_QUERY_HOST="1")
    assert host_trace == "query: host" and len(host.splitlines()) == mers
    for env, fmt in (({}, "device"), ({"JFGPU_QUERY_FORMAT_HOST": "1"}, "host")):
        for out_file in (None, str(tmp_path / ("out_%s.txt" % fmt))):
            got, trace = run_query(cli, db, q, out_file, **env)
            assert got == host, (fmt, out_file)
            assert trace.startswith("query: device k=%d positions=" % k) and trace.endswith(" mers=%d" % mers), trace
            fields = dict(f.split("=") for f in trace.split()[2:])
            assert fields["db"] == kind and fields["format"] == fmt, trace
            assert all(float(fields[name]) >= 0 for name in ("upload_ms", "kernels_ms", "download_ms", "sink_ms")), trace
            if fmt == "device":
                assert float(fields["kernels_ms"]) > 0, trace
    return host


@pytest.mark.parametrize("k,flags", [(21, ["-C"]), (40, ["-C"]), (100, ["-C"]), (100, [])], ids=["21C", "40C", "100C", "100"])
def test_binary_database(cli, tmp_path, k, flags):
    rng = random.Random(13 * k + len(flags))
    genome, db = make_db(cli, tmp_path, k, flags, rng)
    q, runs = make_query(tmp_path, genome, rng)
    mers = sum(n - k + 1 for n in runs)
    text = three_ways(cli, tmp_path, db, q, k, "binary", mers)
    found = sum(1 for l in text.decode().splitlines() if l.split()[1] != "0")
    assert found >= mers // 3 and mers - found >= mers // 10
    # small pieces: the lines of every piece once, in order
    got, trace = run_query(cli, db, q, JFGPU_QUERY_PIECE="700")
    assert got == text and "format=device" in trace


def bloom_query_input(tmp_path, reads, rng):
    """The reads themselves (inserted, some of them twice), one of them on the other strand, and sequence never inserted."""
    seqs = ["".join(r.splitlines()[1:]) for r in open(reads).read().split(">")[1:]]
    q = tmp_path / "bq.fa"
    with open(q, "w") as f:
        for i, s in enumerate(seqs):
            f.write(">r%d\n%s\n" % (i, s))
        f.write(">other_strand\n%s\n" % seqs[3].translate(str.maketrans("ACGTacgt", "TGCAtgca"))[::-1])
        f.write(">with_N_and_lower\n%sN%s\n" % (seqs[5][:70].lower(), seqs[5][70:]))
        f.write(">novel\n%s\n" % "".join(rng.choice("ACGT") for _ in range(1500)))
    return str(q)


def check_bloom(cli, tmp_path, bc, q, k):
    host, _ = run_query(cli, bc, q, JFGPU_QUERY_HOST="1")
    mers = len(host.splitlines())
    assert mers > 1000
    text = three_ways(cli, tmp_path, bc, q, k, "bloomcounter", mers)
    assert {l.split()[1] for l in text.decode().splitlines()} == {"0", "1", "2"}


@pytest.mark.parametrize("k,flags", [(21, ["-C"]), (31, []), (100, ["-C"])], ids=["21C", "31", "100C"])
def test_bloomcounter_written_by_bc(cli, tmp_path, k, flags):
    rng = random.Random(17 * k)
    reads = os.path.join(GOLD, "reads150_dup.fa")
    bc = str(tmp_path / "db.bc")
    subprocess.check_call([cli, "bc", "-m", str(k), "-s", "9000", "-f", "0.001", "-o", bc] + flags + [reads])
    check_bloom(cli, tmp_path, bc, bloom_query_input(tmp_path, reads, rng), k)


@pytest.mark.parametrize("name,k", [("bc_k21C", 21), ("bc_k31", 31), ("bc_k65", 65), ("bc_k100C", 100)])
def test_bloomcounter_written_by_the_reference(cli, tmp_path, name, k):
    rng = random.Random(19 * k)
    reads = os.path.join(GOLD, "reads150_dup.fa")
    check_bloom(cli, tmp_path, os.path.join(GOLD, name + ".ref.bc"), bloom_query_input(tmp_path, reads, rng), k)


def test_truncated_bloomcounter_goes_to_the_host_path(cli, tmp_path):
    """A body one byte short of ceil(m / 5) is never loaded into a device counter: the host path takes the file, and says what
    it says with JFGPU_QUERY_HOST=1 -- that the file is truncated."""
    raw = open(os.path.join(GOLD, "bc_k21C.ref.bc"), "rb").read()
    cut = str(tmp_path / "cut.bc")
    with open(cut, "wb") as f:
        f.write(raw[:-1])
    q = bloom_query_input(tmp_path, os.path.join(GOLD, "reads150_dup.fa"), random.Random(1))
    answers = []
    for env in ({}, {"JFGPU_QUERY_HOST": "1"}):
        r = subprocess.run([cli, "query", cut, "-s", q], env=dict(os.environ, JFGPU_QUERY_TRACE="1", **env), capture_output=True)
        answers.append((r.returncode, r.stdout, r.stderr))
        assert "query: device" not in r.stderr.decode()
    assert answers[0] == answers[1] and answers[0][0] != 0 and b"truncated" in answers[0][2]
    # and one byte too many: the host path again, which answers from the bytes that count
    longer = str(tmp_path / "longer.bc")
    with open(longer, "wb") as f:
        f.write(raw + b"\0")
    got, trace = run_query(cli, longer, q)
    want, _ = run_query(cli, os.path.join(GOLD, "bc_k21C.ref.bc"), q, JFGPU_QUERY_HOST="1")
    assert trace == "query: host" and got == want
