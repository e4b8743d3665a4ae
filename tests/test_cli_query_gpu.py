"""`jellyfish-amd query -s` on the GPU (-m gpu): the sequence files' contract buffers go to jfgpu_query_ascii as they are and
the k-mers are rolled, made canonical and looked up in one kernel, for every mer length (sub_commands/query_main.cc:44-51).
The output is the host path's, byte for byte (JFGPU_QUERY_HOST=1: binary search in the mapped file), its counts are the
dump's, and JFGPU_QUERY_TRACE says which of the two answered.  A device that cannot take the table hands over to the host
before anything is written."""
import json
import os
import random
import subprocess

import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.environ.get("JFGPU_CLI") or os.path.join(ROOT, "bin", "jellyfish-amd")    # JFGPU_CLI: tests/host/build_emu.sh debugging build
_COMP = str.maketrans("ACGTacgt", "TGCAtgca")


@pytest.fixture(scope="module")
def cli(gpu):
    if not os.environ.get("JFGPU_CLI"):
        subprocess.check_call(["make", "-s", "cli"], cwd=ROOT)
    return CLI


def make_db(cli, tmp_path, k, flags, rng):
    genome = "".join(rng.choice("ACGT") for _ in range(20000))
    fa = tmp_path / "reads.fa"
    with open(fa, "w") as f:
        for r in range(1200):
            a = rng.randrange(len(genome) - 260)
            f.write(">r%d\n%s\n" % (r, genome[a:a + 260]))
    db = str(tmp_path / "db.jf")
    subprocess.check_call([cli, "count", "-m", str(k), "-s", "1M", "-o", db] + flags + [str(fa)])
    return genome, db


def make_query(tmp_path, genome, rng):
    """Reads with an N, lower case, a record over several lines, the other strand, and sequence the database has not seen."""
    q = tmp_path / "q.fa"
    multi = genome[5000:5900]
    with open(q, "w") as f:
        f.write(">known\n%s\n" % genome[100:700])
        f.write(">with_N\n%sN%s\n" % (genome[3000:3200], genome[3200:3400]))
        f.write(">lower\n%s\n" % (genome[8000:8150].lower() + genome[8150:8300]))
        f.write(">multi line\n%s\n" % "\n".join(multi[i:i + 70] for i in range(0, len(multi), 70)))
        f.write(">other_strand\n%s\n" % genome[12000:12400].translate(_COMP)[::-1])
        f.write(">novel\n%s\n" % "".join(rng.choice("ACGT") for _ in range(500)))
    return str(q), [600, 200, 200, 300, 900, 400, 500]       # the lengths of the runs of bases


def run_query(cli, db, q, **env):
    r = subprocess.run([cli, "query", db, "-s", q], env=dict(os.environ, JFGPU_QUERY_TRACE="1", **env), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    trace = [l for l in r.stderr.decode().splitlines() if l.startswith("query: ")]
    assert len(trace) == 1, r.stderr.decode()
    return r.stdout, trace[0], r.stderr.decode()


@pytest.mark.parametrize("k,flags", [(21, ["-C"]), (40, ["-C"]), (100, ["-C"]), (100, [])], ids=["21C", "40C", "100C", "100"])
def test_query_sequence_on_the_device_equals_the_host_path(cli, tmp_path, k, flags):
    rng = random.Random(11 * k + len(flags))
    genome, db = make_db(cli, tmp_path, k, flags, rng)
    q, runs = make_query(tmp_path, genome, rng)
    dev, dev_trace, _ = run_query(cli, db, q)
    host, host_trace, _ = run_query(cli, db, q, JFGPU_QUERY_HOST="1")
    mers = sum(n - k + 1 for n in runs)
    assert host_trace == "query: host"
    assert dev_trace.startswith("query: device k=%d positions=" % k) and dev_trace.endswith(" mers=%d" % mers)
    assert int(dev_trace.split("positions=")[1].split()[0]) >= sum(runs)
    assert dev == host
    lines = dev.decode().splitlines()
    assert len(lines) == mers
    want = dict(l.split() for l in subprocess.check_output([cli, "dump", "-c", db]).decode().splitlines())
    assert all(want.get(l.split()[0], "0") == l.split()[1] for l in lines)
    found = sum(1 for l in lines if l.split()[1] != "0")
    assert found >= mers // 3 and len(lines) - found >= mers // 10
    if O.have_ref():
        # oracle/_ref/ref_jf's query takes k-mers, not -s: the reference's binary_query is asked for the k-mers of the
        # output, in order, and must print the same bytes
        for a in range(0, len(lines), 500):
            asked = [l.split()[0] for l in lines[a:a + 500]]
            assert subprocess.check_output([O.REF_JF, "query", db] + asked).decode().splitlines() == lines[a:a + 500]


def test_host_answers_when_the_device_cannot_take_the_table(cli, tmp_path):
    """The database's header is rewritten to a size of 2^50 entries (the JSON header is re-serialised with its length prefix
    and padding; the host's search reads positions through the matrix and is not touched by it): jfgpu_create refuses or
    fails to allocate, nothing has been written, and the host path answers.  No device fault is involved."""
    k = 21
    rng = random.Random(5)
    genome, db = make_db(cli, tmp_path, k, ["-C"], rng)
    q, runs = make_query(tmp_path, genome, rng)
    raw = open(db, "rb").read()
    hlen = int(raw[:9])
    header = json.loads(raw[9:9 + hlen].rstrip(b"\0").decode())
    assert header["size"] == 1 << 20
    header["size"] = 1 << 50
    js = json.dumps(header, separators=(",", ":")).encode()
    js += b"\0" * (-(9 + len(js)) % header.get("alignment", 8))
    big = str(tmp_path / "big.jf")
    with open(big, "wb") as f:
        f.write(b"%09d" % len(js) + js + raw[9 + hlen:])
    want, _, _ = run_query(cli, db, q, JFGPU_QUERY_HOST="1")
    got, trace, err = run_query(cli, big, q)
    assert trace == "query: host" and got == want and len(got.splitlines()) == sum(n - k + 1 for n in runs)
    assert "answering on the host" in err
    _, trace, err = run_query(cli, big, q, JFGPU_QUIET="1")
    assert trace == "query: host" and "answering on the host" not in err
