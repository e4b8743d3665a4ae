"""`jellyfish-amd query -s` answered from the sorted records on the device (-m gpu): the body of a binary/sorted database goes
up as the file has it and is looked up where it lies (jfgpu_sorted_create, jfgpu_sorted_query_text); JFGPU_QUERY_TABLE=1
keeps the path that loads the records into a hash table.  The output of the records path is, byte for byte, that of the table
path, of the host path (JFGPU_QUERY_HOST=1) and of the device look-up with host-built lines (JFGPU_QUERY_FORMAT_HOST=1), to
stdout and to -o, for databases of this and of other writers; the trace names the path (lookup=records | lookup=table)."""
import os
import random
import subprocess

import pytest

from test_cli_query_gpu import ROOT, cli, make_db, make_query, run_query    # noqa: F401 (cli is a fixture)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden")


def fields(trace):
    return dict(f.split("=") for f in trace.split()[2:])


def parity(cli, db, q, tmp_path, k=None):
    """The four paths print the same bytes; returns them."""
    rec, rec_trace, _ = run_query(cli, db, q)
    tab, tab_trace, _ = run_query(cli, db, q, JFGPU_QUERY_TABLE="1")
    host, host_trace, _ = run_query(cli, db, q, JFGPU_QUERY_HOST="1")
    fmt, fmt_trace, _ = run_query(cli, db, q, JFGPU_QUERY_FORMAT_HOST="1")
    assert host_trace == "query: host"
    for trace, lookup, lines in ((rec_trace, "records", "device"), (tab_trace, "table", "device"), (fmt_trace, "records", "host")):
        f = fields(trace)
        assert trace.startswith("query: device k=") and f["lookup"] == lookup and f["format"] == lines and f["db"] == "binary", trace
        assert trace.split()[-1] == "mers=%d" % len(host.splitlines()), trace
        assert float(f["load_ms"]) >= 0 and (k is None or int(f["k"]) == k)
    assert len(host) > 0 and rec == host and tab == host and fmt == host
    out = str(tmp_path / "out.txt")
    r = subprocess.run([cli, "query", db, "-s", q, "-o", out], env=dict(os.environ, JFGPU_QUERY_TRACE="1"), capture_output=True)
    assert r.returncode == 0 and r.stdout == b"" and "lookup=records" in r.stderr.decode(), r.stderr.decode()
    assert open(out, "rb").read() == host
    return host


@pytest.mark.parametrize("k,flags", [(21, ["-C"]), (40, ["-C"]), (100, ["-C"]), (100, [])], ids=["21C", "40C", "100C", "100"])
def test_records_table_host_and_host_lines_agree(cli, tmp_path, k, flags):
    rng = random.Random(13 * k + len(flags))
    genome, db = make_db(cli, tmp_path, k, flags, rng)
    q, runs = make_query(tmp_path, genome, rng)
    out = parity(cli, db, q, tmp_path, k)
    lines = out.decode().splitlines()
    mers = sum(n - k + 1 for n in runs)
    found = sum(1 for l in lines if l.split()[1] != "0")
    assert len(lines) == mers and found >= mers // 3 and mers - found >= mers // 10


@pytest.mark.parametrize("db,fa", [("reads150_k21C.ref.jf", "reads150_s42.fa"), ("edge_k8C.ref.jf", "edge_cases.fa")])
def test_a_database_written_by_the_reference(cli, tmp_path, db, fa):
    out = parity(cli, os.path.join(GOLDEN, db), os.path.join(GOLDEN, fa), tmp_path)
    assert sum(1 for l in out.decode().splitlines() if l.split()[1] != "0") > 100


@pytest.mark.parametrize("writer", ["matrix_xs", "merge", "one_counter_byte"])
def test_other_writers(cli, tmp_path, writer):
    k = 21
    rng = random.Random(77)
    genome, db = make_db(cli, tmp_path, k, ["-C"], rng)
    q, _ = make_query(tmp_path, genome, rng)
    fa = str(tmp_path / "reads.fa")
    want = [l.split() for l in run_query(cli, db, q, JFGPU_QUERY_HOST="1")[0].decode().splitlines()]
    other = str(tmp_path / "other.jf")
    if writer == "matrix_xs":                                 # the xor-shift matrix family: the same counts under another matrix
        subprocess.check_call([cli, "count", "-m", str(k), "-s", "1M", "-C", "--matrix", "xs", "-o", other, fa])
        assert [l.split() for l in parity(cli, other, q, tmp_path, k).decode().splitlines()] == want
    elif writer == "merge":                                   # a merge of the database with itself: every count twice
        subprocess.check_call([cli, "merge", "-o", other, db, db])
        twice = [int(l.split()[1]) for l in parity(cli, other, q, tmp_path, k).decode().splitlines()]
        assert all(c % 2 == 0 for c in twice) and sum(1 for c in twice if c) > 500
    else:                                                     # one counter byte, singletons left out
        subprocess.check_call([cli, "count", "-m", str(k), "-s", "1M", "-C", "-L", "2", "--out-counter-len", "1", "-o", other, fa])
        got = [int(l.split()[1]) for l in parity(cli, other, q, tmp_path, k).decode().splitlines()]
        assert got == [min(255, int(c)) if int(c) >= 2 else 0 for _, c in want] and sum(1 for c in got if c) > 500


def split_db(path):
    raw = open(path, "rb").read()
    off = 9 + int(raw[:9])
    return raw[:off], raw[off:]


def test_truncated_body(cli, tmp_path):
    """A body cut in the middle of a record is refused before any look-up, on the device and on the host alike."""
    k = 21
    rng = random.Random(3)
    genome, db = make_db(cli, tmp_path, k, ["-C"], rng)
    q, _ = make_query(tmp_path, genome, rng)
    head, body = split_db(db)
    cut = str(tmp_path / "cut.jf")
    with open(cut, "wb") as f:
        f.write(head + body[:len(body) - 3])
    res = [subprocess.run([cli, "query", cut, "-s", q], env=dict(os.environ, JFGPU_QUERY_TRACE="1", **env), capture_output=True)
           for env in ({}, {"JFGPU_QUERY_HOST": "1"})]
    assert res[0].returncode == res[1].returncode != 0
    assert res[0].stderr == res[1].stderr and b"multiple of the length of a record" in res[0].stderr and res[0].stdout == res[1].stdout == b""


def test_unsorted_body_is_answered_by_the_host(cli, tmp_path):
    k = 21
    rng = random.Random(4)
    genome, db = make_db(cli, tmp_path, k, ["-C"], rng)
    q, _ = make_query(tmp_path, genome, rng)
    head, body = split_db(db)
    rb = (2 * k + 7) // 8 + 4
    assert len(body) % rb == 0 and len(body) // rb > 1000
    a, b = body[500 * rb:501 * rb], body[501 * rb:502 * rb]
    bad = str(tmp_path / "bad.jf")
    with open(bad, "wb") as f:
        f.write(head + body[:500 * rb] + b + a + body[502 * rb:])
    want, _, _ = run_query(cli, bad, q, JFGPU_QUERY_HOST="1")
    got, trace, err = run_query(cli, bad, q)
    assert trace == "query: host" and "answering on the host" in err and "strictly increasing" in err
    assert got == want
