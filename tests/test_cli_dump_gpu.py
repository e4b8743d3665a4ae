"""`jellyfish-amd dump` and `count --text` on the GPU (-m gpu): the text of binary/sorted records comes from the device
(jfgpu_text_run over the mapped file, jfgpu_dump_next_text over the table's sorted chunks; jellyfish_amd/csrc/abi_text.inl)
and is, byte for byte, what the host loops write (JFGPU_DUMP_HOST=1 runs those: dump_main in
jellyfish_amd/cli/jellyfish_amd.cc, write_text_records_host in jellyfish_amd/include/jellyfish_amd/dumpers.hpp).
JFGPU_DUMP_TRACE says which of the two dumped.  The databases are what the CLI itself writes from tests/golden's read files:
k = 21 and k = 40 with -C, k = 100, and one with --out-counter-len 1, whose counts saturate at 255."""
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CLI = os.environ.get("JFGPU_CLI") or os.path.join(ROOT, "bin", "jellyfish-amd")    # JFGPU_CLI: tests/host/build_emu.sh debugging build
READS = [os.path.join(GOLD, f) for f in ("reads150_s42.fa", "reads150_dup.fa", "edge_cases.fa", "reads_fq_s1473540700.fq")]
ENV = dict(os.environ, SOURCE_DATE_EPOCH="1700000000")             # headers without the clock, the host's name and the directory
for _name in ("JFGPU_DUMP_HOST", "JFGPU_DUMP_DEVICE_MIN", "JFGPU_TEXT_WINDOW", "JFGPU_DUMP_TRACE"):
    ENV.pop(_name, None)

DATABASES = {"k21": ["-m", "21", "-C"], "k40": ["-m", "40", "-C"], "k100": ["-m", "100"], "k21c1": ["-m", "21", "-C", "--out-counter-len", "1"]}
VARIANTS = {"fasta": [], "column": ["-c"], "tab": ["-c", "-t"], "L2-U5": ["-L", "2", "-U", "5"], "to-file": ["-c", "-o", "out.txt"]}


@pytest.fixture(scope="module")
def cli(gpu):
    if not os.environ.get("JFGPU_CLI"):
        subprocess.check_call(["make", "-s", "cli"], cwd=ROOT)
    return CLI


def split_file(path):
    raw = open(path, "rb").read()
    hlen = int(raw[:9])
    return json.loads(raw[9:9 + hlen].rstrip(b"\0").decode()), raw[9 + hlen:]


@pytest.fixture(scope="module")
def dbs(cli, tmp_path_factory):
    """(directory, {name: (file, records)})"""
    d = str(tmp_path_factory.mktemp("dump"))
    out = {}
    for name, args in DATABASES.items():
        reads = READS * (12 if name == "k21c1" else 1)             # (the commonest 21-mer occurs 24 times: 288 saturates one byte)
        subprocess.run([cli, "count", "-s", "1M", "-o", name + ".jf"] + args + reads, cwd=d, env=ENV, check=True, timeout=300)
        header, body = split_file(os.path.join(d, name + ".jf"))
        assert header["format"] == "binary/sorted"
        rb = (header["key_len"] + 7) // 8 + header["counter_len"]
        assert len(body) % rb == 0 and len(body) // rb > 1500
        out[name] = (name + ".jf", len(body) // rb)
    assert split_file(os.path.join(d, "k21c1.jf"))[0]["counter_len"] == 1
    return d, out


def dump(cli, d, args, db, **env):
    """(the text, the trace line, exit status)"""
    if "-o" in args and os.path.exists(os.path.join(d, "out.txt")):
        os.unlink(os.path.join(d, "out.txt"))
    r = subprocess.run([cli, "dump"] + args + [db], cwd=d, env=dict(ENV, JFGPU_DUMP_TRACE="1", **env), capture_output=True, timeout=300)
    trace = [l for l in r.stderr.decode().splitlines() if l.startswith("dump: device ") or l.startswith("dump: host ")]
    assert len(trace) == 1, r.stderr.decode()
    text = open(os.path.join(d, "out.txt"), "rb").read() if "-o" in args else r.stdout
    assert ("-o" not in args) or r.stdout == b""
    return text, trace[0], r.returncode


def field(trace, name):
    return int(trace.split(name + "=")[1].split()[0])


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", list(DATABASES))
def test_dump_on_the_device_writes_the_host_paths_text(cli, dbs, name, variant):
    d, files = dbs
    db, n = files[name]
    args = VARIANTS[variant]
    dev, dev_trace, rc1 = dump(cli, d, args, db, JFGPU_DUMP_DEVICE_MIN="0")
    host, host_trace, rc2 = dump(cli, d, args, db, JFGPU_DUMP_HOST="1")
    assert rc1 == rc2 == 0
    assert dev_trace.startswith("dump: device records=%d kept=" % n), dev_trace
    assert host_trace.startswith("dump: host records=%d kept=" % n), host_trace
    assert field(dev_trace, "kept") == field(host_trace, "kept") and field(dev_trace, "bytes") == len(dev)
    kept = field(dev_trace, "kept")
    if variant != "L2-U5":
        assert kept == n
    elif name == "k100":
        assert kept == n                                           # (every 100-mer of the files occurs 2 or 3 times)
    elif name == "k21c1":
        assert kept == 0 and dev == b""                            # (every 21-mer of twelve passes occurs 12 times or more)
    else:
        assert 0 < kept < n
    assert dev == host
    assert dev.count(b"\n") == field(dev_trace, "kept") * (1 if "-c" in args else 2)
    if name == "k21c1" and variant == "column":
        assert max(int(l.split()[1]) for l in dev.decode().splitlines()) == 255          # counts saturated at one byte


def test_small_windows_write_the_same_text(cli, dbs):
    d, files = dbs
    db, n = files["k21"]
    whole, t1, _ = dump(cli, d, ["-c"], db, JFGPU_DUMP_DEVICE_MIN="0")
    cut, t2, _ = dump(cli, d, ["-c"], db, JFGPU_DUMP_DEVICE_MIN="0", JFGPU_TEXT_WINDOW="500")
    assert cut == whole and field(t1, "windows") == 1 and field(t2, "windows") == (n + 499) // 500 >= 10


def test_small_database_is_answered_by_the_host(cli, dbs):
    """With the default threshold a database of some thousands of records does not go to the device."""
    d, files = dbs
    db, n = files["k40"]
    text, trace, rc = dump(cli, d, ["-c"], db)
    assert rc == 0 and trace.startswith("dump: host records=%d kept=%d" % (n, n)), trace
    assert text == dump(cli, d, ["-c"], db, JFGPU_DUMP_DEVICE_MIN="0")[0]
    over, trace, _ = dump(cli, d, ["-c"], db, JFGPU_DUMP_DEVICE_MIN=str(n + 1))
    assert trace.startswith("dump: host ") and over == text
    at, trace, _ = dump(cli, d, ["-c"], db, JFGPU_DUMP_DEVICE_MIN=str(n))
    assert trace.startswith("dump: device ") and at == text


def test_text_input_takes_the_host_path(cli, dbs):
    d, files = dbs
    subprocess.run([cli, "count", "-m", "21", "-C", "-s", "1M", "--text", "-o", "k21.txt.jf"] + READS, cwd=d, env=ENV, check=True, timeout=300)
    assert split_file(os.path.join(d, "k21.txt.jf"))[0]["format"] == "text/sorted"
    text, trace, rc = dump(cli, d, ["-c"], "k21.txt.jf", JFGPU_DUMP_DEVICE_MIN="0")
    assert rc == 0 and trace.startswith("dump: host records=%d " % files["k21"][1]), trace
    assert text == dump(cli, d, ["-c"], files["k21"][0], JFGPU_DUMP_DEVICE_MIN="0")[0]


def test_truncated_file_gives_the_same_on_both_paths(cli, dbs):
    """A binary file cut in the middle of a record: the whole records before the cut, the same exit status."""
    d, files = dbs
    db, n = files["k40"]
    raw = open(os.path.join(d, db), "rb").read()
    header, body = split_file(os.path.join(d, db))
    rb = (header["key_len"] + 7) // 8 + header["counter_len"]
    keep = n // 2 + 1
    with open(os.path.join(d, "cut.jf"), "wb") as f:
        f.write(raw[:len(raw) - len(body) + keep * rb + rb // 2])
    dev, dev_trace, rc1 = dump(cli, d, ["-c"], "cut.jf", JFGPU_DUMP_DEVICE_MIN="0")
    host, host_trace, rc2 = dump(cli, d, ["-c"], "cut.jf", JFGPU_DUMP_HOST="1")
    assert rc1 == rc2 and dev == host and dev_trace.startswith("dump: device records=%d kept=%d " % (keep, keep))
    assert dev.count(b"\n") == keep and dev == dump(cli, d, ["-c"], db, JFGPU_DUMP_HOST="1")[0][:len(dev)]


@pytest.mark.parametrize("bounds", [[], ["-L", "2", "-U", "5"]], ids=["all", "L2-U5"])
@pytest.mark.parametrize("k", [21, 40])
def test_count_text_writes_the_host_paths_file(cli, dbs, k, bounds):
    d, _ = dbs
    files = []
    for name, env in (("dev", {}), ("host", {"JFGPU_DUMP_HOST": "1"})):
        out = "text_k%d_%d.jf" % (k, len(bounds))                  # (one name: the header holds the command line)
        r = subprocess.run([cli, "count", "-m", str(k), "-C", "-s", "1M", "--text", "-o", out] + bounds + READS, cwd=d,
                           env=dict(ENV, JFGPU_DUMP_TRACE="1", **env), capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        trace = [l for l in r.stderr.decode().splitlines() if l.startswith("[dump] text: ")]
        assert len(trace) == 1 and trace[0].endswith("formatted on the " + ("device" if name == "dev" else "host")), r.stderr.decode()
        files.append(open(os.path.join(d, out), "rb").read())
    assert files[0] == files[1]
    header, body = split_file(os.path.join(d, out))
    assert header["format"] == "text/sorted"
    lines = body.decode().splitlines()
    assert len(lines) > (100 if bounds else 1500) and all(len(l.split()[0]) == k for l in lines[:50])
    if bounds:
        assert all(2 <= int(l.split()[1]) <= 5 for l in lines)
