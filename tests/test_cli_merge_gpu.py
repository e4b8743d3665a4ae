"""`jellyfish-amd merge` on the GPU (-m gpu): binary/sorted inputs are merged by jfgpu_merge_run over the mapped files
(jellyfish_amd/csrc/abi_merge.inl) and the output file is the host heap's, byte for byte (JFGPU_MERGE_HOST=1 runs that one:
do_merge in jellyfish_amd/cli/jellyfish_amd.cc, jellyfish/merge_files.cc:36-176).  JFGPU_MERGE_TRACE says which of the two
merged.  The inputs are what the CLI itself writes: count --disk --no-merge -s 2k over each of tests/golden's read files, at
k = 21 (one key word) and k = 40 (two).  At k = 21 the table is far too small and every count leaves several sorted runs; at
k = 40 the smallest table of two-word keys holds a golden file's 40-mers, so every count leaves one sorted database -- four
inputs of one size and matrix all the same.  count --disk over all the files at once ends in the same records."""
import glob
import json
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CLI = os.environ.get("JFGPU_CLI") or os.path.join(ROOT, "bin", "jellyfish-amd")    # JFGPU_CLI: tests/host/build_emu.sh debugging build
READS = [os.path.join(GOLD, f) for f in ("reads150_s42.fa", "reads150_dup.fa", "edge_cases.fa", "reads_fq_s1473540700.fq")]
ENV = dict(os.environ, SOURCE_DATE_EPOCH="1700000000", JFGPU_MERGE_TRACE="1")      # headers without the clock, the host's name and the directory


@pytest.fixture(scope="module")
def cli(gpu):
    if not os.environ.get("JFGPU_CLI"):
        subprocess.check_call(["make", "-s", "cli"], cwd=ROOT)
    return CLI


def split_file(path):
    raw = open(path, "rb").read()
    hlen = int(raw[:9])
    return json.loads(raw[9:9 + hlen].rstrip(b"\0").decode()), raw[9 + hlen:]


@pytest.fixture(scope="module", params=[21, 40], ids=["k21", "k40"])
def runs(cli, tmp_path_factory, request):
    """(k, directory, the sorted runs of count --disk --no-merge)"""
    k = request.param
    d = str(tmp_path_factory.mktemp("runs%d" % k))
    for i, f in enumerate(READS):
        subprocess.run([cli, "count", "-m", str(k), "-C", "-s", "2k", "--disk", "--no-merge", "-o", "part%d_" % i, f], cwd=d, env=ENV, check=True, timeout=300)
    parts = sorted(glob.glob(os.path.join(d, "part[0-9]_*")))
    assert len(parts) >= (8 if k == 21 else 4)
    assert all(split_file(p)[0]["format"] == "binary/sorted" for p in parts)
    return k, d, parts


def merge(cli, d, out, args, parts, **env):
    """(output file's bytes or stdout text, the trace line, stderr)"""
    r = subprocess.run([cli, "merge", "-o", out] + args + parts, cwd=d, env=dict(ENV, **env), capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    trace = [l for l in r.stderr.decode().splitlines() if l.startswith("merge: device ") or l.startswith("merge: host ")]
    assert len(trace) == 1, r.stderr.decode()
    return open(os.path.join(d, out), "rb").read(), trace[0], r.stderr.decode()


def field(trace, name):
    return int(trace.split(name + "=")[1].split()[0])


@pytest.mark.parametrize("args", [[], ["-m"], ["-M"], ["-L", "2", "-U", "5"], ["-M", "-L", "3"], ["-j"]],
                         ids=["sum", "min", "max", "L2-U5", "max-L3", "jaccard"])
def test_merge_on_the_device_writes_the_host_paths_file(cli, runs, args):
    k, d, parts = runs
    dev, dev_trace, _ = merge(cli, d, "out.jf", args, parts)
    host, host_trace, _ = merge(cli, d, "out.jf", args, parts, JFGPU_MERGE_HOST="1")
    assert dev_trace.startswith("merge: device inputs=%d windows=" % len(parts)), dev_trace
    assert host_trace.startswith("merge: host inputs=%d windows=0 records=" % len(parts)), host_trace
    n_in = sum(len(split_file(p)[1]) // ((2 * k + 7) // 8 + split_file(p)[0]["counter_len"]) for p in parts)
    assert field(dev_trace, "records") == field(host_trace, "records") == n_in
    assert field(dev_trace, "written") == field(host_trace, "written")
    assert dev == host                                           # the whole file, header and records
    if args == ["-j"]:
        lines = dev.decode().splitlines()
        assert len(lines) == 2 and lines[0].startswith("Jaccard  ") and lines[1].startswith("wJaccard ")
    else:
        header, body = split_file(os.path.join(d, "out.jf"))
        assert len(body) == field(dev_trace, "written") * ((2 * k + 7) // 8 + header["counter_len"])
        assert (len(body) > 0) or args == ["-m"]                 # (a k-mer in every run is rare: -m may keep nothing)


def test_small_windows_write_the_same_file(cli, runs):
    """JFGPU_MERGE_WINDOW=500 over some 15,000 records: the position range goes through the device in dozens of windows."""
    k, d, parts = runs
    whole, t1, _ = merge(cli, d, "w1.jf", [], parts)
    cut, t2, _ = merge(cli, d, "w1.jf", [], parts, JFGPU_MERGE_WINDOW="500")
    assert cut == whole and field(t1, "windows") == 1 and field(t2, "windows") >= max(24, field(t1, "records") // 500)


def test_count_disk_ends_in_the_same_merge(cli, runs):
    k, d, parts = runs
    merged, _, _ = merge(cli, d, "merged.jf", [], parts)
    r = subprocess.run([cli, "count", "-m", str(k), "-C", "-s", "2k", "--disk", "-o", "auto.jf"] + READS, cwd=d, env=ENV, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    trace = [l for l in r.stderr.decode().splitlines() if l.startswith("merge: ")]
    if k == 21:                                                  # the table spilled: the runs went through the device merge
        assert len(trace) == 1 and trace[0].startswith("merge: device inputs=") and field(trace[0], "inputs") >= 3, r.stderr.decode()
    else:                                                        # (it held everything: written out directly)
        assert trace == []
    assert not glob.glob(os.path.join(d, "auto.jf[0-9]*"))       # the runs were merged and unlinked
    h1, b1 = split_file(os.path.join(d, "merged.jf"))
    h2, b2 = split_file(os.path.join(d, "auto.jf"))
    assert b1 == b2 and len(b1) > 0
    assert set(h1) <= set(h2) and {"size", "key_len", "counter_len", "format"} <= set(h1)
    for f in set(h1) - {"cmdline", "exe_path"}:                  # (the two commands' own; count's header also has canonical and val_len)
        assert h1[f] == h2[f], f


def test_text_inputs_are_merged_on_the_host(cli, tmp_path):
    d = str(tmp_path)
    subprocess.run([cli, "count", "-m", "21", "-C", "-s", "2k", "--text", "--disk", "--no-merge", "-o", "t"] + READS[:2], cwd=d, env=ENV, check=True, timeout=300)
    parts = sorted(glob.glob(os.path.join(d, "t[0-9]*")))
    assert len(parts) >= 2
    out, trace, _ = merge(cli, d, "t.jf", [], parts)
    assert trace.startswith("merge: host inputs=%d " % len(parts)) and len(out) > 0


def test_host_merges_when_the_device_declines(cli, runs):
    """A header that names a size that is no power of two is one jfgpu_merge_create refuses; nothing has been written, the
    host path merges and says so once (not under JFGPU_QUIET).  No device fault is involved."""
    k, d, parts = runs
    odd = []
    for i, p in enumerate(parts[:2]):
        raw = open(p, "rb").read()
        hlen = int(raw[:9])
        header = json.loads(raw[9:9 + hlen].rstrip(b"\0").decode())
        header["size"] = header["size"] * 3
        js = json.dumps(header, separators=(",", ":")).encode()
        js += b"\0" * (-(9 + len(js)) % header.get("alignment", 8))
        odd.append(os.path.join(d, "odd%d" % i))
        with open(odd[-1], "wb") as f:
            f.write(b"%09d" % len(js) + js + raw[9 + hlen:])
    want, _, _ = merge(cli, d, "odd_host.jf", [], odd, JFGPU_MERGE_HOST="1")
    got, trace, err = merge(cli, d, "odd_host.jf", [], odd)
    assert trace.startswith("merge: host ") and got == want and "merging on the host" in err
    _, trace, err = merge(cli, d, "odd_host.jf", [], odd, JFGPU_QUIET="1")
    assert trace.startswith("merge: host ") and "merging on the host" not in err
