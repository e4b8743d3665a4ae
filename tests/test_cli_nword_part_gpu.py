"""The reference's tests/large_key.sh case, set up exactly as tests/test_cli_gpu.py::test_large_key_golden_k100 sets it up
(oracle/_ref's generator, the first 10001 lines of seq1m_0.fa, 100-mers), counted with JFGPU_MODE=2 in the environment: the
partitioned insert of four-word keys (kernels_nword_part.hip.hpp) behind the command line.  A table that fits (-s 2M), a
size hint 1000 times too small (-s 2k: ten doublings, the partition geometry re-made each time) and -s 2k --disk (sorted
runs merged at the end) give the golden ordered md5 of the manifest, and a JFGPU_FLUSH_TRACE line on stderr shows that the
tile kernel of these keys ran."""
import hashlib
import json
import os
import subprocess

import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MANIFEST = json.load(open(os.path.join(ROOT, "tests", "golden", "manifest.json")))
CLI = os.environ.get("JFGPU_CLI") or os.path.join(ROOT, "bin", "jellyfish-amd")


@pytest.fixture(scope="module")
def cli(gpu):
    if not os.environ.get("JFGPU_CLI"):
        subprocess.check_call(["make", "-s", "cli"], cwd=ROOT)
    return CLI


@pytest.fixture(scope="module")
def large_key_input(tmp_path_factory):
    if not os.access(O.REF_GEN, os.X_OK):
        pytest.skip("oracle/_ref not built")
    d = str(tmp_path_factory.mktemp("large_key"))
    subprocess.check_call([O.REF_GEN, "-o", "seq1m"] + MANIFEST["reference_md5"]["seq1m"], cwd=d)
    return d, b"".join(open(os.path.join(d, "seq1m_0.fa"), "rb").readlines()[:10001])


@pytest.mark.parametrize("name,extra", [("m100_2M.jf", ["-s", "2M"]), ("m100_2k.jf", ["-s", "2k"]), ("m100_2k_disk.jf", ["-s", "2k", "--disk"])])
def test_large_key_golden_k100_through_the_partitioned_path(cli, large_key_input, name, extra):
    d, head = large_key_input
    env = dict(os.environ, JFGPU_MODE="2", JFGPU_FLUSH_TRACE="1")
    r = subprocess.run([cli, "count", "-t", "4", "-o", name, "-m", "100"] + extra + ["/dev/fd/0"], input=head, cwd=d, env=env, stderr=subprocess.PIPE, check=True)
    trace = r.stderr.decode(errors="replace")
    assert "tile_insert_nword_kernel" in trace and "p1_nword_granule_kernel" in trace, trace[-2000:]
    out = subprocess.check_output([cli, "dump", "-c", name], cwd=d)
    md5 = hashlib.md5(b"".join(sorted(l.split(b" ")[0] + b"\n" for l in out.splitlines()))).hexdigest()
    assert md5 == MANIFEST["reference_md5"]["large_key_m100.ordered"], name
