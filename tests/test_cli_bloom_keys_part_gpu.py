"""`bc` for mers above 32 bases with JFGPU_BLOOM_MODE in the environment: the partitioned Bloom insert of two- to four-word
keys (kernels_bloom_part_keys.hip.hpp) behind the command line.  `bc -s 30M -f 0.001` makes a counter of 420 M cells (1282
segments: two levels, so the flush prints its JFGPU_FLUSH_TRACE line); the file written under JFGPU_BLOOM_MODE=partitioned is
the file written under JFGPU_BLOOM_MODE=direct byte for byte (SOURCE_DATE_EPOCH pins the header's provenance), and the flush
line on stderr shows that the switch took effect."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CLI = os.environ.get("JFGPU_CLI") or os.path.join(ROOT, "bin", "jellyfish-amd")


@pytest.fixture(scope="module")
def cli(gpu):
    if not os.environ.get("JFGPU_CLI"):
        subprocess.check_call(["make", "-s", "cli"], cwd=ROOT)
    return CLI


@pytest.mark.parametrize("k", [100, 63])
def test_bc_partitioned_writes_the_direct_file(cli, tmp_path, k):
    inp = os.path.join(GOLD, "reads150_dup.fa")
    files, traces = {}, {}
    for mode, extra in (("direct", {}), ("partitioned", {"JFGPU_FLUSH_TRACE": "1"})):
        d = tmp_path / mode                                    # (the header records the command line: the same one in both runs)
        d.mkdir()
        env = dict(os.environ, JFGPU_BLOOM_MODE=mode, SOURCE_DATE_EPOCH="0", **extra)
        r = subprocess.run([cli, "bc", "-m", str(k), "-C", "-s", "30M", "-f", "0.001", "-o", "out.bc", inp], cwd=str(d), env=env, stderr=subprocess.PIPE,
                           check=True, timeout=600)
        files[mode] = open(str(d / "out.bc"), "rb").read()
        traces[mode] = r.stderr.decode(errors="replace")
    assert len(files["direct"]) > 80_000_000
    assert files["partitioned"] == files["direct"]
    assert "[jfgpu flush] Bloom:" in traces["partitioned"], traces["partitioned"][-2000:]
    assert "[jfgpu flush]" not in traces["direct"]
