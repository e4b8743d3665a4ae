"""CPU run (not -m gpu) of the partitioned Bloom insert for mers of 33 to 128 bases (kernels_bloom_part_keys.hip.hpp): the
engine and tests/kernels/stage_harness_bloom_keys.hip compiled by g++ against tests/host/hip_emu (as
tests/test_nword_part_emu.py builds the n-word harness), then tests/test_gpu_stage_bloom_p1_keys.py and
tests/test_gpu_bloom_keys_part.py executed against those libraries in a subprocess each, the filter of 1282 segments (P2 on
the path) included.  Left to the GPU run: the table of 128-mers of the attach case, whose smallest size is more memory than the
emulation hands out.

What this is and is not: see tests/test_emu_kernels.py.  Races, memory ordering and speed are the GPU run's to judge."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "host", "_build")
RUNS = [
    ("tests/test_gpu_stage_bloom_p1_keys.py", None),
    ("tests/test_gpu_bloom_keys_part.py", "not (attach and 128)"),
]


@pytest.fixture(scope="module")
def emu_libs():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    subprocess.check_call([os.path.join(ROOT, "tests", "host", "build_emu.sh")])
    subprocess.check_call([os.path.join(ROOT, "tests", "host", "build_ktbk_emu.sh")])
    libs = os.path.join(BUILD, "libjfgpu_emu.so"), os.path.join(BUILD, "libjfgpu_ktbk_emu.so")
    assert all(os.path.exists(p) for p in libs)
    return libs


@pytest.mark.parametrize("module,select", RUNS, ids=lambda v: (v or "all").replace("tests/", "").replace(" ", "_"))
def test_bloom_keys_partitioned_tests_pass_on_the_host_emulation(emu_libs, module, select):
    env = dict(os.environ, JFGPU_LIB=emu_libs[0], JFKTBK_LIB=emu_libs[1], JFGPU_EMU_THREADS="4")
    cmd = [sys.executable, "-m", "pytest", "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider", "--durations=5", module]
    if select:
        cmd += ["-k", select]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout
