"""CPU run of the stage tests (not -m gpu): tests/kernels/stage_harness.hip compiled by g++ against tests/host/hip_emu, then
tests/test_gpu_stage_*.py executed against that library in a subprocess each -- the ring, tile, sort-based, two-word and
partitioned-Bloom kernels' logic checked against their stage contracts on every CPU test run, without a device.

What this is and is not: see tests/test_emu_kernels.py.  The harness library under tests/host/_build is test infrastructure,
loaded only here (JFKT_LIB); races, memory ordering and speed are the GPU run's to judge.  Measured times of the eight
modules under the emulation: profiles/stage_harness_emu_times.txt.  One case is the device's alone: the two-word tile
kernel at k = 63 in a table of 2^29 slots (8 GB) skips itself here, as the k = 63 tests of tests/test_gpu_wide.py do."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "host", "_build")
MODULES = ["tests/test_gpu_stage_p2.py", "tests/test_gpu_stage_tile.py", "tests/test_gpu_stage_p1.py",
           "tests/test_gpu_stage_p2_sort.py", "tests/test_gpu_stage_p1_wide.py", "tests/test_gpu_stage_tile_wide.py",
           "tests/test_gpu_stage_bloom_p1.py", "tests/test_gpu_stage_bloom_seg.py"]
SKIPS = {"tests/test_gpu_stage_tile_wide.py": 1}             # (the k = 63 case at 2^29 slots)


@pytest.fixture(scope="module")
def emu_libs():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    subprocess.check_call([os.path.join(ROOT, "tests", "host", "build_emu.sh")])
    subprocess.check_call([os.path.join(ROOT, "tests", "host", "build_kt_emu.sh")])
    libs = os.path.join(BUILD, "libjfgpu_emu.so"), os.path.join(BUILD, "libjfgpu_kt_emu.so")
    assert all(os.path.exists(p) for p in libs)
    return libs


@pytest.mark.parametrize("module", MODULES)
def test_stage_tests_pass_on_the_host_emulation(emu_libs, module):
    # (JFGPU_LIB: the `gpu` fixture asks the product binding for a device; the stage tests themselves use JFKT_LIB's only)
    env = dict(os.environ, JFGPU_LIB=emu_libs[0], JFKT_LIB=emu_libs[1], JFGPU_EMU_THREADS="4")
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider", "--durations=5", module],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout
    if SKIPS.get(module):
        assert "%d skipped" % SKIPS[module] in r.stdout
    else:
        assert "skipped" not in r.stdout
