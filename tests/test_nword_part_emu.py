"""CPU run (not -m gpu) of the partitioned insert of three- and four-word keys (kernels_nword_part.hip.hpp):

  * the engine and tests/kernels/stage_harness_nword.hip compiled by g++ against tests/host/hip_emu (as
    tests/test_stage_kernels_emu.py builds the other harness), then tests/test_gpu_stage_nword.py and a subset of
    tests/test_gpu_nword_part.py -- k = 65 at 2^12 slots, k = 100 at 2^22 -- executed against those libraries in a subprocess each;
  * tests/host/nword_plan_check.cc, built with AddressSanitizer and UndefinedBehaviorSanitizer into a stand-alone program and
    run as a plain child process: the partition geometry of every k in 65 .. 128 at every legal lsize (no geometry's largest
    item is the all-ones hole), the plans part_plan.inl makes for these keys, and that every kernel they name exists.

What this is and is not: see tests/test_emu_kernels.py.  Races, memory ordering and speed are the GPU run's to judge."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "host", "_build")
RUNS = [
    ("tests/test_gpu_stage_nword.py", None),
    ("tests/test_gpu_nword_part.py", "65-12 or uniform and 22"),
    ("tests/test_gpu_nword_part.py", "overflow or growth or flushed or attach"),
]


@pytest.fixture(scope="module")
def emu_libs():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    subprocess.check_call([os.path.join(ROOT, "tests", "host", "build_emu.sh")])
    subprocess.check_call([os.path.join(ROOT, "tests", "host", "build_ktn_emu.sh")])
    libs = os.path.join(BUILD, "libjfgpu_emu.so"), os.path.join(BUILD, "libjfgpu_ktn_emu.so")
    assert all(os.path.exists(p) for p in libs)
    return libs


@pytest.mark.parametrize("module,select", RUNS, ids=lambda v: (v or "all").replace("tests/", "").replace(" ", "_"))
def test_nword_partitioned_tests_pass_on_the_host_emulation(emu_libs, module, select):
    env = dict(os.environ, JFGPU_LIB=emu_libs[0], JFKTN_LIB=emu_libs[1], JFGPU_EMU_THREADS="4")
    cmd = [sys.executable, "-m", "pytest", "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider", "--durations=5", module]
    if select:
        cmd += ["-k", select]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout


def test_geometry_and_plans_of_three_and_four_word_keys(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "nword_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-x", "c++", "-DJFGPU_EMU", "-I" + os.path.join(ROOT, "tests", "host", "hip_emu"),
                           "-pthread", "-w", "-o", exe, os.path.join(ROOT, "tests", "host", "nword_plan_check.cc")], cwd=ROOT, timeout=1500)
    r = subprocess.run([exe], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-3000:]
    assert "nword_plan_check: ok" in r.stdout and "FAILED" not in r.stdout
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
