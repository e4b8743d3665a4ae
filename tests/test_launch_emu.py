"""CPU run (not -m gpu): the one launch entry for kernels with dynamic LDS (jellyfish_amd/csrc/hip_launch.hpp), checked by
tests/host/launch_check.cc under the host emulation, which records every hipFuncSetAttribute and aborts a launch that asks
for more than 64 KiB from a function whose limit was not raised.  The program is built stand-alone, once with AddressSanitizer
and UBSan and once with ThreadSanitizer, and run as a plain child process: the first launch of a kernel sets its limit to what
it asks for, a smaller or equal one sets nothing, a larger one raises it, kernels are independent, no LDS means no call,
eight threads on one kernel end at the largest size; and a direct hipLaunchKernelGGL at 65 KiB with no attribute aborts."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path, name, sanitize):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=" + sanitize, "-fno-omit-frame-pointer", "-DJFGPU_EMU",
                           "-I" + os.path.join(ROOT, "tests", "host", "hip_emu"), "-pthread", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "launch_check.cc")], cwd=ROOT, timeout=600)
    return exe


def run_clean(exe, tmp_path):
    r = subprocess.run([exe], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "launch_check: ok" in r.stdout
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]


def test_the_limit_is_raised_by_the_launch_and_only_upwards(tmp_path):
    exe = build(tmp_path, "launch_check", "address,undefined")
    run_clean(exe, tmp_path)
    # a launch beyond 64 KiB that did not go through the launcher: the emulator aborts, naming both sizes
    r = subprocess.run([exe, "direct"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "not refused" not in r.stdout
    assert "66560 bytes of dynamic LDS" in r.stderr and "raised to 0" in r.stderr, r.stderr[-3000:]


def test_eight_threads_on_one_kernel_without_a_data_race(tmp_path):
    run_clean(build(tmp_path, "launch_check_tsan", "thread"), tmp_path)
