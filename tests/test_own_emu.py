"""CPU run (not -m gpu): the host code's ownership of device memory, pinned memory, streams and events, checked by
tests/host/own_check.cc -- the engine's translation unit under the host emulation, built here with AddressSanitizer into a
stand-alone program and run as a plain child process.  Every allocation of every create function and of a small merge,
text, table and Bloom run is made to fail once: the call must report it, hand nothing half-built out and leave nothing
allocated; LeakSanitizer's report at exit covers what the emulation's counters do not see.  The same for the multi-GPU
communicator on its in-process transport: its create at world 2 and 4, a key-path step, an item-path step, a step whose
shards double and the merge of two Bloom counters.

The build takes about as long as the emulated engine's own (tests/host/build_emu.sh)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_failed_allocations_leave_nothing_behind(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "own_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address", "-fno-omit-frame-pointer", "-x", "c++", "-DJFGPU_EMU",
                           "-I" + os.path.join(ROOT, "tests", "host", "hip_emu"), "-pthread", "-w", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "own_check.cc")], cwd=ROOT, timeout=1500)
    r = subprocess.run([exe], cwd=str(tmp_path), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "own_check: ok" in r.stdout
    assert "Sanitizer" not in r.stderr, r.stderr[-3000:]
    # every family of entry points was reached
    for what in ("jfgpu_create k = 21", "jfgpu_create k = 40", "jfgpu_create k = 100", "jfgpu_bc_create k = 21", "jfgpu_bc_create k = 100",
                 "jfgpu_bf_create", "jfgpu_parser_create + bgzf", "jfgpu_merge_create", "jfgpu_text_create", "jfgpu_merge_run",
                 "jfgpu_text_run", "add_keys / lookup / query", "jfgpu_bc_keys", "jfgpu_comm_create_local W = 2",
                 "jfgpu_comm_create_local W = 4", "comm step, keys", "comm step, items", "comm step, comm_grow",
                 "jfgpu_comm_bc_merge_local"):
        assert what in r.stdout, what
