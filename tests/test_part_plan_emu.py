"""CPU run (not -m gpu): what the partitioned insert path decides -- which P1 kernel, when to flush first, which P2, how many
groups, which arena blocks -- checked without a device by tests/host/plan_check.cc.  The plans are pure functions of plain
facts (jellyfish_amd/csrc/part_plan.inl); the program calls them on facts written out by hand and on the rows of
tests/host/plan_cases.txt, which the code printed before it was split into plan and executor, and compares with
expectations that do not come from the plan code.  Built here with AddressSanitizer and UndefinedBehaviorSanitizer into a
stand-alone program and run as a plain child process.

The build takes about as long as the emulated engine's own (tests/host/build_emu.sh)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every arm of the plans a row must reach (plan_check prints "arm <name>" for each it saw)
ARMS = [
    # what the GPU tests of the 2^33 / 2^34-slot geometries assert from the counters, and the rule no GPU test reaches
    "gpu_rows_roles", "gpu_rows_shared_ring", "gpu_rows_exact_batch", "gran_max_exact", "gran_max_pairs_single_pass",
    "granule_cap_too_large", "granule_cap_small_batch",
    # P1: every kind of kernel, the four reasons to flush first, the two refusals
    "p1_ring", "p1_keys_granule", "p1_granule64", "p1_wide", "p1_exact_sorted", "p1_exact_keys_sorted", "p1_exact_plain",
    "p1_flush_segments", "p1_flush_wide_share", "p1_flush_even", "p1_flush_arena_full", "p1_refuse_wide", "p1_refuse_filter",
    # the flush: routes, P2 kinds, groups, switches, arenas too small
    "flush_items_direct", "flush_single_level_one_word", "flush_single_level_two_word",
    "flush_sort_4", "flush_sort_8", "flush_sort_16", "flush_exact_pair", "flush_exact_tiles",
    "flush_share_forced_single_pass", "flush_share_forced_exact", "flush_p2_cap", "flush_two_streams", "flush_tile_pair_0",
    "flush_arena_too_small_for_regions",      # (a row written out by hand: no recorded flush was large enough for it)
    "flush_arena_too_small_for_tmp",
]


def test_plans_of_the_partitioned_insert_match_what_the_code_decided_before_the_split(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-x", "c++", "-DJFGPU_EMU", "-I" + os.path.join(ROOT, "tests", "host", "hip_emu"),
                           "-pthread", "-w", "-o", exe, os.path.join(ROOT, "tests", "host", "plan_check.cc")], cwd=ROOT, timeout=1500)
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "host", "plan_cases.txt")], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-3000:]
    assert "plan_check: ok" in r.stdout
    assert "FAILED" not in r.stdout
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    seen = {line.split()[2] for line in r.stdout.splitlines() if line.startswith("plan_check: arm ")}
    missing = [a for a in ARMS if a not in seen]
    assert not missing, missing
