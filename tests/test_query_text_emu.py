"""CPU run (not -m gpu) of the Bloom-counter query and of the query formatter: the engine's device sources built against the
host emulation (tests/host/build_emu.sh, as tests/test_emu_kernels.py does), then a named selection of
tests/test_gpu_bloom_query.py and tests/test_gpu_query_text.py against that library in a subprocess -- check() of a sequence
at every key view against the oracle, the reference's file bodies, the tile edges, the device form's guards, pending
partitioned increments; format_dev at every mer length, alignment and count value; the host forms' pieces, sinks and
refusals on a table and on a counter.

The selection is every case of the two modules: none of them puts a table at k = 63, 64 or 128, whose smallest geometries
(8, 32 and 64 GB) the emulation does not allocate -- the tables are of 21-, 40- and 100-mers, and every k from 1 to 128 goes
through a Bloom counter and through format_dev, which need none.  Left to the GPU run: the command line
(tests/test_cli_query_text_gpu.py), and everything the emulation cannot show -- what the kernels' stores and loads do at
their real alignment and width on the device, LDS sizes, occupancy and speed.

What this is and is not: see tests/test_emu_kernels.py."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "host", "_build")

B = "tests/test_gpu_bloom_query.py::"
Q = "tests/test_gpu_query_text.py::"
PIECES = ("k", "1000", "4096", "default")
SELECTION = [B + "test_every_key_view_against_the_oracle[%d-%s]" % (k, c)
             for k in (1, 12, 21, 31, 32, 33, 40, 63, 64, 65, 96, 97, 128) for c in ("C", "fw")] + \
            [B + "test_a_counter_of_1009_cells[%d]" % k for k in (21, 40, 100)] + \
            [B + "test_reference_files[%s]" % n for n in ("bc_k21C", "bc_k31", "bc_k100C", "bc_k65")] + \
            [B + "test_tile_edges[%d]" % k for k in (21, 40, 100)] + \
            [B + "test_unaligned_device_buffers_and_guards[%d]" % k for k in (21, 40, 100)] + \
            [B + "test_query_sees_pending_partitioned_increments", B + "test_errors"] + \
            [Q + "test_format_dev[%d]" % k for k in (1, 2, 21, 32, 33, 64, 65, 128)] + \
            [Q + "test_query_text_of_a_table[%d-%s]" % (k, p) for k in (21, 40, 100) for p in PIECES] + \
            [Q + "test_query_text_of_a_bloom_counter[%d-%s]" % (k, p) for k in (21, 65) for p in PIECES] + \
            [Q + "test_errors"]


@pytest.fixture(scope="module")
def emu_lib():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    subprocess.check_call([os.path.join(ROOT, "tests", "host", "build_emu.sh")])
    lib = os.path.join(BUILD, "libjfgpu_emu.so")
    assert os.path.exists(lib)
    return lib


def test_bloom_query_and_query_text_on_the_host_emulation(emu_lib):
    env = dict(os.environ, JFGPU_LIB=emu_lib, JFGPU_CLI=os.path.join(BUILD, "jellyfish-amd-emu"), JFGPU_EMU_THREADS="4")
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider"] + SELECTION,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "%d passed" % len(SELECTION) in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout
