"""CPU run (not -m gpu) of the look-ups in sorted records: the engine's device sources built against the host emulation
(tests/host/build_emu.sh, as tests/test_bloom_nword_emu.py does), then a selection of tests/test_gpu_sorted_query.py and
tests/test_cli_query_sorted_gpu.py against that library in a subprocess -- every key width once (k = 63, 64 and 128 among
them: no table is built, so they are as small as the rest), the index seams, the runs of empty buckets, the refusals and one
case of the command line.  Left to the GPU run: the other strand of every width, the record shapes, the near misses, the
unaligned device buffers and the rest of the command line."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "host", "_build")

T = "tests/test_gpu_sorted_query.py::"
SELECTION = [T + "test_every_key_width_against_the_oracle[%d-C]" % k for k in (5, 21, 31, 32, 33, 40, 63, 64, 65, 96, 97, 100, 128)] + \
            [T + "test_index_seams[%d-%s]" % (n, per) for n in (0, 1, 2, 255, 256, 257, 513) for per in ("1", "8", "n")] + \
            [T + "test_three_records_in_a_large_file", T + "test_runs_of_empty_buckets", T + "test_refusals",
             "tests/test_cli_query_sorted_gpu.py::test_records_table_host_and_host_lines_agree[100C]"]


@pytest.fixture(scope="module")
def emu_lib():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    subprocess.check_call([os.path.join(ROOT, "tests", "host", "build_emu.sh")])
    lib = os.path.join(BUILD, "libjfgpu_emu.so")
    assert os.path.exists(lib)
    return lib


def test_sorted_query_on_the_host_emulation(emu_lib):
    env = dict(os.environ, JFGPU_LIB=emu_lib, JFGPU_CLI=os.path.join(BUILD, "jellyfish-amd-emu"), JFGPU_EMU_THREADS="4")
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider"] + SELECTION,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "%d passed" % len(SELECTION) in r.stdout and "failed" not in r.stdout
