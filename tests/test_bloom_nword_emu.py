"""CPU run (not -m gpu) of the Bloom counters for mers of 65 to 128 bases: the engine's device sources built against the
host emulation (tests/host/build_emu.sh, as tests/test_emu_kernels.py does), then tests/test_gpu_bloom_nword.py's library
tests against that library in a subprocess -- the reference's file bodies, random input against the oracle at every
key-word boundary, `count --bc` on tables of three- and four-word keys (one of which doubles with the filter attached), and
the refusals.  Left to the GPU run: the one-pass filter and the command line (the GPU module's parts 4 and 6), and
`count --bc` on a table of 128-mers, whose smallest geometry is 2^31 slots of 32 bytes -- more than the emulation
allocates."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "host", "_build")

T = "tests/test_gpu_bloom_nword.py::"
SELECTION = [T + "test_nword_bloom_bytes_identical_to_reference[bc_k100C]",
             T + "test_nword_bloom_bytes_identical_to_reference[bc_k65]"] + \
            [T + "test_nword_bloom_against_oracle_on_random_input[%d-%s-%s]" % (k, c, m)
             for k in (65, 96, 97, 128) for c in ("C", "fw") for m in ("opt_m", "m1009")] + \
            [T + "test_count_bc_on_nword_tables[%s]" % i for i in ("65", "65-grows", "100")] + \
            [T + "test_routing_refuses_an_nword_table_with_a_filter[65]",
             T + "test_routing_refuses_an_nword_table_with_a_filter[100]",
             T + "test_mer_length_129_is_refused"]


@pytest.fixture(scope="module")
def emu_lib():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    subprocess.check_call([os.path.join(ROOT, "tests", "host", "build_emu.sh")])
    lib = os.path.join(BUILD, "libjfgpu_emu.so")
    assert os.path.exists(lib)
    return lib


def test_nword_bloom_on_the_host_emulation(emu_lib):
    env = dict(os.environ, JFGPU_LIB=emu_lib, JFGPU_CLI=os.path.join(BUILD, "jellyfish-amd-emu"), JFGPU_EMU_THREADS="4")
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider"] + SELECTION,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "%d passed" % len(SELECTION) in r.stdout and "failed" not in r.stdout
