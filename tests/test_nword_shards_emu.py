"""CPU run (not -m gpu) of the sharded tables of keys of three and four words: the engine's device sources built against
the host emulation (tests/host/build_emu.sh, as tests/test_emu_kernels.py does), then a selection of
tests/test_gpu_nword_shards.py against that library in a subprocess -- routing by owner, messages in rounds, steps cut into
pieces, shards that grow together and the two passes of `count --if`, at world sizes 2 and 4 over the local transport.
The command-line tests need the inter-process transport, which the emulation does not have: they stay GPU-only."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "host", "_build")

T = "tests/test_gpu_nword_shards.py::"
SELECTION = [
    T + "test_the_parent_refusal_is_gone",
    T + "test_sharded_nword_keys_equal_single_table[65-True-2-None-None]",
    T + "test_sharded_nword_keys_equal_single_table[65-True-4-None-None]",
    T + "test_sharded_nword_keys_equal_single_table[100-True-2-None-None]",
    T + "test_sharded_nword_keys_equal_single_table[100-True-4-None-None]",
    T + "test_sharded_nword_keys_equal_single_table[100-True-4-997-None]",
    T + "test_sharded_nword_keys_equal_single_table[65-True-2-None-24000]",
    T + "test_sharded_nword_keys_equal_single_table[100-True-4-None-30000]",
    T + "test_nword_shards_grow_together[100-2]",
    T + "test_prime_and_update_over_nword_shards",
]


@pytest.fixture(scope="module")
def emu_lib():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    subprocess.check_call([os.path.join(ROOT, "tests", "host", "build_emu.sh")])
    lib = os.path.join(BUILD, "libjfgpu_emu.so")
    assert os.path.exists(lib)
    return lib


def test_nword_shards_on_the_host_emulation(emu_lib):
    env = dict(os.environ, JFGPU_LIB=emu_lib, JFGPU_CLI=os.path.join(BUILD, "jellyfish-amd-emu"), JFGPU_EMU_THREADS="4")
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider"] + SELECTION,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "%d passed" % len(SELECTION) in r.stdout and "failed" not in r.stdout
