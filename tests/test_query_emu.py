"""CPU run of the query tests (not -m gpu): tests/test_gpu_query.py and tests/test_cli_query_gpu.py executed against the
host-emulated engine (tests/host/_build/libjfgpu_emu.so and the CLI linked to it) in a subprocess each -- the logic of
query_ascii_kernel at every key width, the seam of the host form and the CLI's device path and fallback checked on every
CPU test run, without a device.

What this is and is not: see tests/test_emu_kernels.py.  The tables of k = 63, 64 and 128 start at 8, 32 and 64 GB and are
the device's alone: their cases skip themselves here (six of the key-width test, one of the add_key_vals test)."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "host", "_build")
MODULES = ["tests/test_gpu_query.py", "tests/test_cli_query_gpu.py"]
SKIPS = {"tests/test_gpu_query.py": 7}


@pytest.fixture(scope="module")
def emu_lib():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    subprocess.check_call([os.path.join(ROOT, "tests", "host", "build_emu.sh")])
    lib, cli = os.path.join(BUILD, "libjfgpu_emu.so"), os.path.join(BUILD, "jellyfish-amd-emu")
    assert os.path.exists(lib) and os.access(cli, os.X_OK)
    return lib, cli


@pytest.mark.parametrize("module", MODULES)
def test_query_tests_pass_on_the_host_emulation(emu_lib, module):
    env = dict(os.environ, JFGPU_LIB=emu_lib[0], JFGPU_CLI=emu_lib[1], JFGPU_EMU_THREADS="4")
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider", "--durations=5", module],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout
    if SKIPS.get(module):
        assert "%d skipped" % SKIPS[module] in r.stdout
    else:
        assert "skipped" not in r.stdout
