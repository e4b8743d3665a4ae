"""CPU run of the text tests (not -m gpu): tests/test_gpu_text.py and tests/test_cli_dump_gpu.py executed against the
host-emulated engine (tests/host/_build/libjfgpu_emu.so and the CLI linked to it) in a subprocess each -- the logic of the
length, scan and write kernels at every key width and count value, the host's windows and pipeline, jfgpu_dump_next_text and
the CLI's device path and fallback checked on every CPU test run, without a device.

What this is and is not: see tests/test_emu_kernels.py."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "host", "_build")
MODULES = ["tests/test_gpu_text.py", "tests/test_cli_dump_gpu.py"]


@pytest.fixture(scope="module")
def emu_lib():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    subprocess.check_call([os.path.join(ROOT, "tests", "host", "build_emu.sh")])
    lib, cli = os.path.join(BUILD, "libjfgpu_emu.so"), os.path.join(BUILD, "jellyfish-amd-emu")
    assert os.path.exists(lib) and os.access(cli, os.X_OK)
    return lib, cli


@pytest.mark.parametrize("module", MODULES)
def test_text_tests_pass_on_the_host_emulation(emu_lib, module):
    env = dict(os.environ, JFGPU_LIB=emu_lib[0], JFGPU_CLI=emu_lib[1], JFGPU_EMU_THREADS="4")
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider", "--durations=5", module],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout
