"""CPU run of the bgzip-compressed FASTA / FASTQ input (not -m gpu): tests/test_gpu_stream_cut.py, tests/test_gpu_bgzf_seq.py
and tests/test_cli_bgzf_gpu.py executed against the host-emulated library and CLI (tests/host/build_emu.sh), in the same way
as tests/test_sam_emu.py.  A logic check of the device sources -- the cut kernel, the stream entry points, the feed -- on
every CPU test run; races, memory ordering and speed are the GPU run's to show.  The two-rank case is left to the GPU."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "host", "_build")

MODULES = {
    "tests/test_gpu_stream_cut.py": [],
    "tests/test_gpu_bgzf_seq.py": [],
    "tests/test_cli_bgzf_gpu.py": ["--deselect", "tests/test_cli_bgzf_gpu.py::test_compressed_files_on_two_ranks"],
}


@pytest.fixture(scope="module")
def emu_lib():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    subprocess.check_call([os.path.join(ROOT, "tests", "host", "build_emu.sh")])
    lib = os.path.join(BUILD, "libjfgpu_emu.so")
    assert os.path.exists(lib)
    return lib


@pytest.mark.parametrize("module", sorted(MODULES))
def test_bgzf_sequence_input_passes_its_gpu_tests_on_the_host_emulation(emu_lib, module):
    env = dict(os.environ, JFGPU_LIB=emu_lib, JFGPU_CLI=os.path.join(BUILD, "jellyfish-amd-emu"), JFGPU_EMU_THREADS="4")
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider", module] + MODULES[module],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "failed" not in r.stdout and "skipped" not in r.stdout
