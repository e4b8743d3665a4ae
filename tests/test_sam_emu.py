"""CPU run of `count --sam` (not -m gpu): a selection of tests/test_gpu_sam.py -- the BGZF inflate against zlib, damaged
members, the record-start recovery on files built to defeat its guesses, and the CLI's `count --sam` against `count` of
the same reads as FASTQ -- executed against the host-emulated library and CLI (tests/host/build_emu.sh), in the same
way as tests/test_emu_kernels.py.  A logic check of the device sources on every CPU test run; races, memory ordering
and speed are the GPU run's to show."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "host", "_build")

SELECTION = [
    "tests/test_gpu_sam.py::test_inflate_equals_zlib[default]",
    "tests/test_gpu_sam.py::test_inflate_equals_zlib[stored]",
    "tests/test_gpu_sam.py::test_inflate_equals_zlib[fixed]",
    "tests/test_gpu_sam.py::test_inflate_equals_zlib[huffman]",
    "tests/test_gpu_sam.py::test_damaged_members_are_errors_not_faults",
    "tests/test_gpu_sam.py::test_record_starts_equal_the_serial_walk[1-fake_headers]",
    "tests/test_gpu_sam.py::test_record_starts_equal_the_serial_walk[3-long_read]",
    "tests/test_gpu_sam.py::test_record_starts_equal_the_serial_walk[1-aligned_members]",
    "tests/test_gpu_sam.py::test_record_starts_equal_the_serial_walk[1000-empty_reads]",
    "tests/test_gpu_sam.py::test_record_starts_equal_the_serial_walk[1000-big_header]",
    "tests/test_gpu_sam.py::test_count_sam_equals_count_of_the_same_reads_as_fastq[21-True]",
    "tests/test_gpu_sam.py::test_count_sam_equals_count_of_the_same_reads_as_fastq[100-True]",
    "tests/test_gpu_sam.py::test_quality_mask_missing_qualities_and_odd_bases[qopt0]",
    "tests/test_gpu_sam.py::test_count_sam_with_other_options",
    "tests/test_gpu_sam.py::test_truncated_and_corrupt_bam_are_refused",
    "tests/test_gpu_sam.py::test_cram_and_plain_gzip_are_refused_by_name",
    "tests/test_gpu_sam.py::test_bgzf_with_another_extra_subfield_before_bc",
    "tests/test_gpu_sam.py::test_count_sam_against_the_oracle_counts[21]",
    "tests/test_gpu_sam.py::test_sam_alone_is_enough_input_and_listed_in_help",
]


@pytest.fixture(scope="module")
def emu_lib():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    subprocess.check_call([os.path.join(ROOT, "tests", "host", "build_emu.sh")])
    lib = os.path.join(BUILD, "libjfgpu_emu.so")
    assert os.path.exists(lib)
    return lib


def test_sam_input_passes_its_gpu_tests_on_the_host_emulation(emu_lib):
    env = dict(os.environ, JFGPU_LIB=emu_lib, JFGPU_CLI=os.path.join(BUILD, "jellyfish-amd-emu"), JFGPU_EMU_THREADS="4")
    r = subprocess.run([sys.executable, "-m", "pytest", "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider"] + SELECTION,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "%d passed" % len(SELECTION) in r.stdout and "failed" not in r.stdout
