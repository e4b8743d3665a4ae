"""CPU run of the inflate conformance tests (not -m gpu): all of tests/test_gpu_inflate_conformance.py executed against
the host-emulated library (tests/host/build_emu.sh), in the way of tests/test_sam_emu.py, and the checks of the fixtures
themselves, which need no engine: every directed case has the zlib verdict it is built for, the valid generator is
never refused by zlib, and the mutated class holds both verdicts.  A logic check of the kernel's source on every CPU
test run; the GPU run shows the same on the device."""
import os
import re
import shutil
import subprocess
import sys

import pytest

import deflate_fixtures as DF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "host", "_build")
MODULE = "tests/test_gpu_inflate_conformance.py"


@pytest.fixture(scope="module")
def emu_lib():
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    subprocess.check_call([os.path.join(ROOT, "tests", "host", "build_emu.sh")])
    lib = os.path.join(BUILD, "libjfgpu_emu.so")
    assert os.path.exists(lib)
    return lib


def test_every_directed_case_has_the_verdict_it_names():
    assert len(DF.DIRECTED) > 150
    for name in sorted(DF.DIRECTED):
        c = DF.directed_case(name)                               # (asserts zlib's verdict, and zlib's bytes where it accepts)
        assert c.verdict == DF.DIRECTED[name][0], name
        assert (c.want is None) == (c.verdict == "refuse")
        assert c.isize <= 65536 or c.fits_bgzf(), name           # such a member must be reachable through the scan
    # the writer against zlib's own reader, both ways
    for size in (0, 1, 63, 64, 65, 4096, 65536):
        for kind in DF.CRC_KINDS:
            assert len(DF.crc_case(size, kind).want) == size


def test_the_valid_generator_is_never_refused_by_zlib():
    cases = DF.generated_valid(DF.VALID_SEED, DF.VALID_COUNT)      # raises on the first stream zlib refuses or reads otherwise
    assert len(cases) == DF.VALID_COUNT and all(c.want is not None for c in cases)
    sizes = [c.isize for c in cases]
    assert min(sizes) == 0 and max(sizes) == 65536


def test_the_mutated_class_holds_both_verdicts():
    cases = DF.generated_mutated(DF.MUTATED_SEED, DF.MUTATED_COUNT)
    verdicts = [c.verdict for c in cases]
    assert verdicts.count("accept") >= 1 and verdicts.count("refuse") >= 1
    assert any(c.want is not None and c.name.endswith("token") for c in cases)


def test_inflate_conformance_passes_on_the_host_emulation(emu_lib):
    env = dict(os.environ, JFGPU_LIB=emu_lib, JFGPU_CLI=os.path.join(BUILD, "jellyfish-amd-emu"), JFGPU_EMU_THREADS="4")
    base = [sys.executable, "-m", "pytest", "-m", "gpu", "-q", "-p", "no:cacheprovider", MODULE]
    r = subprocess.run(base + ["--collect-only"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    collected = sum(1 for line in r.stdout.splitlines() if line.startswith(MODULE + "::"))
    assert collected >= len(DF.DIRECTED) + 6, r.stdout[-2000:]
    r = subprocess.run(base, cwd=ROOT, env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stdout[-8000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) passed", r.stdout)
    assert m and int(m.group(1)) == collected and "failed" not in r.stdout and "skipped" not in r.stdout, r.stdout[-2000:]
