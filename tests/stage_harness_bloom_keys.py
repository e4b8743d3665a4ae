"""Python side of tests/kernels/stage_harness_bloom_keys.hip: the library that is the engine plus one entry point launching
P1b of the partitioned Bloom insert for keys of two, three and four words (p1_bloom_keys_kernel) ALONE with the caller's
arguments.  Test infrastructure, used by tests/test_gpu_stage_bloom_p1_keys.py only; modelled on tests/stage_harness_nword.py.

The library is a superset of the engine, so it gets a ctypes binding of its own: a private copy of jellyfish_amd.capi bound
to it (`Harness.capi`).  A handle of one library never goes to another.

JFKTBK_LIB names a library built elsewhere (tests/test_bloom_keys_part_emu.py: the host emulation); without it the device
build is made, or found up to date, by `make kernel-harness-bloom-keys`."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P = C.c_void_p
HOLE = 0xFFFFFFFF

CONSTS = ["kPBlock", "kGran", "kPTilePos", "kBloomSegBits", "kBloomItemLow", "kBloomKeysPer", "kGranMaxB"]

_SIGNATURES = {
    "jfktb_const": (C.c_uint64, [C.c_int]),
    "jfktb_p1": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, _P, C.c_uint64, C.c_int64, C.c_int64, C.c_uint32, C.c_uint32, _P, _P, _P, _P,
                           C.c_char_p, C.c_size_t]),
}


class Harness:
    def __init__(self, path):
        from jellyfish_amd import capi as product
        spec = importlib.util.spec_from_file_location("jellyfish_amd_capi_stage_harness_bloom_keys", product.__file__)
        self.capi = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(self.capi)
        self.capi.LIB_PATH = path
        self.lib = self.capi.load()
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = res, args
        self.const = {n: int(self.lib.jfktb_const(i)) for i, n in enumerate(CONSTS)}

    def bloom(self, k, m, nh, canonical=True, seed=7):
        """a Bloom counter of THIS library, in mode 1: the engine launches nothing partitioned by itself"""
        b = self.capi.Bloom(k, m, nh, canonical=canonical, seed=seed)
        b.set_mode(1)
        b.n_seg = (b.nb_bytes + 0xFFFF) >> 16
        return b

    def bloom_p1(self, bloom, part, bases, lo, hi, cap, grid, sentinel):
        """p1_bloom_keys_kernel over bases[lo, hi); out: (2^b1 + 1, cap), the last region a guard"""
        buf = np.frombuffer(bytes(bases), dtype=np.uint8)
        b1, b2 = part
        nb = 1 << b1
        out = np.full((nb + 1) * cap, sentinel, dtype=np.uint32)
        gcur = np.zeros(2 * nb, dtype=np.uint32)
        tot = np.zeros(nb, dtype=np.uint64)
        mers = C.c_uint64(0)
        name = C.create_string_buffer(256)
        self.capi._check(self.lib.jfktb_p1(bloom._h, b1, b2, bloom.n_seg, buf.ctypes.data, len(buf), lo, hi, cap, grid, out.ctypes.data, gcur.ctypes.data,
                                           tot.ctypes.data, C.byref(mers), name, len(name)))
        return dict(out=out.reshape(nb + 1, cap), gcur=gcur[:nb], gshort=gcur[nb:], tot=tot, mers=mers.value, launched=name.value.decode())


_harness = None


def load():
    """The harness library, built (or found up to date) by the Makefile unless JFKTBK_LIB names one.  One per process."""
    global _harness
    if _harness is None:
        path = os.environ.get("JFKTBK_LIB")
        if not path:
            subprocess.check_call(["make", "-s", "kernel-harness-bloom-keys"], cwd=ROOT)
            path = os.path.join(ROOT, "tests", "kernels", "_build", "libjfgpu_ktbk.so")
        assert os.path.exists(path), path + " is missing"
        _harness = Harness(path)
    return _harness
