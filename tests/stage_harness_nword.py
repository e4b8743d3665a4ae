"""Python side of tests/kernels/stage_harness_nword.hip: the library that is the engine plus entry points launching ONE stage
of the partitioned insert of three- and four-word keys (P1n, the exact P2 on 256-bit items, Tn and its direct kernel) with
the caller's arguments.  Test infrastructure, used by tests/test_gpu_stage_nword.py only; modelled on tests/stage_harness.py.
Items of 32 bytes are Python ints here and rows of four 64-bit words, lowest first, at the C boundary.

The library is a superset of the engine, so it gets a ctypes binding of its own: a private copy of jellyfish_amd.capi bound
to it (`Harness.capi`).  A handle of one library never goes to another.

JFKTN_LIB names a library built elsewhere (tests/test_nword_part_emu.py: the host emulation); without it the device build is
made, or found up to date, by `make kernel-harness-nword`."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P = C.c_void_p
M64 = (1 << 64) - 1
HOLE256 = (1 << 256) - 1

CONSTS = ["kPBlock", "kGran", "kNChunk", "kNTileBlock", "kP2NWordPer", "kNTileBits", "kPTilePos", "kNLoBits", "item_bytes"]
GEOM = ["lsize_l", "tile_bits", "rem_bits", "tag_bits", "cnt_bits", "nbytes", "returning", "part_ok", "b1", "b2", "rest_shift", "item_bits",
        "lsize_g", "canonical", "tag_full", "key_bits", "max_probe", "item256"]

_SIGNATURES = {
    "jfktn_const": (C.c_uint64, [C.c_int]),
    "jfktn_geom": (C.c_int, [_P, _P, C.c_uint32]),
    "jfktn_p1": (C.c_int, [_P, C.c_uint32, _P, C.c_uint64, C.c_int64, C.c_int64, C.c_uint32, C.c_uint32, _P, _P, _P, _P, C.c_char_p, C.c_size_t]),
    "jfktn_p2": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, C.c_uint64, _P,
                           C.c_char_p, C.c_size_t]),
    "jfktn_tile": (C.c_int, [_P, C.c_int, C.c_uint32, _P, _P, _P, _P, _P, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, _P, C.c_char_p, C.c_size_t]),
}


def to_words(items):
    """Python ints (or an (n, 4) array) as the (n, 4) uint64 array that crosses the C boundary"""
    if isinstance(items, np.ndarray) and items.ndim == 2:
        return np.ascontiguousarray(items, dtype=np.uint64)
    a = np.empty((len(items), 4), dtype=np.uint64)
    for q in range(4):
        a[:, q] = [(int(x) >> (64 * q)) & M64 for x in items]
    return a


def from_words(a):
    a = np.asarray(a, dtype=np.uint64).reshape(-1, 4)
    return [sum(int(w) << (64 * q) for q, w in enumerate(r)) for r in a.tolist()]


class Harness:
    def __init__(self, path):
        from jellyfish_amd import capi as product
        spec = importlib.util.spec_from_file_location("jellyfish_amd_capi_stage_harness_nword", product.__file__)
        self.capi = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(self.capi)
        self.capi.LIB_PATH = path
        self.lib = self.capi.load()
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = res, args
        self.const = {n: int(self.lib.jfktn_const(i)) for i, n in enumerate(CONSTS)}

    def geom(self, table):
        out = np.zeros(len(GEOM), dtype=np.uint64)
        self.capi._check(self.lib.jfktn_geom(table._h, out.ctypes.data, len(GEOM)))
        return {n: int(v) for n, v in zip(GEOM, out)}

    def _segs(self, segs):
        keep = [(to_words(i), np.ascontiguousarray(o, dtype=np.uint64), int(s)) for i, o, s in segs]
        n = len(keep)
        items = (_P * n)(*[i.ctypes.data for i, _, _ in keep])
        offs = (_P * n)(*[o.ctypes.data for _, o, _ in keep])
        n_items = np.array([len(i) for i, _, _ in keep], dtype=np.uint64)
        n_off = np.array([len(o) for _, o, _ in keep], dtype=np.uint64)
        sh = np.array([s for _, _, s in keep], dtype=np.uint32)
        return keep, n, items, offs, n_items, n_off, sh

    def p1(self, table, b1, bases, lo, hi, cap, grid, sentinel):
        """p1_nword_granule_kernel over bases[lo, hi); out: (2^b1 + 1, cap, 4) words, the last region a guard"""
        buf = np.frombuffer(bytes(bases), dtype=np.uint8)
        nb = 1 << b1
        out = np.empty(((nb + 1) * cap, 4), dtype=np.uint64)
        for q in range(4):
            out[:, q] = (sentinel >> (64 * q)) & M64
        gcur = np.zeros(2 * nb, dtype=np.uint32)
        tot = np.zeros(nb, dtype=np.uint64)
        ctr = np.zeros(2, dtype=np.uint64)
        name = C.create_string_buffer(256)
        self.capi._check(self.lib.jfktn_p1(table._h, b1, buf.ctypes.data, len(buf), lo, hi, cap, grid, out.ctypes.data, gcur.ctypes.data,
                                           tot.ctypes.data, ctr.ctypes.data, name, len(name)))
        return dict(out=out.reshape(nb + 1, cap, 4), gcur=gcur[:nb], gshort=gcur[nb:], tot=tot, mers=int(ctr[0]), ctr_direct=int(ctr[1]),
                    launched=name.value.decode())

    def p2(self, table, b2e, tag_bits, segs, bucket0, nbk, n_dest, base, n_out, sentinel):
        """the exact P2; segs: [(items, off, sh)]; returns out as (n_out, 4) words and goff"""
        keep, n, items, offs, n_items, n_off, sh = self._segs(segs)
        out = np.empty((n_out, 4), dtype=np.uint64)
        for q in range(4):
            out[:, q] = (sentinel >> (64 * q)) & M64
        goff = np.full(n_dest + 1, M64, dtype=np.uint64)
        base_a = np.ascontiguousarray(base, dtype=np.uint64)
        name = C.create_string_buffer(256)
        self.capi._check(self.lib.jfktn_p2(table._h, b2e, tag_bits, n, items, n_items.ctypes.data, offs, n_off.ctypes.data, sh.ctypes.data, bucket0, nbk,
                                           n_dest, base_a.ctypes.data, out.ctypes.data, n_out, goff.ctypes.data, name, len(name)))
        return dict(out=out, goff=goff, launched=name.value.decode())

    def tile(self, table, segs, tile0=0, n_units=0, grid=1, kernel="tile", cap=0):
        """kernel 'tile' (tile_insert_nword_kernel) or 'direct' (items_direct_nword_kernel: one granule batch of 2^b1 regions of
        cap items); segs: [(items as Python ints, off, sh)]"""
        keep, n, items, offs, n_items, n_off, sh = self._segs(segs)
        ctr = np.zeros(2, dtype=np.uint64)
        name = C.create_string_buffer(256)
        self.capi._check(self.lib.jfktn_tile(table._h, {"tile": 0, "direct": 1}[kernel], n, items, n_items.ctypes.data, offs, n_off.ctypes.data,
                                             sh.ctypes.data, tile0, n_units, grid, cap, ctr.ctypes.data, name, len(name)))
        return dict(full=int(ctr[0]), ovf_used=int(ctr[1]), launched=name.value.decode())


_harness = None


def load():
    """The harness library, built (or found up to date) by the Makefile unless JFKTN_LIB names one.  One per process."""
    global _harness
    if _harness is None:
        path = os.environ.get("JFKTN_LIB")
        if not path:
            subprocess.check_call(["make", "-s", "kernel-harness-nword"], cwd=ROOT)
            path = os.path.join(ROOT, "tests", "kernels", "_build", "libjfgpu_ktn.so")
        assert os.path.exists(path), path + " is missing"
        _harness = Harness(path)
    return _harness
