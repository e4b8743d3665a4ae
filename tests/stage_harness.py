"""Python side of tests/kernels/stage_harness.hip: the library that is the engine plus entry points launching ONE stage
of the partitioned insert path (P1, P2, T; the sort-based P2 and the two-word path's P1w and Tw; the partitioned Bloom
insert's P1b, P2 with the Bloom functors, Tb and its direct kernel) with the caller's arguments.  Test infrastructure, used by tests/test_gpu_stage_*.py only.  Items of 16 bytes are Python ints here and pairs
of 64-bit words, low word first, at the C boundary (to_words / from_words).

The library is a superset of the engine, so it gets a ctypes binding of its own: a private copy of jellyfish_amd.capi bound
to it (`Harness.capi`).  A table made there is what the stage launches take and what lookup / dump_records / stats /
digest read back.  A handle of one library never goes to the other.

JFKT_LIB names a library built elsewhere (tests/test_stage_kernels_emu.py: the host emulation); without it the device
build is made, or found up to date, by `make kernel-harness`."""
import ctypes as C
import importlib.util
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P = C.c_void_p
HOLE = 0xFFFFFFFF

CONSTS = ["kPBlock", "kP2StragPerBlock", "kStragPerBlock", "kGran", "kRingSlots", "kRingUnit", "kTileBlock", "kTileRound4",
          "kTileRound8", "kMaxTileBits", "kBucketBits", "kPTilePos", "kG2Blocks", "kTileQueueBytes"]
GEOM = ["lsize_l", "tile_bits", "rem_bits", "tag_bits", "cnt_bits", "slot32", "hash_xs", "nbytes", "returning", "part_ok", "b1", "b2",
        "rest_shift", "item32", "lsize_g", "canonical", "tag_full", "key_bits"]
HOLE128 = (1 << 128) - 1
M64 = (1 << 64) - 1

_SIGNATURES = {
    "jfkt_const": (C.c_uint64, [C.c_int]),
    "jfkt_geom": (C.c_int, [_P, _P, C.c_uint32]),
    "jfkt_p2": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P,
                          C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, _P, C.c_uint64, _P, _P, _P, C.c_char_p, C.c_size_t]),
    "jfkt_tile": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint32, _P, C.c_uint64, _P, C.c_uint64, C.c_uint32, C.c_uint64,
                            C.c_uint32, C.c_uint32, C.c_char_p, C.c_size_t]),
    "jfkt_p1": (C.c_int, [_P, C.c_int, C.c_uint32, _P, C.c_uint64, C.c_int64, C.c_int64, C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P, _P,
                          C.c_uint64, _P, _P, C.c_char_p, C.c_size_t]),
    "jfkt_p2_sort": (C.c_int, [_P, C.c_int, C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P,
                               C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _P, C.c_uint64, _P, _P, C.c_uint32, C.c_uint32, _P, _P,
                               _P, C.c_uint64, _P, _P, C.c_char_p, C.c_size_t]),
    "jfkt_p1_wide": (C.c_int, [_P, C.c_uint32, _P, C.c_uint64, C.c_int64, C.c_int64, C.c_uint32, C.c_uint32, _P, _P, _P, _P, C.c_char_p, C.c_size_t]),
    "jfkt_tile_wide": (C.c_int, [_P, C.c_int, C.c_uint32, _P, _P, _P, _P, _P, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, C.c_char_p, C.c_size_t]),
    "jfkt_bloom_const": (C.c_uint64, [C.c_int]),
    "jfkt_bloom_p1": (C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, _P, C.c_uint64, C.c_int64, C.c_int64, C.c_uint32, C.c_uint32,
                                C.c_int, _P, _P, _P, _P, _P, _P, C.c_char_p, C.c_size_t]),
    "jfkt_bloom_seg": (C.c_int, [_P, C.c_uint32, _P, _P, _P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32, C.c_char_p, C.c_size_t]),
    "jfkt_bloom_items_direct": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint32, _P, C.c_uint64, _P, C.c_uint64, C.c_uint64, C.c_uint32, C.c_char_p, C.c_size_t]),
    "jfkt_bloom_p2": (C.c_int, [_P, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _P, _P, _P, _P, _P, C.c_uint32, C.c_uint32, C.c_uint32,
                                _P, _P, _P, _P, _P, C.c_char_p, C.c_size_t]),
}
BLOOM_CONSTS = ["kBloomSegBits", "kBloomItemLow", "kBloomPer", "kBloomRingBytes", "kP2PairPer", "kGranMaxB"]


def to_words(items, item_bytes):
    """items (Python ints or an array) as the array that crosses the C boundary: uint32 / uint64, or (n, 2) uint64 low word first"""
    if item_bytes == 16 and isinstance(items, np.ndarray) and items.ndim == 2:
        return np.ascontiguousarray(items, dtype=np.uint64)
    if item_bytes == 16:
        a = np.empty((len(items), 2), dtype=np.uint64)
        if len(items):
            a[:, 0] = [int(x) & M64 for x in items]
            a[:, 1] = [int(x) >> 64 for x in items]
        return a
    return np.ascontiguousarray(items, dtype=np.uint32 if item_bytes == 4 else np.uint64)


def from_words(a, item_bytes):
    """the inverse: a list of Python ints"""
    if item_bytes == 16:
        a = np.asarray(a, dtype=np.uint64).reshape(-1, 2)
        return [(int(h) << 64) | int(l) for l, h in zip(a[:, 0].tolist(), a[:, 1].tolist())]
    return np.asarray(a).tolist()


class Harness:
    def __init__(self, path):
        from jellyfish_amd import capi as product
        spec = importlib.util.spec_from_file_location("jellyfish_amd_capi_stage_harness", product.__file__)
        self.capi = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(self.capi)
        self.capi.LIB_PATH = path
        self.lib = self.capi.load()
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(self.lib, name)
            fn.restype, fn.argtypes = res, args
        self.const = {n: int(self.lib.jfkt_const(i)) for i, n in enumerate(CONSTS)}
        self.const.update({n: int(self.lib.jfkt_bloom_const(i)) for i, n in enumerate(BLOOM_CONSTS)})

    def geom(self, table):
        out = np.zeros(len(GEOM), dtype=np.uint64)
        self.capi._check(self.lib.jfkt_geom(table._h, out.ctypes.data, len(GEOM)))
        return {n: int(v) for n, v in zip(GEOM, out)}

    def p2(self, table, kernel, nv, pd, b2e, tag_bits, segs, cap, bucket0, nbk, out, rec_cap=1 << 16):
        """segs: [(items uint32[], off uint64[], sh)]; out: uint32[n_dest * cap], pre-filled by the caller (not modified: the
        result is a copy).  kernel: 'roles' or 'shared'."""
        keep = [(np.ascontiguousarray(i, dtype=np.uint32), np.ascontiguousarray(o, dtype=np.uint64), int(s)) for i, o, s in segs]
        n = len(keep)
        items = (_P * n)(*[i.ctypes.data for i, _, _ in keep])
        offs = (_P * n)(*[o.ctypes.data for _, o, _ in keep])
        n_items = np.array([len(i) for i, _, _ in keep], dtype=np.uint64)
        n_off = np.array([len(o) for _, o, _ in keep], dtype=np.uint64)
        sh = np.array([s for _, _, s in keep], dtype=np.uint32)
        assert len(out) % cap == 0
        n_dest = len(out) // cap
        res = np.array(out, dtype=np.uint32, copy=True)
        shared = kernel == "shared"
        gcur = np.zeros(2 * n_dest, dtype=np.uint32)
        rec = np.zeros((rec_cap, 3), dtype=np.uint64)
        n_rec, ctr = C.c_uint64(0), C.c_uint64(0)
        strag_n = np.zeros((self.const["kG2Blocks"] if shared else 1) * nbk, dtype=np.uint32)
        name = C.create_string_buffer(256)
        self.capi._check(self.lib.jfkt_p2(table._h, int(shared), nv, pd, b2e, tag_bits, n, items, n_items.ctypes.data, offs, n_off.ctypes.data,
                                          sh.ctypes.data, cap, bucket0, nbk, n_dest, res.ctypes.data, gcur.ctypes.data, rec.ctypes.data, rec_cap,
                                          C.byref(n_rec), C.byref(ctr), strag_n.ctypes.data, name, len(name)))
        return dict(out=res.reshape(n_dest, cap), gcur=gcur[:n_dest], gshort=gcur[n_dest:], rec=rec[:min(n_rec.value, rec_cap)], n_rec=n_rec.value,
                    ctr_direct=ctr.value, strag_n=strag_n, launched=name.value.decode())

    def tile(self, table, items, off, sh, n_units, tpb, heavy=False, sample=False, holes=True, tile0=0, grid=0):
        items = np.ascontiguousarray(items)
        assert items.dtype in (np.uint32, np.uint64)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        name = C.create_string_buffer(256)
        self.capi._check(self.lib.jfkt_tile(table._h, tpb, int(heavy), int(sample), int(holes), items.dtype.itemsize, items.ctypes.data, len(items),
                                            off.ctypes.data, len(off), sh, tile0, n_units, grid, name, len(name)))
        return name.value.decode()

    def p1(self, table, variant, b1, bases, lo, hi, cap, grid, sentinel, rec_cap=1 << 16):
        """bases: bytes of the contract buffer (its start is the 16-byte aligned base); the k-mers of [lo, hi) are taken."""
        buf = np.frombuffer(bytes(bases), dtype=np.uint8)
        nb = 1 << b1
        out = np.full((nb + 1) * cap, sentinel, dtype=np.uint32)
        gcur = np.zeros(2 * nb, dtype=np.uint32)
        tot = np.zeros(nb, dtype=np.uint64)
        strag = np.zeros((grid, self.const["kStragPerBlock"]), dtype=np.uint64)
        strag_n = np.zeros(grid, dtype=np.uint32)
        rec = np.zeros((rec_cap, 3), dtype=np.uint64)
        n_rec, ctr = C.c_uint64(0), np.zeros(2, dtype=np.uint64)
        name = C.create_string_buffer(256)
        self.capi._check(self.lib.jfkt_p1(table._h, variant, b1, buf.ctypes.data, len(buf), lo, hi, cap, grid, out.ctypes.data, gcur.ctypes.data,
                                          tot.ctypes.data, strag.ctypes.data, strag_n.ctypes.data, rec.ctypes.data, rec_cap, C.byref(n_rec),
                                          ctr.ctypes.data, name, len(name)))
        return dict(out=out.reshape(nb + 1, cap), gcur=gcur[:nb], gshort=gcur[nb:], tot=tot, strag=strag, strag_n=strag_n,
                    rec=rec[:min(n_rec.value, rec_cap)], n_rec=n_rec.value, mers=int(ctr[0]), ctr_direct=int(ctr[1]), launched=name.value.decode())

    def _segs(self, segs, item_bytes):
        keep = [(to_words(i, item_bytes), np.ascontiguousarray(o, dtype=np.uint64), int(s)) for i, o, s in segs]
        n = len(keep)
        items = (_P * n)(*[i.ctypes.data for i, _, _ in keep])
        offs = (_P * n)(*[o.ctypes.data for _, o, _ in keep])
        n_items = np.array([len(i) for i, _, _ in keep], dtype=np.uint64)
        n_off = np.array([len(o) for _, o, _ in keep], dtype=np.uint64)
        sh = np.array([s for _, _, s in keep], dtype=np.uint32)
        return keep, n, items, offs, n_items, n_off, sh

    def p2_sort(self, table, scheme, item_bytes, b2e, tag_bits, segs, bucket0, nbk, n_dest, sentinel, cap=0, pair=False, base=None, n_out=0,
                finish_range=None, rec_cap=1 << 17):
        """segs: [(items, off uint64[], sh)], items Python ints (16 bytes) or arrays.  scheme 0: n_dest regions of cap items, filled
        with `sentinel` before the launch; finish_range (d0, nd): granule_finish_range_kernel over it instead of
        granule_finish_kernel.  scheme 1: base[q] where bucket q starts in an output of n_out items.  Items come back as arrays
        (4, 8 bytes) or (n, 2) word arrays (16 bytes: from_words)."""
        keep, n, items, offs, n_items, n_off, sh = self._segs(segs, item_bytes)
        if scheme == 0:
            n_out = n_dest * cap
        if item_bytes == 16:
            out = np.empty((n_out, 2), dtype=np.uint64)
            out[:, 0], out[:, 1] = sentinel & M64, sentinel >> 64
        else:
            out = np.full(n_out, sentinel, dtype=np.uint32 if item_bytes == 4 else np.uint64)
        gcur = np.zeros(2 * n_dest, dtype=np.uint32)
        off2 = np.full(2 * n_dest, M64, dtype=np.uint64)
        goff = np.full(n_dest + 1, M64, dtype=np.uint64)
        base_a = np.ascontiguousarray(base if base is not None else [], dtype=np.uint64)
        rec = np.zeros((rec_cap, 3), dtype=np.uint64)
        n_rec, ctr = C.c_uint64(0), C.c_uint64(0)
        fr = finish_range or (0, 0)
        name = C.create_string_buffer(256)
        self.capi._check(self.lib.jfkt_p2_sort(table._h, scheme, item_bytes, int(pair), b2e, tag_bits, n, items, n_items.ctypes.data, offs, n_off.ctypes.data,
                                               sh.ctypes.data, cap, bucket0, nbk, n_dest, out.ctypes.data, n_out, gcur.ctypes.data, off2.ctypes.data,
                                               fr[0], fr[1], base_a.ctypes.data if len(base_a) else None, goff.ctypes.data,
                                               rec.ctypes.data, rec_cap, C.byref(n_rec), C.byref(ctr), name, len(name)))
        return dict(out=out, gcur=gcur[:n_dest], gshort=gcur[n_dest:], off2=off2.reshape(n_dest, 2), goff=goff, rec=rec[:min(n_rec.value, rec_cap)],
                    n_rec=n_rec.value, ctr_direct=ctr.value, launched=name.value.decode())

    def p1_wide(self, table, b1, bases, lo, hi, cap, grid, sentinel):
        """p1_wide_granule_kernel over bases[lo, hi); out: (2^b1 + 1, cap, 2) words, the last region a guard"""
        buf = np.frombuffer(bytes(bases), dtype=np.uint8)
        nb = 1 << b1
        out = np.empty(((nb + 1) * cap, 2), dtype=np.uint64)
        out[:, 0], out[:, 1] = sentinel & M64, sentinel >> 64
        gcur = np.zeros(2 * nb, dtype=np.uint32)
        tot = np.zeros(nb, dtype=np.uint64)
        ctr = np.zeros(2, dtype=np.uint64)
        name = C.create_string_buffer(256)
        self.capi._check(self.lib.jfkt_p1_wide(table._h, b1, buf.ctypes.data, len(buf), lo, hi, cap, grid, out.ctypes.data, gcur.ctypes.data,
                                               tot.ctypes.data, ctr.ctypes.data, name, len(name)))
        return dict(out=out.reshape(nb + 1, cap, 2), gcur=gcur[:nb], gshort=gcur[nb:], tot=tot, mers=int(ctr[0]), ctr_direct=int(ctr[1]),
                    launched=name.value.decode())

    def tile_wide(self, table, kernel, segs, tile0=0, n_units=0, grid=1, cap=0):
        """kernel: 'plain' (tile_insert_wide_kernel), 'pipe' (tile_insert_wide_pipe_kernel) or 'direct' (items_direct_wide_kernel:
        one granule batch of 2^b1 regions of cap items); segs: [(items as Python ints, off, sh)]"""
        keep, n, items, offs, n_items, n_off, sh = self._segs(segs, 16)
        name = C.create_string_buffer(256)
        self.capi._check(self.lib.jfkt_tile_wide(table._h, {"plain": 0, "pipe": 1, "direct": 2}[kernel], n, items, n_items.ctypes.data, offs,
                                                 n_off.ctypes.data, sh.ctypes.data, tile0, n_units, grid, cap, name, len(name)))
        return name.value.decode()

    # ---- the partitioned Bloom insert: a counter made by self.bloom(), part = (b1, b2); the filter's bytes through load() / read() ----
    def bloom(self, k, m, nh, canonical=True, seed=7):
        """a Bloom counter of THIS library, in mode 1: the engine launches nothing partitioned by itself"""
        b = self.capi.Bloom(k, m, nh, canonical=canonical, seed=seed)
        b.set_mode(1)
        b.n_seg = (b.nb_bytes + 0xFFFF) >> 16
        return b

    def bloom_p1(self, bloom, family, nbt, per, part, bases, lo, hi, cap, grid, sentinel, run_stragglers=False):
        """family: 'granule', 'granule2' or 'ring'; out: (2^b1 + 1, cap), the last region a guard"""
        buf = np.frombuffer(bytes(bases), dtype=np.uint8)
        b1, b2 = part
        nb = 1 << b1
        out = np.full((nb + 1) * cap, sentinel, dtype=np.uint32)
        gcur = np.zeros(2 * nb, dtype=np.uint32)
        tot = np.zeros(nb, dtype=np.uint64)
        strag = np.zeros((grid, self.const["kStragPerBlock"]), dtype=np.uint64)
        strag_n = np.zeros(grid, dtype=np.uint32)
        mers = C.c_uint64(0)
        name = C.create_string_buffer(256)
        self.capi._check(self.lib.jfkt_bloom_p1(bloom._h, {"granule": 0, "granule2": 1, "ring": 2}[family], nbt, per, b1, b2, bloom.n_seg, buf.ctypes.data, len(buf),
                                                lo, hi, cap, grid, int(run_stragglers), out.ctypes.data, gcur.ctypes.data, tot.ctypes.data, strag.ctypes.data,
                                                strag_n.ctypes.data, C.byref(mers), name, len(name)))
        return dict(out=out.reshape(nb + 1, cap), gcur=gcur[:nb], gshort=gcur[nb:], tot=tot, strag=strag, strag_n=strag_n, mers=mers.value,
                    launched=name.value.decode())

    def bloom_seg(self, bloom, segs, n_seg, seg0=0, grid=1):
        """bloom_segment_kernel; segs: [(items uint32[], off uint64[], sh)], one to three"""
        keep, n, items, offs, n_items, n_off, sh = self._segs(segs, 4)
        name = C.create_string_buffer(256)
        self.capi._check(self.lib.jfkt_bloom_seg(bloom._h, n, items, n_items.ctypes.data, offs, n_off.ctypes.data, sh.ctypes.data, n_seg, seg0, grid, name, len(name)))
        return name.value.decode()

    def bloom_items_direct(self, bloom, part, items, off, cap, grid=2):
        items = np.ascontiguousarray(items, dtype=np.uint32)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        name = C.create_string_buffer(256)
        self.capi._check(self.lib.jfkt_bloom_items_direct(bloom._h, part[0], part[1], bloom.n_seg, items.ctypes.data, len(items), off.ctypes.data, len(off), cap, grid,
                                                          name, len(name)))
        return name.value.decode()

    def bloom_p2(self, bloom, kernel, part, segs, cap2, bucket0, nbk, sentinel):
        """kernel: 'granule', 'roles' or 'shared'; out: (2^(b1 + b2), cap2) filled with `sentinel` before the launch"""
        keep, n, items, offs, n_items, n_off, sh = self._segs(segs, 4)
        b1, b2 = part
        n_dest = 1 << (b1 + b2)
        out = np.full(n_dest * cap2, sentinel, dtype=np.uint32)
        gcur = np.zeros(2 * n_dest, dtype=np.uint32)
        off2 = np.full(2 * n_dest, M64, dtype=np.uint64)
        ctr = C.c_uint64(0)
        kern = {"granule": 0, "roles": 1, "shared": 2}[kernel]
        strag_n = np.zeros((1 if kern == 1 else self.const["kG2Blocks"]) * nbk, dtype=np.uint32)
        name = C.create_string_buffer(256)
        self.capi._check(self.lib.jfkt_bloom_p2(bloom._h, kern, b1, b2, bloom.n_seg, n, items, n_items.ctypes.data, offs, n_off.ctypes.data, sh.ctypes.data, cap2,
                                                bucket0, nbk, out.ctypes.data, gcur.ctypes.data, off2.ctypes.data, C.byref(ctr), strag_n.ctypes.data, name, len(name)))
        return dict(out=out.reshape(n_dest, cap2), gcur=gcur[:n_dest], gshort=gcur[n_dest:], off2=off2.reshape(n_dest, 2), ctr_direct=ctr.value, strag_n=strag_n,
                    launched=name.value.decode())


_harness = None


def load():
    """The harness library, built (or found up to date) by the Makefile unless JFKT_LIB names one.  One per process."""
    global _harness
    if _harness is None:
        path = os.environ.get("JFKT_LIB")
        if not path:
            subprocess.check_call(["make", "-s", "kernel-harness"], cwd=ROOT)
            path = os.path.join(ROOT, "tests", "kernels", "_build", "libjfgpu_kt.so")
        assert os.path.exists(path), path + " is missing"
        _harness = Harness(path)
    return _harness
