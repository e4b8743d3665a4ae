"""jfgpu_text_* and jfgpu_dump_next_text on the GPU (-m gpu, over capi.Text): binary/sorted records formatted as text
(jellyfish_amd/csrc/kernels_text.hip.hpp, abi_text.inl) against a formatter written here in plain Python -- integer shifts
and str(count), no engine code.  Output bytes are compared whole.

Shapes: every key width (k = 1 .. 128, key bytes a multiple of 8 and not, partial top bytes, every word count), counts of
1, 2, 3, 4, 5 and 8 bytes, every count value at which the number of digits or the conversion path changes, 0 to 5,000
records, windows that are no multiple of a tile, the three layouts (so that tiles start at every offset mod 4), all-A and
all-T keys, dirt above the key's bits, filters that empty single tiles and whole runs of them, format_dev at and one byte
under the needed capacity, a sink that stops the run, and the table's sorted dump as text."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U64 = 2 ** 64 - 1
COLUMN, FASTA = 0, 1
LAYOUTS = [(COLUMN, " "), (COLUMN, "\t"), (FASTA, " ")]
KS = [1, 3, 4, 5, 16, 21, 31, 32, 33, 40, 64, 65, 96, 97, 127, 128]
COUNTER_LENS = [1, 2, 3, 4, 5, 8]
# every value at which the digits or the conversion path (32-bit / 64-bit) change
VALUES = sorted({0, 9, 10, 99, 100, 2 ** 32 - 1, 2 ** 32, U64} | {10 ** j - 1 for j in range(1, 20)} | {10 ** j for j in range(1, 20)})


def py_format(body, k, cl, layout=COLUMN, sep=" ", lower=0, upper=U64):
    """The reference of these tests: dump_main.cc:35-52 restated.  Returns (text, kept)."""
    kb = (2 * k + 7) // 8
    rb = kb + cl
    body = bytes(body)
    assert len(body) % rb == 0
    mask = (1 << (2 * k)) - 1
    out, kept = [], 0
    for o in range(0, len(body), rb):
        key = int.from_bytes(body[o:o + kb], "little") & mask
        v = int.from_bytes(body[o + kb:o + rb], "little")
        if not lower <= v <= upper:
            continue
        mer = "".join("ACGT"[(key >> (2 * (k - 1 - i))) & 3] for i in range(k))
        out.append("%s%s%s\n" % (mer, sep, str(v)) if layout == COLUMN else ">%s\n%s\n" % (str(v), mer))
        kept += 1
    return "".join(out).encode(), kept


def make_body(rng, k, cl, n, values=None):
    """n records: the first two keys all-A and all-T, the rest random; counts go round `values` (those that fit cl bytes) and
    are random after that."""
    kb = (2 * k + 7) // 8
    top = 256 ** cl - 1
    vals = [v for v in (VALUES if values is None else values) if v <= top]
    recs = []
    for i in range(n):
        key = 0 if i == 0 else (1 << (2 * k)) - 1 if i == 1 else rng.getrandbits(2 * k)
        v = vals[i % len(vals)] if i < 2 * len(vals) else rng.randrange(top + 1) >> rng.randrange(8 * cl)
        recs.append(key.to_bytes(kb, "little") + v.to_bytes(cl, "little"))
    return np.frombuffer(b"".join(recs), dtype=np.uint8)


def check(got, want):
    if got != want:
        i = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
        raise AssertionError("%d bytes, expected %d; first difference at byte %d: %r, expected %r"
                             % (len(got), len(want), i, got[max(0, i - 40):i + 40], want[max(0, i - 40):i + 40]))


def run_text(gpu, body, k, cl, layout=COLUMN, sep=" ", **kw):
    with gpu.Text(k, cl, layout=layout, separator=sep, **kw) as x:
        return x.run(body), x.counts(), x.line_max


@pytest.mark.parametrize("k", KS)
def test_every_key_width(gpu, k):
    rng = random.Random(k)
    cl = COUNTER_LENS[KS.index(k) % len(COUNTER_LENS)]
    body = make_body(rng, k, cl, 700)                               # three tiles, the last one short
    for layout, sep in LAYOUTS:
        got, counts, line_max = run_text(gpu, body, k, cl, layout, sep)
        want, kept = py_format(body, k, cl, layout, sep)
        check(got, want)
        assert counts == (1, 700, kept, len(want))
        assert line_max == k + 2 + len(str(256 ** cl - 1)) + (layout == FASTA)


@pytest.mark.parametrize("cl", COUNTER_LENS)
def test_every_counter_len_and_count_value(gpu, cl):
    rng = random.Random(100 + cl)
    for k in (21, 40):
        body = make_body(rng, k, cl, 300)
        for layout, sep in LAYOUTS:
            got, _, _ = run_text(gpu, body, k, cl, layout, sep)
            check(got, py_format(body, k, cl, layout, sep)[0])


def test_line_max_follows_counter_len_and_upper(gpu):
    for cl, digits in zip(range(1, 9), (3, 5, 8, 10, 13, 15, 17, 20)):
        with gpu.Text(21, cl) as x:
            assert x.line_max == 21 + 2 + digits
        with gpu.Text(21, cl, layout=FASTA) as x:
            assert x.line_max == 21 + 3 + digits
    with gpu.Text(21, 8, upper=99) as x:
        assert x.line_max == 21 + 2 + 2
    with gpu.Text(21, 1, upper=10 ** 6) as x:
        assert x.line_max == 21 + 2 + 3


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 5000])
def test_record_counts(gpu, n):
    rng = random.Random(n)
    for k, cl in ((21, 4), (33, 8)):
        body = make_body(rng, k, cl, n)
        for layout, sep in LAYOUTS:
            got, counts, _ = run_text(gpu, body, k, cl, layout, sep)
            want, kept = py_format(body, k, cl, layout, sep)
            check(got, want)
            assert counts == (1 if n else 0, n, kept, len(want))


@pytest.mark.parametrize("window,windows", [(300, 17), (4096, 2), (0, 1)])
def test_windows(gpu, window, windows):
    rng = random.Random(7)
    k, cl, n = 31, 5, 5000
    body = make_body(rng, k, cl, n)
    chunks = []
    with gpu.Text(k, cl, layout=FASTA, window_records=window) as x:
        got = x.run(body, sink=lambda text, nrec: chunks.append((len(text), nrec)) or 0)
        want, kept = py_format(body, k, cl, FASTA)
        check(got, want)
        assert x.counts() == (windows, n, kept, len(want))
        assert len(chunks) == windows and sum(c[0] for c in chunks) == len(want) and sum(c[1] for c in chunks) == n
        ms = x.last_ms()
        assert len(ms) == 4 and all(v >= 0 for v in ms)
        # the same formatter again, on another body: nothing of the first run is left
        body2 = make_body(rng, k, cl, 777)
        check(x.run(body2), py_format(body2, k, cl, FASTA)[0])


@pytest.mark.parametrize("k", [5, 33])
def test_dirty_top_byte(gpu, k):
    rng = random.Random(k)
    cl, kb = 4, (2 * k + 7) // 8
    clean = make_body(rng, k, cl, 600)
    dirty = clean.copy().reshape(-1, kb + cl)
    dirty[:, kb - 1] |= np.uint8((0xFF << (2 * k - 8 * (kb - 1))) & 0xFF)      # every bit of the top key byte above 2k
    assert (dirty != clean.reshape(-1, kb + cl)).any()
    for layout, sep in LAYOUTS:
        want = py_format(clean, k, cl, layout, sep)[0]
        check(run_text(gpu, clean, k, cl, layout, sep)[0], want)
        check(run_text(gpu, dirty.reshape(-1), k, cl, layout, sep)[0], want)


def test_filters(gpu):
    rng = random.Random(9)
    k, cl, kb = 21, 4, 6
    # six tiles; tiles 2 to 4 hold counts of 1000 and more, the others below 1000; odd records are 7 everywhere else
    recs = []
    for i in range(6 * 256 - 40):
        tile = i // 256
        v = rng.randrange(1000, 2 ** 32) if 1 <= tile <= 3 else (7 if i & 1 else rng.randrange(8, 1000))
        recs.append(rng.getrandbits(2 * k).to_bytes(kb, "little") + v.to_bytes(cl, "little"))
    body = np.frombuffer(b"".join(recs), dtype=np.uint8)
    n = len(recs)
    for lower, upper in ((0, U64),                # everything
                         (2 ** 33, U64),          # nothing
                         (8, U64),                # every other record of tiles 1, 5 and 6, all of 2 to 4
                         (0, 999),                # tiles 2 to 4 keep nothing: zero-length blocks in the middle of the scan
                         (7, 7)):
        for layout, sep in LAYOUTS:
            chunks = []
            with gpu.Text(k, cl, layout=layout, separator=sep, lower=lower, upper=upper) as x:
                got = x.run(body, sink=lambda text, nrec: chunks.append(len(text)) or 0)
                want, kept = py_format(body, k, cl, layout, sep, lower, upper)
                check(got, want)
                assert x.counts() == (1, n, kept, len(want))
            if lower == 2 ** 33:
                assert want == b"" and chunks == []                 # the sink gets no bytes
            else:
                assert 0 < kept < n or (lower, upper) == (0, U64)


def test_format_dev_capacity(gpu):
    rng = random.Random(13)
    k, cl, n, guard = 40, 8, 1000, 64
    body = make_body(rng, k, cl, n)
    want, kept = py_format(body, k, cl, COLUMN, "\t")
    need = len(want)
    with gpu.Table(21, 1 << 13) as t, gpu.Text(k, cl, separator="\t") as x:     # (the table lends its device allocator)
        d_rec, d_txt = t.malloc(len(body) + 64), t.malloc(need + guard + 8)
        try:
            t.h2d(d_rec, body)
            for shift in (0, 1, 2, 3):                             # the text at every alignment
                t.h2d(d_txt, np.full(need + guard + 8, 0xA5, dtype=np.uint8))
                assert x.format_dev(d_rec, n, d_txt + shift, need) == (need, kept)
                out = t.d2h(d_txt, need + guard + 8).tobytes()
                check(out[shift:shift + need], want)
                assert out[:shift] == b"\xA5" * shift and out[shift + need:] == b"\xA5" * (guard + 8 - shift)
            # one byte short: an error, nothing written anywhere, and the formatter still works
            t.h2d(d_txt, np.full(need + guard + 8, 0xA5, dtype=np.uint8))
            with pytest.raises(gpu.JfgpuError) as e:
                x.format_dev(d_rec, n, d_txt, need - 1)
            assert e.value.code == gpu.E_INVALID and str(need) in e.value.msg
            assert t.d2h(d_txt, need + guard + 8).tobytes() == b"\xA5" * (need + guard + 8)
            assert x.format_dev(d_rec, n, d_txt, need) == (need, kept)
            check(t.d2h(d_txt, need).tobytes(), want)
            assert x.format_dev(d_rec, 0, d_txt, 0) == (0, 0)
            with pytest.raises(gpu.JfgpuError):                    # records off a 16-byte boundary are refused
                x.format_dev(d_rec + 8, 10, d_txt, need)
        finally:
            t.free(d_rec)
            t.free(d_txt)


def test_sink_failure(gpu):
    rng = random.Random(17)
    k, cl = 21, 4
    body = make_body(rng, k, cl, 2000)
    want = py_format(body, k, cl)[0]
    with gpu.Text(k, cl, window_records=500) as x:
        seen = []

        def stop_at_second(text, nrec):
            seen.append(nrec)
            return 1 if len(seen) == 2 else 0

        with pytest.raises(gpu.JfgpuError) as e:
            x.run(body, sink=stop_at_second)
        assert "sink" in e.value.msg and len(seen) == 2
        check(x.run(body), want)
        assert x.counts()[0] == 4


def test_bad_parameters_are_refused(gpu):
    for kw in (dict(k=0, counter_len=4), dict(k=129, counter_len=4), dict(k=21, counter_len=0), dict(k=21, counter_len=9),
               dict(k=21, counter_len=4, layout=2), dict(k=21, counter_len=4, separator=",")):
        with pytest.raises(gpu.JfgpuError):
            gpu.Text(**kw)


@pytest.mark.parametrize("k,ocl", [(21, 4), (21, 8), (40, 4), (40, 8), (100, 4), (100, 8)])
def test_dump_next_text(gpu, k, ocl):
    rng = random.Random(k + ocl)
    n, kw = 12000, (2 * k + 63) // 64                              # more than a tile of the table holds: several chunks
    keys = {rng.getrandbits(2 * k) for _ in range(n)}
    keys = np.array([[(x >> (64 * w)) & U64 for w in range(kw)] for x in sorted(keys)], dtype=np.uint64)
    top = 256 ** ocl - 1
    vals = np.array([VALUES[i % len(VALUES)] if VALUES[i % len(VALUES)] not in (0,) and VALUES[i % len(VALUES)] <= top else 1 + i for i in range(len(keys))],
                    dtype=np.uint64)
    with gpu.Table(k, 1 << 15, canonical=False, out_counter_len=ocl) as t:
        t.add_key_vals(keys, vals)
        t.sync()
        recs = t.dump_records()
        assert len(recs) == len(keys)
        tile = t.info.tile_slots
        for layout, sep in ((COLUMN, " "), (FASTA, " ")):
            want = py_format(recs.reshape(-1), k, ocl, layout, sep)[0]
            with gpu.Text(k, ocl, layout=layout, separator=sep) as x:
                for cap in (tile * x.line_max, len(recs) * x.line_max + tile * x.line_max):
                    total, _ = t.dump_begin()
                    assert total == len(recs)
                    got, nrec, calls = [], 0, 0
                    try:
                        while True:
                            nr, text = t.dump_next_text(x, cap)
                            if nr == 0:
                                assert text == b""
                                break
                            got.append(text)
                            nrec += nr
                            calls += 1
                    finally:
                        t.dump_end()
                    check(b"".join(got), want)
                    assert nrec == len(recs)
                    assert calls == 1 if cap > tile * x.line_max else calls > 1
                # a buffer that cannot hold one tile is refused, and the dump goes on after that
                t.dump_begin()
                try:
                    with pytest.raises(gpu.JfgpuError) as e:
                        t.dump_next_text(x, tile * x.line_max - 1)
                    assert e.value.code == gpu.E_INVALID
                    assert t.dump_next_text(x, len(recs) * x.line_max + tile * x.line_max)[1] == want
                finally:
                    t.dump_end()
        # a formatter of another k or counter_len is refused
        for bad in (dict(k=k + 1, counter_len=ocl) if k < 128 else dict(k=k - 1, counter_len=ocl), dict(k=k, counter_len=ocl - 1)):
            with gpu.Text(**bad) as x:
                t.dump_begin()
                try:
                    with pytest.raises(gpu.JfgpuError) as e:
                        t.dump_next_text(x, 1 << 24)
                    assert e.value.code == gpu.E_INVALID
                finally:
                    t.dump_end()
