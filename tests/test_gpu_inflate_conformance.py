"""Inflate conformance: deflate streams written by hand (tests/deflate_fixtures.py), judged by zlib's decoder.

bgzf_inflate_kernel (kernels_bgzf.hip.hpp) must return exactly zlib's bytes for every stream zlib accepts and
JFGPU_E_CORRUPT for every stream zlib refuses -- whatever encoder wrote it.  -m gpu only; the whole module also runs on
the host emulation in the CPU suite (tests/test_inflate_conformance_emu.py).

  * directed cases: every header encoding, Huffman set, match, block and framing edge named in deflate_fixtures.DIRECTED,
    each alone (a member that is the last bytes of its upload) and the accepted ones again in one call
  * CRC lane split: payloads of 0..200, 4095..4097 and 65472..65536 bytes as stored, fixed and dynamic members
  * generated streams: seeded random valid streams, hundreds per call, and the same streams damaged in one place

A refused member goes alone, so that the block the engine reports is the crafted one, and after every refusal the same
Parser inflates a good file.  Expected bytes and verdicts come from zlib, never from the engine.
"""
import zlib

import pytest

import deflate_fixtures as DF
import sam_fixtures as F

pytestmark = pytest.mark.gpu

BATCH = 200                                        # accept-class members per inflate call

GOOD_DATA = b"a good member after a refused one; " * 40
GOOD = F.bgzf(GOOD_DATA, block_size=500, variants=("default", "fixed", "stored"))


@pytest.fixture(scope="module")
def engine(gpu):
    p = gpu.Parser(21)
    yield gpu, p
    p.close()


def table(capi, rows):
    t = (capi.BgzfBlock * len(rows))()
    for i, (c_off, u_off, c_len, isize, crc) in enumerate(rows):
        t[i].c_off, t[i].u_off, t[i].c_len, t[i].isize, t[i].crc32 = c_off, u_off, c_len, isize, crc
    return t


def inflate_all(capi, p, cases, eof=False):
    """The members in one call -> the bytes of each.  Where every member fits BGZF, the engine's own scan must find the
    same table."""
    upload, rows = DF.layout(cases, eof)
    if all(c.fits_bgzf() for c in cases):
        blocks, used = capi.bgzf_scan(upload)
        assert used == len(upload)
        assert [(b.c_off, b.u_off, b.c_len, b.isize, b.crc32) for b in blocks][:len(rows)] == rows
    n = p.inflate_table(upload, table(capi, rows))
    data = p.stream_read(0, n)
    p.stream_consume(n)
    assert n == sum(c.isize for c in cases)
    return [data[u_off:u_off + isize] for _, u_off, _, isize, _ in rows]


def expect_accept(capi, p, cases, eof=False):
    got = inflate_all(capi, p, cases, eof)
    wrong = [c.name for c, g in zip(cases, got) if g != c.want]
    assert not wrong, "inflated bytes differ from zlib's: %s" % wrong[:20]


def expect_refuse(capi, p, c):
    assert c.want is None
    upload, rows = DF.layout([c])
    try:
        if c.isize > 65536:                                      # more than a member may hold: the scan says so
            n = p.inflate(upload)
        else:
            n = p.inflate_table(upload, table(capi, rows))
    except capi.JfgpuError as e:
        assert e.code == capi.E_CORRUPT, (c.name, e.msg)
    else:
        p.stream_consume(n)                                      # (leave the parser clean for the tests that follow)
        pytest.fail("%s: the engine inflated a member the reference refuses" % c.name)
    n = p.inflate(GOOD)                                          # the parser still works
    assert p.stream_read(0, n) == GOOD_DATA
    p.stream_consume(n)


def explain(capi, p, c):
    """For the failure message of an accept-class case: what the engine said."""
    upload, rows = DF.layout([c])
    try:
        n = p.inflate_table(upload, table(capi, rows))
    except capi.JfgpuError as e:
        return "refused: " + e.msg
    data = p.stream_read(0, n)
    p.stream_consume(n)
    return "ok" if data == c.want else "wrong bytes"


@pytest.mark.parametrize("name", DF.directed_names("accept"))
def test_directed_stream_inflates_to_zlibs_bytes(engine, name):
    capi, p = engine
    c = DF.directed_case(name)
    assert c.want is not None
    said = explain(capi, p, c)                                   # alone: the member is the last bytes of the upload
    assert said == "ok", (name, said)
    expect_accept(capi, p, [c], eof=True)


@pytest.mark.parametrize("name", DF.directed_names("refuse"))
def test_directed_stream_is_refused_as_zlib_refuses_it(engine, name):
    capi, p = engine
    expect_refuse(capi, p, DF.directed_case(name))


def test_directed_accepted_streams_in_one_call(engine):
    capi, p = engine
    cases = [DF.directed_case(n) for n in DF.directed_names("accept")]
    expect_accept(capi, p, cases, eof=True)
    expect_accept(capi, p, cases[::-1])


@pytest.mark.parametrize("kind", DF.CRC_KINDS)
def test_crc_lane_split_sizes(engine, kind):
    capi, p = engine
    cases = [DF.crc_case(size, kind) for size in DF.CRC_SIZES]
    assert [c.isize for c in cases] == DF.CRC_SIZES
    expect_accept(capi, p, cases)


def test_crc_lane_split_all_encodings_in_one_call(engine):
    capi, p = engine
    small = [s for s in DF.CRC_SIZES if s <= 4097]
    cases = [DF.crc_case(size, kind) for size in small for kind in DF.CRC_KINDS]
    expect_accept(capi, p, cases, eof=True)


def test_generated_valid_streams(engine):
    capi, p = engine
    cases = DF.generated_valid(DF.VALID_SEED, DF.VALID_COUNT)          # (every one accepted by zlib: asserted in the fixture)
    assert len(cases) == DF.VALID_COUNT and all(c.want is not None for c in cases)
    for i in range(0, len(cases), BATCH):
        expect_accept(capi, p, cases[i:i + BATCH])


def test_generated_mutated_streams(engine):
    capi, p = engine
    cases = DF.generated_mutated(DF.MUTATED_SEED, DF.MUTATED_COUNT)
    accepted = [c for c in cases if c.want is not None]
    refused = [c for c in cases if c.want is None]
    assert accepted and refused, "the mutated class must hold both verdicts"
    print("mutated streams: %d accepted, %d refused by the reference" % (len(accepted), len(refused)))
    expect_accept(capi, p, accepted)
    for c in refused:
        expect_refuse(capi, p, c)


def test_crc_of_the_trailer_is_checked_for_crafted_members(engine):
    """The harness itself: a crafted member with a false CRC32 must not pass (or nothing above would mean much)."""
    capi, p = engine
    c = DF.directed_case("hlit_257")
    bad = DF.Case(c.name, c.cdata, None, c.crc ^ 0x80, c.isize)
    expect_refuse(capi, p, bad)
    assert zlib.crc32(c.want) & 0xFFFFFFFF == c.crc
