"""The serial models and the corpus of tests/parse_fixtures.py against the oracle's restatement of the reference's reader,
and the host reader (jellyfish_amd/include/jellyfish_amd/sequence_parser.hpp, the fallback for every chunk the device
refuses) against both.  CPU only.

The oracle restates the reference's GENERAL reader, which takes more than the device's strict four-line FASTQ layout.  The
layouts in GENERAL_READER_TAKES are refused by the device and read by the reference; for those the expected buffer is
written out here, from mer_overlap_sequence_parser's rules, and the oracle and the host reader must both give it:
  * sequence lines are gathered up to a line that starts with '+', so a wrapped sequence, and a record without a '+'
    line, are sequence (read_sequence);
  * blank lines are skipped wherever a line may start (skip_newlines);
  * the quality is skipped with istream::ignore(|sequence| - seen + 1, line end): it takes one byte more than the
    sequence has when no line end comes first, so a quality line one byte too long passes (skip_quals);
  * an input that ends after a header or inside the sequence lines just ends (read_fastq's loop); one that ends after
    the '+' line has no quality and is refused.
Every other `refuse` case must raise in the oracle, as an input the device refuses for a reason the reference shares."""
import os
import subprocess

import pytest

import oracle_lib as O
import parse_fixtures as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = F.cases()

GENERAL_READER_TAKES = {
    "fastq-refused-0": b"ACGTACGT",                 # wrapped sequence, wrapped quality
    "fastq-refused-2": b"ACGTNAC",                  # blank line between records
    "fastq-refused-3": b"ACGTNAC",                  # the input ends inside the second record's sequence
    "fastq-refused-4": b"ACGT-IIII",                # no '+' line: everything is sequence
    "fastq-quality-one-longer": b"ACGTNGG",
    "fastq-quality-one-longer-last": b"GGNACGT",
    "fastq-4n+1-lines": b"ACGTN",
    "fastq-4n+1-lines-no-newline": b"ACGTN",
    "fastq-4n+2-lines": b"ACGTNAC",
}


def model(fmt, data):
    return F.model_fasta(data) if fmt == "fa" else F.model_fastq(data)


def param(cases):
    return pytest.mark.parametrize("case", cases, ids=[c[0] for c in cases])


def test_corpus_has_every_family_and_every_expectation():
    assert {F.family(c[0]) for c in CASES} == {"seam", "header", "cr", "span", "fastq", "short_lines"}
    assert {c[3] for c in CASES} == {"accept", "refuse", "short_lines"}
    for cid, fmt, data, expect in CASES:
        assert (model(fmt, data) == F.REFUSE) == (expect == "refuse"), cid
    over = [c[2].count(b"\n") - F.short_lines_limit(c[2]) for c in CASES if c[3] == "short_lines"]
    assert {-1, 0, 1} <= set(over) and max(over) == 1


def test_models_on_literals():
    """The rules, spelled out once by hand."""
    assert F.model_fasta(b">a\r\r\nACGT\r\r\n\r\nAC\rGT\nTTTT\r\n\r>b\nGGGG\r") == b"NACGTAC\rGTTTTTNGGGG"
    assert F.model_fasta(b"AC>GT\n\r\r>x>y\nA\r\rC\r") == b"AC>GTNA\r\rC"
    assert F.model_fasta(b"\r\rAC\n") == b"AC" and F.model_fasta(b"\r>h") == b"N" and F.model_fasta(b"A\r>h\n") == b"A\r>h"
    assert F.fasta_model(b">a\n>b\n\n>c\nAC\n")[1] == 3
    assert F.model_fastq(b"@r\nAC\rGT\r\r\n+x\n!III~\r\n", ord('"')) == b"NNC\rGT"
    assert F.model_fastq(b"@r\n\n+\n") == b"N" and F.model_fastq(b"@r\n\n+\n\n") == b"N" and F.model_fastq(b"") == b""
    assert F.model_fastq(b"@r\nAC\n+\nII\n@s\n") is F.REFUSE and F.model_fastq(b"@r\nAC\n+\nI") is F.REFUSE


@param([c for c in CASES if c[3] != "refuse"])
def test_models_equal_the_oracle(case):
    cid, fmt, data, expect = case
    assert model(fmt, data).lstrip(b"N") == O.parse_file(F.oracle_input(fmt, data)).lstrip(b"N")


@param([c for c in CASES if c[3] == "refuse"])
def test_refused_chunks_in_the_oracle(case):
    cid, fmt, data, expect = case
    if cid in GENERAL_READER_TAKES:
        assert O.parse_file(data) == GENERAL_READER_TAKES[cid]
    else:
        with pytest.raises(RuntimeError):
            O.parse_file(data)


def test_general_reader_list_names_corpus_cases():
    ids = {c[0] for c in CASES if c[3] == "refuse"}
    assert set(GENERAL_READER_TAKES) <= ids


@pytest.fixture(scope="module")
def parser_emu(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pemu") / "parser_emu")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "jellyfish_amd", "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "host", "parser_emu.cc")])
    return exe


@param(CASES)
def test_host_reader_on_the_corpus(parser_emu, tmp_path, case):
    """Output equal to the model where the model accepts, refusals exactly where the oracle refuses (and the oracle's
    buffer where the general reader takes what the strict layout does not)."""
    cid, fmt, data, expect = case
    given = F.oracle_input(fmt, data)
    path = tmp_path / "in.txt"
    path.write_bytes(given)
    if expect != "refuse":
        want = model(fmt, data).lstrip(b"N")
    elif cid in GENERAL_READER_TAKES:
        want = GENERAL_READER_TAKES[cid]
    else:
        want = None
    for buf in (64, 4096):
        r = subprocess.run([parser_emu, "21", str(buf), str(path)], capture_output=True)
        if want is None:
            assert r.returncode == 1 and b"Invalid fastq sequence" in r.stderr, buf
        else:
            assert r.returncode == 0, (buf, r.stderr)
            assert r.stdout.lstrip(b"N") == want, buf
