"""SAM text as input (the reference opens -x with sam_open, which reads BAM and SAM text alike: source/read_chimeric_alignments.cpp:563).

The lines become BAM records through arriba_amd/csrc/device/sam_core.hpp -- on the device (agpu_sam.hip) and, stepped on the host, in ahost_sam_transcode and the host
ingest.  The independent side of the comparisons is tools/bam_to_sam.py (BAM -> text, written from the SAM specification) and records built here with struct."""
import ctypes
import gzip
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

import conftest
import parity
from test_host_and_device_logic import DEVICE_INGEST_DATASETS, _batch_columns, _device_batch_columns, _write_bgzf

sys.path.insert(0, os.path.join(conftest.ROOT, "tools"))
from bam_to_sam import bam_to_sam  # noqa: E402

SAM_DATASETS = ("toy3k", "shuffled2k", "itd6k")
assert all(name in DEVICE_INGEST_DATASETS for name in SAM_DATASETS)


# ---- helpers ------------------------------------------------------------------------------------------------------------------------------------------------

def _targets(names):
    """the @SQ names as agpu_ingest_sam_targets / ahost_sam_transcode take them: the names back to back, offsets [n + 1]"""
    joined = "".join(names).encode()
    offsets = np.zeros(len(names) + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum([len(name) for name in names])
    return ctypes.create_string_buffer(joined, max(len(joined), 1)), offsets


def _transcode(function, leading, text, names):
    """(status, records, n_records, bad_line) of ahost_sam_transcode / agpu_sam_transcode"""
    joined, offsets = _targets(names)
    out = ctypes.create_string_buffer(2 * len(text) + 64)
    out_bytes, n_records, bad_line = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    status = function(*(leading + (text, len(text), ctypes.cast(joined, ctypes.c_void_p), offsets.ctypes.data, len(names), ctypes.cast(out, ctypes.c_void_p), len(out),
                                 ctypes.byref(out_bytes), ctypes.byref(n_records), ctypes.byref(bad_line))))
    assert out_bytes.value <= len(out)
    return status, out.raw[:out_bytes.value], n_records.value, bad_line.value


def _host_transcode(text, names):
    from arriba_amd import _capi
    return _transcode(_capi.host_library().ahost_sam_transcode, (), text, names)


def _records_of_bam(path):
    """the records of a BAM file (everything behind its header), uncompressed"""
    stream = gzip.open(path, "rb").read()
    assert stream[:4] == b"BAM\x01"
    at = 8 + struct.unpack_from("<i", stream, 4)[0]
    n_ref = struct.unpack_from("<i", stream, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", stream, at)[0]
    return stream[at:]


def _without_bins(records):
    """the two `bin` bytes of every record zeroed: the generator of the datasets writes the constant 4680, not reg2bin"""
    masked = bytearray(records)
    at = 0
    while at < len(masked):
        masked[at + 14:at + 16] = b"\0\0"
        at += 4 + struct.unpack_from("<i", masked, at)[0]
    assert at == len(masked)
    return bytes(masked)


@pytest.fixture(scope="module")
def sam_text(dataset_files):
    """name -> (SAM text of the dataset's BAM file with its header lines, reference names); converted once per session by tools/bam_to_sam.py"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = bam_to_sam(open(dataset_files(name) + ".bam", "rb").read())
        return cache[name]
    return get


@pytest.fixture(scope="module")
def text_samples(dataset_files, sam_text, tmp_path_factory):
    """name -> prefix of a directory where PREFIX.bam is the SAM TEXT of the dataset (the format is told by content, not by name), next to links to its .fa, .gtf and rule files"""
    cache = {}

    def get(name):
        if name not in cache:
            prefix = dataset_files(name)
            directory = str(tmp_path_factory.mktemp("text_" + name))
            for entry in os.listdir(os.path.dirname(prefix)):
                if entry.startswith(os.path.basename(prefix) + ".") and not entry.endswith(".bam"):
                    os.symlink(os.path.join(os.path.dirname(prefix), entry), os.path.join(directory, entry))
            mine = os.path.join(directory, os.path.basename(prefix))
            with open(mine + ".bam", "wb") as out:
                out.write(sam_text(name)[0])
            cache[name] = mine
        return cache[name]
    return get


def _reg2bin(beg, end):
    """SAMv1 section 5.3"""
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


CIGAR_CODES = {op: code for code, op in enumerate("MIDNSHP=X")}
BASE_CODES = {base: code for code, base in enumerate("=ACMGRSVTWYHKDBN")}
HAND_NAMES = ["chr1", "chr2", "chrUn_KI270442v1"]


def _record(qname, flag, ref, pos, mapq, cigar, next_ref, next_pos, tlen, seq, qual, aux=b""):
    """the BAM record of SAMv1 section 4.2; pos / next_pos 1-based as in the text, cigar / seq / qual as in the text ('*' = none)"""
    ops = [] if cigar == "*" else [(int(length), op) for length, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]
    reference_length = sum(length for length, op in ops if op in "MDN=X")
    if reference_length == 0 or flag & 4:
        reference_length = 1
    bases = "" if seq == "*" else seq
    codes = [BASE_CODES[base.upper()] for base in bases] + [0]
    packed = bytes(codes[i] << 4 | codes[i + 1] for i in range(0, len(bases), 2))
    qualities = b"\xff" * len(bases) if qual == "*" else bytes(ord(q) - 33 for q in qual)
    body = struct.pack("<iiBBHHHiiii", ref, pos - 1, len(qname) + 1, mapq, _reg2bin(pos - 1, pos - 1 + reference_length), len(ops), flag, len(bases), next_ref, next_pos - 1, tlen)
    body += qname.encode() + b"\0" + b"".join(struct.pack("<I", length << 4 | CIGAR_CODES[op]) for length, op in ops) + packed + qualities + aux
    return struct.pack("<i", len(body)) + body


def _hand_made_cases():
    """[(line of SAM text, its record built with struct)]"""
    cases = []

    def case(fields, record_arguments, tags="", aux=b""):
        cases.append(("\t".join(str(field) for field in fields) + tags, _record(*record_arguments, aux=aux)))
    # '*' in RNAME, CIGAR, SEQ and QUAL; RNEXT '*'; POS 0
    case(["unplaced", 4, "*", 0, 0, "*", "*", 0, 0, "*", "*"], ("unplaced", 4, -1, 0, 0, "*", -1, 0, 0, "*", "*"))
    # RNEXT '='; even l_seq
    case(["pair/1", 99, "chr1", 100, 60, "10M", "=", 200, 110, "ACGTACGTAC", "IIIIIIII#!"], ("pair/1", 99, 0, 100, 60, "10M", 0, 200, 110, "ACGTACGTAC", "IIIIIIII#!"))
    # RNEXT another reference; odd l_seq; lower case and every IUPAC code; QUAL '*'
    case(["iupac", 65, "chr2", 7, 3, "5S12M", "chrUn_KI270442v1", 1, -40, "acgtnMRSVWYHKDB=N", "*"], ("iupac", 65, 1, 7, 3, "5S12M", 2, 1, -40, "acgtnMRSVWYHKDB=N", "*"))
    # a read name of 254 characters; every CIGAR operation
    long_name = "n" * 254
    case([long_name, 0, "chr1", 5, 255, "1M2I3D4N5S6H7P8=9X", "*", 0, 0, "ACGTACGTACGTACGTACGTACGTACGTA", "~" * 29], (long_name, 0, 0, 5, 255, "1M2I3D4N5S6H7P8=9X", -1, 0, 0, "ACGTACGTACGTACGTACGTACGTACGTA", "~" * 29))
    # every type of optional field
    tags = "\tXA:A:c\tXi:i:-5\tXf:f:1.5\tXZ:Z:hello world\tXE:Z:\tXH:H:1AE301\tBc:B:c,-1,2\tBC:B:C,1,255\tBs:B:s,-300,300\tBS:B:S,0,65535\tBi:B:i,-70000,70000\tBI:B:I,0,4294967295\tBf:B:f,0.5,-2,3e2\tBe:B:S"
    aux = (b"XAAc" + b"Xic" + struct.pack("<b", -5) + b"Xff" + struct.pack("<f", 1.5) + b"XZZhello world\0" + b"XEZ\0" + b"XHH1AE301\0" + b"BcBc" + struct.pack("<Ibb", 2, -1, 2) + b"BCBC" + struct.pack("<IBB", 2, 1, 255)
           + b"BsBs" + struct.pack("<Ihh", 2, -300, 300) + b"BSBS" + struct.pack("<IHH", 2, 0, 65535) + b"BiBi" + struct.pack("<Iii", 2, -70000, 70000) + b"BIBI" + struct.pack("<III", 2, 0, 4294967295)
           + b"BfBf" + struct.pack("<Ifff", 3, 0.5, -2.0, 300.0) + b"BeBS" + struct.pack("<I", 0))
    case(["tags", 16, "chr1", 10, 1, "4M", "*", 0, 0, "ACGT", "ABCD"], ("tags", 16, 0, 10, 1, "4M", -1, 0, 0, "ACGT", "ABCD"), tags, aux)
    # an 'i' value takes the smallest type that holds it: each boundary
    tags = "\tI1:i:-129\tI2:i:-128\tI3:i:255\tI4:i:256\tI5:i:65535\tI6:i:65536\tI7:i:-32769\tI8:i:-32768\tI9:i:0"
    aux = (b"I1s" + struct.pack("<h", -129) + b"I2c" + struct.pack("<b", -128) + b"I3C" + struct.pack("<B", 255) + b"I4S" + struct.pack("<H", 256) + b"I5S" + struct.pack("<H", 65535) + b"I6I" + struct.pack("<I", 65536)
           + b"I7i" + struct.pack("<i", -32769) + b"I8s" + struct.pack("<h", -32768) + b"I9C" + struct.pack("<B", 0))
    case(["integers", 0, "chr2", 1, 0, "1M", "*", 0, 0, "A", "*"], ("integers", 0, 1, 1, 0, "1M", -1, 0, 0, "A", "*"), tags, aux)
    # reg2bin on three spans: inside one 16 kb bin, across two of them, across two 128 kb bins
    for name, pos, cigar in (("bin_smallest", 1, "10M"), ("bin_across_16k", 16380, "50M"), ("bin_across_128k", 131070, "10M200N10M")):
        case([name, 0, "chr1", pos, 9, cigar, "*", 0, 0, "*", "*"], (name, 0, 0, pos, 9, cigar, -1, 0, 0, "*", "*"))
    assert [struct.unpack_from("<H", record, 14)[0] for _, record in cases[-3:]] == [4681, 585, 73]
    # a read of 3 000 bases: longer than what a wavefront stages
    bases = "".join("ACGTTGCAAN"[(7 * k) % 10] for k in range(3000))
    qualities = "".join(chr(33 + (11 * k) % 60) for k in range(3000))
    case(["long_read", 0, "chr2", 1000, 20, "3000M", "*", 0, 0, bases, qualities], ("long_read", 0, 1, 1000, 20, "3000M", -1, 0, 0, bases, qualities), "\tNM:i:3", b"NMC\x03")
    case(["behind_the_long_read", 0, "chr2", 1001, 20, "3M", "*", 0, 0, "AAC", "ABC"], ("behind_the_long_read", 0, 1, 1001, 20, "3M", -1, 0, 0, "AAC", "ABC"))
    return cases


def _hand_made_texts():
    """{variant: (text, expected records)}: line feeds; carriage return + line feed; a last line without its line feed"""
    cases = _hand_made_cases()
    lines, expected = [line for line, _ in cases], b"".join(record for _, record in cases)
    return {"line feeds": ("\n".join(lines) + "\n", expected), "carriage returns": ("\r\n".join(lines) + "\r\n", expected), "no last line feed": ("\n".join(lines), expected),
            "carriage return at the very end": ("\r\n".join(lines) + "\r", expected)}


GOOD_LINE = "good%d\t0\tchr1\t%d\t60\t4M\t*\t0\t0\tACGT\tIIII\tNH:i:1"
MALFORMED_LINES = {
    "ten fields": "r\t0\tchr1\t1\t60\t4M\t*\t0\t0\tACGT",
    "unknown reference": "r\t0\tchr9\t1\t60\t4M\t*\t0\t0\tACGT\tIIII",
    "unknown mate reference": "r\t0\tchr1\t1\t60\t4M\tchr\t0\t0\tACGT\tIIII",
    "CIGAR operation Q": "r\t0\tchr1\t1\t60\t2M2Q\t*\t0\t0\tACGT\tIIII",
    "CIGAR without a length": "r\t0\tchr1\t1\t60\tM\t*\t0\t0\tACGT\tIIII",
    "SEQ and QUAL differ": "r\t0\tchr1\t1\t60\t4M\t*\t0\t0\tACGT\tIII",
    "FLAG 12x": "r\t12x\tchr1\t1\t60\t4M\t*\t0\t0\tACGT\tIIII",
    "POS empty": "r\t0\tchr1\t\t60\t4M\t*\t0\t0\tACGT\tIIII",
    "MAPQ 256": "r\t0\tchr1\t1\t256\t4M\t*\t0\t0\tACGT\tIIII",
    "empty line": "",
    "header line behind an alignment": "@CO\tlate",
    "optional field of unknown type": "r\t0\tchr1\t1\t60\t4M\t*\t0\t0\tACGT\tIIII\tXX:q:1",
    "optional field cut short": "r\t0\tchr1\t1\t60\t4M\t*\t0\t0\tACGT\tIIII\tXX:",
    "array value out of range": "r\t0\tchr1\t1\t60\t4M\t*\t0\t0\tACGT\tIIII\tXX:B:c,128",
    "line of tabs": "\t" * 10,
}


def _malformed_cases():
    """[(what, text, line number of the malformed line, records of the other lines)]: every malformed line at a place of its own, behind 0-2 header lines"""
    cases = []
    for k, (what, bad) in enumerate(sorted(MALFORMED_LINES.items())):
        header = ["@HD\tVN:1.6", "@SQ\tSN:chr1\tLN:100000"][:k % 3]
        good = [GOOD_LINE % (i, 10 + i) for i in range(5)]
        place = 1 + k % 4  # (never the first alignment: an '@' line there would be a header line)
        lines = good[:place] + [bad] + good[place:]
        if k % 5 == 4:  # a second malformed line further down: the smallest number is reported
            lines.append("r\t0")
        text = "\n".join(header + lines) + ("\n" if k % 2 == 0 or bad == "" else "")
        expected = b"".join(_record("good%d" % i, 0, 0, 10 + i, 60, "4M", -1, 0, 0, "ACGT", "IIII", b"NHC\x01") for i in range(5))
        cases.append((what, text, len(header) + place + 1, expected))
    return cases


def write_malformed_cases(directory):
    """for tools/sanitize_sam.sh: every malformed text as DIRECTORY/<expected line number>_<k>.sam"""
    for k, (what, text, line, _) in enumerate(_malformed_cases()):
        with open(os.path.join(directory, "%d_%d.sam" % (line, k)), "w", newline="") as out:
            out.write(text)


# ---- CPU tier -----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SAM_DATASETS)
def test_text_of_a_bam_file_transcodes_back_to_its_records(name, built, dataset_files, sam_text):
    """BAM -> text by tools/bam_to_sam.py (written from the specification) -> records by sam_core.hpp stepped on the host: the records of the file, byte for byte (bin aside)"""
    text, names = sam_text(name)
    original = _records_of_bam(dataset_files(name) + ".bam")
    status, records, n_records, bad_line = _host_transcode(text, names)
    assert (status, bad_line) == (0, 0)
    assert n_records == text.count(b"\n") - sum(1 for line in text.split(b"\n") if line.startswith(b"@")) and n_records > 4000
    assert len(records) == len(original)
    assert _without_bins(records) == _without_bins(original)


@pytest.mark.parametrize("variant", sorted(_hand_made_texts()))
def test_hand_made_lines_give_the_records_of_the_specification(variant, built):
    text, expected = _hand_made_texts()[variant]
    status, records, n_records, bad_line = _host_transcode(text.encode(), HAND_NAMES)
    assert (status, bad_line, n_records) == (0, 0, len(_hand_made_cases()))
    at = 0
    for line, record in _hand_made_cases():  # (record by record: a difference names its line)
        assert records[at:at + len(record)] == record, line[:60]
        at += len(record)
    assert records == expected


@pytest.mark.parametrize("what,text,line,expected", _malformed_cases(), ids=[case[0] for case in _malformed_cases()])
def test_malformed_lines_are_told_with_their_number(what, text, line, expected, built, monkeypatch):
    """every line is parsed from a heap copy of exactly its size (ARRIBA_SAM_ISOLATE_LINES): under tools/sanitize_sam.sh (AddressSanitizer) a read outside the line is a failure"""
    from arriba_amd import _capi
    monkeypatch.setenv("ARRIBA_SAM_ISOLATE_LINES", "1")
    status, records, n_records, bad_line = _host_transcode(text.encode(), HAND_NAMES)
    assert status != 0 and bad_line == line
    assert re.match(r"failed to load alignments: SAM line %d: \w" % line, _capi.host_library().ahost_last_error().decode())
    assert n_records == 5 and records == expected  # (the other lines are transcoded all the same)


@pytest.mark.parametrize("container", ["plain", "gzip", "bgzf"])
def test_feed_hands_on_whole_lines(container, built, dataset_files, sam_text, tmp_path):
    """ahost_bam_open / ahost_bam_next on text: the header lines are read on the host, every piece is of kind 3, ends on a line end and knows the number of its first line"""
    from arriba_amd import _capi
    from arriba_amd.pipeline import HostSession
    prefix = dataset_files("toy3k")
    text, names = sam_text("toy3k")
    path = str(tmp_path / "toy3k.bam")  # (by content, not by name)
    if container == "plain":
        open(path, "wb").write(text)
    elif container == "gzip":
        with gzip.open(path, "wb") as out:
            out.write(text)
    else:
        _write_bgzf(path, text, 6)
    session = HostSession(prefix + ".fa", prefix + ".gtf")
    lib, handle = session._lib, session._session
    config = _capi.IngestConfig()
    assert lib.ahost_bam_open(handle, path.encode(), 0, 100, ctypes.byref(config)) == 0, lib.ahost_last_error()
    try:
        assert config.n_targets == len(names) and config.first_record_offset == 0
        pointers = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint32()
        assert lib.ahost_bam_sam_targets(handle, ctypes.byref(pointers[0]), ctypes.byref(pointers[1]), ctypes.byref(pointers[2])) == 1
        offsets = np.ctypeslib.as_array(ctypes.cast(pointers[1], ctypes.POINTER(ctypes.c_uint32)), (pointers[2].value + 1,))
        joined = ctypes.string_at(pointers[0], int(offsets[-1])).decode()
        assert [joined[offsets[t]:offsets[t + 1]] for t in range(pointers[2].value)] == names
        header_lines = sum(1 for line in text.split(b"\n") if line.startswith(b"@"))
        body = text[sum(len(line) + 1 for line in text.split(b"\n")[:header_lines]):]
        buffer = ctypes.create_string_buffer(1 << 20)
        piece = _capi.BamPiece()
        pieces, lines_before = [], header_lines
        while True:
            status = lib.ahost_bam_next(handle, buffer, len(buffer), None, 0, ctypes.byref(piece))
            assert status >= 0, lib.ahost_last_error()
            if status == 0:
                break
            assert piece.stored_bgzf == 3 and piece.bytes > 0 and piece.first_line == lines_before + 1
            pieces.append(buffer.raw[:piece.bytes])
            assert pieces[-1].endswith(b"\n")
            lines_before += pieces[-1].count(b"\n")
        assert len(pieces) >= 3 and b"".join(pieces) == body
        # one sample over several GPUs: not from text, and the message says why
        assert lib.ahost_bam_open_part(handle, path.encode(), 0, 100, 0, 2, ctypes.byref(config)) != 0
        assert "SAM text has no record sizes" in lib.ahost_last_error().decode()
    finally:
        lib.ahost_bam_close(handle)


@pytest.mark.parametrize("name", SAM_DATASETS)
def test_host_ingest_reads_text(name, built, dataset_files, sam_text, text_samples):
    """HostSession.read_chimeric_alignments on the text -- a file, and the bytes in memory -- gives the batch of the BAM file"""
    from arriba_amd.pipeline import HostSession
    prefix = dataset_files(name)
    expected = _batch_columns(parity.open_session(prefix))
    for source in (text_samples(name) + ".bam", sam_text(name)[0]):
        session = HostSession(prefix + ".fa", prefix + ".gtf")
        session.read_chimeric_alignments(source)
        columns = _batch_columns(session)
        different = [key for key in expected if expected[key] != columns[key]]
        assert not different, different
    assert expected["n"] > 1500


def test_host_ingest_tells_a_malformed_line(built, dataset_files, sam_text, tmp_path):
    from arriba_amd.pipeline import ArribaError, HostSession
    prefix = dataset_files("toy3k")
    lines = sam_text("toy3k")[0].split(b"\n")
    lines[4000] = b"\t".join(lines[4000].split(b"\t")[:10])
    session = HostSession(prefix + ".fa", prefix + ".gtf")
    with pytest.raises(ArribaError, match="failed to load alignments: SAM line 4001: fewer than 11 fields"):
        session.read_chimeric_alignments(b"\n".join(lines))


def test_cpp_driver_on_the_harness_says_that_it_has_no_transcoder(built, dataset_files, emu_api, text_samples, tmp_path):
    """the test-only build of the C++ driver against the host stepping harness links without the transcoder's kernels and refuses text with a message"""
    directory = os.path.join(conftest.ROOT, "tests", "emu")
    subprocess.run(["make", "-s", "-C", directory, "workflow_on_harness"], check=True)
    prefix = text_samples("toy3k")
    result = subprocess.run([os.path.join(directory, "workflow_on_harness"), prefix + ".fa", prefix + ".gtf", prefix + ".bam", str(tmp_path / "f.tsv")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert result.returncode != 0 and "SAM text needs the transcoder of the device library" in result.stderr


# ---- GPU tier -----------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def device():
    """(api, context) of the device library; one context for the transcoder tests"""
    from arriba_amd import _capi
    api = _capi.bind_device_api(_capi.device_library())
    params = _capi.Params()
    api.default_params(ctypes.byref(params))
    context = api.create(0, ctypes.byref(params))
    assert context, api.last_error()
    yield api, context
    api.destroy(context)


def _device_transcode(device, text, names):
    api, context = device
    return _transcode(api.sam_transcode, (context,), text, names)


@pytest.mark.gpu
def test_device_transcoder_equals_the_host_transcoder(built, device, sam_text):
    """agpu_sam_transcode (sam_newline_count / sam_line_start / sam_size / sam_emit kernels) against ahost_sam_transcode (the same sam_core.hpp stepped on the host), byte for
    byte and on the malformed line: the text of toy3k (8 k lines), the hand-made lines (a read longer than the staging window among them), every malformed text"""
    text, names = sam_text("toy3k")
    mine, theirs = _device_transcode(device, text, names), _host_transcode(text, names)
    assert mine[0] == 0 and mine[2] > 4000 and mine == theirs
    for variant, (text, expected) in sorted(_hand_made_texts().items()):
        mine = _device_transcode(device, text.encode(), HAND_NAMES)
        assert mine == _host_transcode(text.encode(), HAND_NAMES) and mine[1] == expected and mine[0] == 0, variant
    for what, text, line, expected in _malformed_cases():
        mine = _device_transcode(device, text.encode(), HAND_NAMES)
        assert mine[0] != 0 and mine[3] == line and mine[1] == expected, what
        assert mine[1:] == _host_transcode(text.encode(), HAND_NAMES)[1:], what
        assert re.match(r"failed to load alignments: SAM line %d: \w" % line, device[0].last_error().decode()), what


@pytest.mark.gpu
@pytest.mark.parametrize("windows", [None, "1048576,65536"])
@pytest.mark.parametrize("name", SAM_DATASETS)
def test_device_ingest_from_text_builds_the_batch_of_the_bam_file(name, windows, built, dataset_files, text_samples, monkeypatch):
    """the text in pieces of 1 MiB (lines straddle them) through agpu_ingest_push_sam, the front of the ingest in windows behind it: every column of the batch, coverage_t and the
    strandedness vote equal the HOST ingest of the BAM file"""
    from arriba_amd.pipeline import DevicePipeline, HostSession
    if windows is None:
        monkeypatch.delenv("ARRIBA_INGEST_WINDOWS", raising=False)
    else:
        monkeypatch.setenv("ARRIBA_INGEST_WINDOWS", windows)
    prefix = dataset_files(name)
    host = parity.open_session(prefix)
    expected = _batch_columns(host)
    expected["coverage"] = int(host._lib.ahost_coverage_checksum(host._session))
    session = HostSession(prefix + ".fa", prefix + ".gtf")
    pipeline = DevicePipeline(session, bam=text_samples(name) + ".bam", piece_bytes=1 << 20)
    columns = _device_batch_columns(session, pipeline)
    different = [key for key in expected if expected[key] != columns[key]]
    assert not different, different
    assert pipeline.ingest_result.records == sum(1 for line in open(text_samples(name) + ".bam", "rb") if not line.startswith(b"@"))
    if "--shuffle" not in DEVICE_INGEST_DATASETS[name]:  # (mates apart: the windows are given up and everything is sorted behind the last piece)
        assert pipeline.ingest_result.windows >= 1
    assert pipeline.detect_strandedness() == host.detect_strandedness()
    pipeline.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["toy3k", "rules8k"])
def test_workflow_from_text(name, built, text_samples, tmp_path):
    """text in, fusions.tsv and discarded.tsv out, both equal to the reference's files, every (remaining=N) of its log met.  run_workflow notes 18 stages
    on every run and two more (recover_known_fusions, filter_blacklisted_ranges) with the rule files of rules8k; the last one is recover_isoforms"""
    stages = parity.check_workflow(text_samples(name), conftest.golden_dir(name), str(tmp_path), rules=name == "rules8k", device_ingest=True)
    assert len(stages) == (20 if name == "rules8k" else 18) and stages[-1][0] == "recover_isoforms" and stages[-1][1] > 40


@pytest.mark.gpu
def test_command_line_reads_text_from_a_file_and_from_standard_input(built, dataset_files, sam_text, tmp_path):
    """arriba_gpu_workflow -x sample.sam, and cat sample.sam | arriba_gpu_workflow -x /dev/stdin: each a fresh process, both give the reference's two files"""
    prefix = dataset_files("toy3k")
    golden = conftest.golden_dir("toy3k")
    sample = str(tmp_path / "sample.sam")
    open(sample, "wb").write(sam_text("toy3k")[0])
    binary = os.path.join(conftest.ROOT, "arriba_amd", "lib", "arriba_gpu_workflow")
    for way in ("file", "stdin"):
        outputs = [str(tmp_path / (way + ".fusions.tsv")), str(tmp_path / (way + ".discarded.tsv"))]
        command = [binary, "-x", sample if way == "file" else "/dev/stdin", "-g", prefix + ".gtf", "-a", prefix + ".fa", "-o", outputs[0], "-O", outputs[1], "-f", "blacklist"]
        result = subprocess.run(["timeout", "-k", "10", "120"] + command, stdin=open(sample, "rb") if way == "stdin" else subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        assert result.returncode == 0, (way, result.stderr[-2000:])
        for mine, reference in zip(outputs, ("fusions.tsv.gz", "discarded.tsv.gz")):
            assert open(mine).read() == gzip.open(os.path.join(golden, reference), "rt").read(), (way, reference)


@pytest.mark.gpu
def test_a_malformed_line_fails_the_sample_and_not_the_next_one(built, dataset_files, sam_text, text_samples, tmp_path):
    """a malformed line in the second of three pieces: the sample fails with the number of the line, and the BAM file ingested next on the same pipeline comes out right"""
    from arriba_amd.pipeline import ArribaError, DevicePipeline, HostSession
    prefix = dataset_files("toy3k")
    text = sam_text("toy3k")[0]
    lines = text.split(b"\n")
    sizes = np.cumsum([len(line) + 1 for line in lines])
    header_bytes = int(sizes[sum(1 for line in lines if line.startswith(b"@")) - 1])
    bad = int(np.searchsorted(sizes, header_bytes + (3 << 19)))  # in the middle of the second MiB behind the header lines
    assert (text.__len__() - header_bytes) > (2 << 20) and not lines[bad].startswith(b"@")
    fields = lines[bad].split(b"\t")
    fields[5] = b"10M5Q"
    lines[bad] = b"\t".join(fields)
    damaged = str(tmp_path / "damaged.bam")
    open(damaged, "wb").write(b"\n".join(lines))
    host = parity.open_session(prefix)
    expected = _batch_columns(host)
    expected["coverage"] = int(host._lib.ahost_coverage_checksum(host._session))
    session = HostSession(prefix + ".fa", prefix + ".gtf")
    pipeline = DevicePipeline(session, bam=prefix + ".bam", piece_bytes=1 << 20)
    with pytest.raises(ArribaError, match="failed to load alignments: SAM line %d: malformed CIGAR" % (bad + 1)):
        pipeline.read_chimeric_alignments(damaged, piece_bytes=1 << 20)
    pipeline.read_chimeric_alignments(prefix + ".bam", piece_bytes=1 << 20)
    columns = _device_batch_columns(session, pipeline)
    different = [key for key in expected if expected[key] != columns[key]]
    assert not different, different
    pipeline.close()
