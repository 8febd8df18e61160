"""--supporting-alignments: one small sorted, indexed BAM file per row of fusions.tsv with the alignments of the row's read_identifiers that lie near its breakpoints (what the
reference's scripts/extract_fusion-supporting_alignments.sh gets from samtools view / sort / index).

The independent side is `_restate`: the script restated in plain Python from its rules -- the names are the comma-separated entries of column 30, a record belongs to a name when
its QNAME equals it byte for byte; per breakpoint (columns 5 and 6, printed position P, window W) the region is CONTIG:max(P,W)-W .. max(P,W)+W, 1-based and closed, which a record
with 0-based pos and exclusive end overlaps when pos < P'+W and end > max(P'-W-1, 0); every input record at most once; the order of --sorted-bam.  tools/read_bam.py reads the
files and checks their blocks.  `_checks` is applied to every file produced:
  1. the header equals the header of the --sorted-bam file of the same input
  2. the records equal the restatement's list, byte for byte and in order
  3. they are a subsequence of the records of the --sorted-bam file
  4. blocks are stored and hold 0xff00 bytes except the last, and the file has the length computed from its records
  5. 30 seeded regions per file and the two windows themselves give the brute-force set through the .bai; the pseudo-bin counts and n_no_coor == 0 hold
The CPU tier runs arriba_amd/csrc/device/supporting_core.hpp stepped on the host (ahost_supporting_alignments), the GPU tier the kernels of agpu_supporting.hip, byte for byte
against it."""
import ctypes
import gzip
import os
import random
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import conftest

sys.path.insert(0, os.path.join(conftest.ROOT, "tools"))
import read_bam  # noqa: E402

DATASET_NAMES = ["toy3k", "shuffled2k", "itd6k"]
PAYLOAD, FRAME = 0xff00, 31
HAND_WINDOW = 1000


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------------------------------

def _split(stream):
    """uncompressed BAM stream -> (header bytes, record bytes)"""
    assert stream[:4] == b"BAM\x01"
    at = 8 + struct.unpack_from("<i", stream, 4)[0]
    n_ref = struct.unpack_from("<i", stream, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", stream, at)[0]
    return stream[:at], stream[at:]


def _records(record_bytes):
    out, at = [], 0
    while at < len(record_bytes):
        size = 4 + struct.unpack_from("<i", record_bytes, at)[0]
        out.append(record_bytes[at:at + size])
        at += size
    assert at == len(record_bytes)
    return out


def _references_of(header):
    l_text = struct.unpack_from("<i", header, 4)[0]
    at, out = 12 + l_text, []
    for _ in range(struct.unpack_from("<i", header, 8 + l_text)[0]):
        l_name = struct.unpack_from("<i", header, at)[0]
        out.append((header[at + 4:at + 3 + l_name].decode(), struct.unpack_from("<I", header, at + 4 + l_name)[0]))
        at += 8 + l_name
    return out


CIGAR_CODES = {op: code for code, op in enumerate("MIDNSHP=X")}
CONSUMES_REFERENCE = (0, 2, 3, 7, 8)


def _record(qname, flag, ref, pos, cigar, l_seq, next_ref=-1, next_pos=-1, aux=b""):
    """a BAM record (SAMv1 4.2); pos 0-based, cigar a list of (length, op); the `bin` field holds a constant, as the datasets' generator writes it"""
    body = struct.pack("<iiBBHHHiiii", ref, pos, len(qname) + 1, 30, 4680, len(cigar), flag, l_seq, next_ref, next_pos, 0)
    body += qname.encode() + b"\0" + b"".join(struct.pack("<I", length << 4 | CIGAR_CODES[op]) for length, op in cigar)
    body += bytes((17 * k + 1) & 0xff for k in range((l_seq + 1) // 2)) + bytes(k % 41 for k in range(l_seq)) + aux
    return struct.pack("<i", len(body)) + body


def _pad(size):
    """an optional field of exactly `size` bytes (>= 4)"""
    return b"XPZ" + b"x" * (size - 4) + b"\0"


def _write_bgzf(path, payload, level):
    """`payload` as a BGZF file: blocks of 0xff00 bytes, deflated at `level` (0: stored), and the end-of-file block"""
    with open(path, "wb") as out:
        for at in range(0, len(payload), PAYLOAD):
            piece = payload[at:at + PAYLOAD]
            deflater = zlib.compressobj(level, zlib.DEFLATED, -15)
            body = deflater.compress(piece) + deflater.flush()
            out.write(struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(body) + 25) + body + struct.pack("<II", zlib.crc32(piece), len(piece)))
        out.write(read_bam.EOF_BLOCK)


class Parsed(object):
    """what the restatement needs of a record, read with struct from its bytes"""
    __slots__ = ("bytes", "ref", "pos", "end", "flag", "name")

    def __init__(self, data):
        self.bytes = data
        self.ref, self.pos, l_read_name, _, _, n_cigar, self.flag = struct.unpack_from("<iiBBHHH", data, 4)
        self.name = data[36:36 + l_read_name - 1]
        length = 0
        if not self.flag & 4:
            for op in struct.unpack_from("<%dI" % n_cigar, data, 36 + l_read_name):
                if op & 15 in CONSUMES_REFERENCE:
                    length += op >> 4
        self.end = self.pos + (length if length > 0 else 1)


def _sorted(records):
    """the order of --sorted-bam: (refID as unsigned, pos + 1, reverse strand), ties in input order"""
    parsed = [Parsed(record) for record in records]
    return [parsed[k] for k in sorted(range(len(parsed)), key=lambda k: (parsed[k].ref & 0xffffffff, parsed[k].pos + 1, parsed[k].flag >> 4 & 1, k))]


def _region(position, window):
    """printed 1-based position -> the region of the script, 1-based and closed"""
    centre = max(position, window)
    return centre - window, centre + window


def _overlaps(record, ref, position, window):
    low, high = _region(position, window)
    return record.ref >= 0 and record.ref == ref and record.pos < high and record.end > max(low - 1, 0)


def _restate(sorted_records, rows, window):
    """rows: [(names, ((ref, P), (ref, P)))] with P the printed 1-based position -> per row the records of its file"""
    out = []
    for names, breakpoints in rows:
        listed = set(names)
        out.append([record for record in sorted_records if record.name in listed and any(_overlaps(record, ref, position, window) for ref, position in breakpoints)])
    return out


class Case(object):
    """an input with its rows: header, record bytes, the explicit list of names, rows as the restatement takes them and as the C ABI takes them"""

    def __init__(self, header, record_bytes, rows, extra_names=()):
        self.header, self.record_bytes, self.rows = header, record_bytes, rows
        self.references = _references_of(header)
        self.sorted = _sorted(_records(record_bytes))
        # the list of names as a caller would give it: every listing of a name is an entry of its own (the same name more than once), plus names no row lists
        self.names, entries, self.name_begin = [], [], [0]
        for names, _ in rows:
            for name in names:
                entries.append(len(self.names))
                self.names.append(name)
            self.name_begin.append(len(entries))
        self.names += list(extra_names)
        self.entries = entries

    def abi_rows(self):
        from arriba_amd import _capi
        ref = np.array([[ref for ref, _ in breakpoints] for _, breakpoints in self.rows], dtype=np.int32).reshape(-1)
        breakpoint = np.array([[position - 1 for _, position in breakpoints] for _, breakpoints in self.rows], dtype=np.int32).reshape(-1)
        name_begin, names = np.array(self.name_begin, dtype=np.uint64), np.array(self.entries, dtype=np.uint32)
        keep = (ref, breakpoint, name_begin, names)
        return _capi.SupportingRows(len(self.rows), ref.ctypes.data, breakpoint.ctypes.data, name_begin.ctypes.data, names.ctypes.data if names.size else None), keep

    def pipeline_rows(self):
        n = len(self.rows)
        return {"ref": np.array([[ref for ref, _ in breakpoints] for _, breakpoints in self.rows], dtype=np.int32).reshape(n, 2),
                "breakpoint": np.array([[position - 1 for _, position in breakpoints] for _, breakpoints in self.rows], dtype=np.int32).reshape(n, 2),
                "name_begin": np.array(self.name_begin, dtype=np.uint64), "names": np.array(self.entries, dtype=np.uint32)}


def _rows_of_fusions(text, references):
    """the data rows of a fusions.tsv -> [(names, ((ref, P), (ref, P)))]"""
    number = {name: k for k, (name, _) in enumerate(references)}
    rows = []
    for line in text.split("\n"):
        if not line or line.startswith("#"):
            continue
        fields = line.split("\t")
        breakpoints = []
        for column in (4, 5):
            contig, _, position = fields[column].rpartition(":")
            breakpoints.append((number.get(contig, number.get("chr" + contig, -1)), int(position)))
        rows.append(([] if fields[29] == "." else [name.encode() for name in fields[29].split(",")], tuple(breakpoints)))
    return rows


def _hand_made(header):
    """records on the references of toy3k and rows around them, W = HAND_WINDOW; returns a Case"""
    references = _references_of(header)
    assert len(references) >= 4 and all(length >= 255000 for _, length in references[:4])
    last = references[3][1]  # the printed position of the last base of reference 3
    long_name = "y" * 254
    base = _record("exact", 0, 2, 100000, [(5, "M")], 5)
    big = _record("g_big", 0, 2, 150000, [(5, "M")], 5)
    small = _record("g", 0, 2, 150010, [(1, "M")], 1)
    assert len(small) == 44
    records = [
        # row 0: (reference 0, P = 5000) and (reference 1, P = 20000): the window on reference 0 is 4000 .. 6000, 1-based and closed
        _record("ends_before", 0, 0, 3989, [(10, "M")], 10),       # its last base is 3999: one base in front of the window
        _record("ends_on_first", 0, 0, 3990, [(10, "M")], 10),     # its last base is 4000
        _record("starts_on_last", 16, 0, 5999, [(10, "M")], 10),   # its first base is 6000
        _record("starts_past", 0, 0, 6000, [(10, "M")], 10),       # its first base is 6001
        _record("r1", 0, 0, 4500, [(20, "M")], 20), _record("r10", 0, 0, 4600, [(20, "M")], 20),
        _record("x", 0, 0, 4700, [(20, "M")], 20), _record(long_name, 16, 0, 4800, [(20, "M")], 20),
        _record("shared", 0, 0, 5000, [(30, "M")], 30), _record("shared", 16, 1, 50400, [(30, "M")], 30),
        _record("unlisted", 0, 0, 5000, [(30, "M")], 30),
        # row 1: (reference 2, P = 300): P < W, the region is 1 .. 2000; and the last base of reference 3
        _record("clamp_first", 0, 2, 0, [(10, "M")], 10), _record("clamp_in", 0, 2, 1990, [(20, "M")], 20), _record("clamp_out", 0, 2, 2000, [(20, "M")], 20),
        _record("at_last_base", 0, 3, last - 1, [(1, "M")], 1), _record("before_last_window", 0, 3, last - 1 - HAND_WINDOW - 10, [(9, "M")], 9),
        # row 2: both breakpoints on reference 1 (P = 50000 and P = 50500): a record in both windows, the mates, the twins, a listed name without a coordinate
        _record("in_both", 0, 1, 50200, [(40, "M")], 40),
        _record("mates", 73, 1, 50100, [(50, "M")], 50, 1, 50100), _record("mates", 133, 1, 50100, [], 50, 1, 50100),
        _record("twin", 0, 1, 50300, [(25, "M")], 25), _record("twin", 0, 1, 50300, [(25, "M")], 25),
        _record("in_both", 4, -1, -1, [], 20), _record("nocoord", 77, -1, -1, [], 20),
        # row 3: its names have records, none of them in its windows: an empty file
        _record("lonely", 0, 2, 200000, [(20, "M")], 20),
        # row 4: a read of 70 000 bases over three blocks of its file, behind 30 kB
        _record("pad30k", 0, 3, 99000, [(12, "M")], 12, aux=_pad(30000)), _record("long_read", 0, 3, 100000, [(70000, "M")], 70000),
        # row 5: a file that ends exactly on a block boundary
        _record("exact", 0, 2, 100000, [(5, "M")], 5, aux=_pad(PAYLOAD - len(base))),
        # row 6: a last block of 40 bytes
        _record("g_big", 0, 2, 150000, [(5, "M")], 5, aux=_pad(PAYLOAD - 4 - len(big))), small,
    ]
    generator = random.Random(11)
    for k in range(24):  # records of names nobody lists, all over the windows
        records.append(_record("filler_%d" % k, generator.choice((0, 16, 99, 147)), generator.randrange(4), generator.choice((4000, 5000, 1000, 50200, 100000)) + generator.randrange(-900, 900), [(40, "M"), (generator.randrange(1, 300), "N"), (35, "M")], 75))
    generator.shuffle(records)
    rows = [
        ([b"ends_before", b"ends_on_first", b"starts_on_last", b"starts_past", b"r1", b"x", long_name.encode(), b"shared", b"r1"], ((0, 5000), (1, 20000))),  # (r1 twice: once in the file)
        ([b"clamp_first", b"clamp_in", b"clamp_out", b"at_last_base", b"before_last_window"], ((2, 300), (3, last))),
        ([b"in_both", b"mates", b"twin", b"nocoord", b"shared"], ((1, 50000), (1, 50500))),
        ([b"lonely", b"r10", b"nocoord"], ((0, 100000), (0, 200000))),
        ([b"pad30k", b"long_read"], ((3, 100001), (0, 250000))),
        ([b"exact"], ((2, 100001), (2, 100001))),
        ([b"g_big", b"g"], ((2, 150001), (1, 1))),
    ]
    return Case(header, b"".join(records), rows, extra_names=[b"nobody", b"r100"])


@pytest.fixture(scope="module")
def cases(dataset_files):
    """name -> Case: the three datasets with the rows of their golden fusions.tsv, and the hand-made records on the references of toy3k"""
    cache = {}

    def get(name):
        if name not in cache:
            if name in DATASET_NAMES:
                header, record_bytes = _split(gzip.open(dataset_files(name) + ".bam", "rb").read())
                text = gzip.open(os.path.join(conftest.golden_dir(name), "fusions.tsv.gz"), "rt").read()
                cache[name] = Case(header, record_bytes, _rows_of_fusions(text, _references_of(header)))
            else:
                cache[name] = _hand_made(get("toy3k").header)
        return cache[name]
    return get


# ---- the checks -----------------------------------------------------------------------------------------------------------------------------------------------

def _host_sorted(case, path):
    from arriba_amd import _capi
    lib = _capi.host_library()
    assert lib.ahost_sorted_bam_write(case.header, len(case.header), case.record_bytes, len(case.record_bytes), path.encode(), None) == 0, lib.ahost_last_error()
    return read_bam.BamFile(path)


def _regions(references, records, breakpoints, window, seed):
    """30 seeded regions (reference number, begin, end), 0-based and half open, and the two windows themselves"""
    generator = random.Random(seed)
    populated = sorted({record.ref for record in records if 0 <= record.ref < len(references)}) or [0]
    regions = []
    for k in range(30):
        reference = generator.choice(populated) if k % 5 else generator.randrange(len(references))
        length = references[reference][1]
        span = min(length, max(1, int(2 ** generator.uniform(0, np.log2(length)))))
        begin = generator.randrange(0, length - span + 1)
        if k % 7 == 0:
            begin = min(begin >> 14 << 14, length - 1)
        regions.append((reference, begin, min(begin + span, length)))
    for k, record in enumerate(records[:10]):  # ... some of which touch the ends of records
        regions[k] = (record.ref, max(record.end - 1, 0), record.end) if k % 2 else (record.ref, record.pos, record.pos + 1)
    for ref, position in breakpoints:
        if 0 <= ref < len(references):
            low, high = _region(position, window)
            regions.append((ref, max(low - 1, 0), min(high, references[ref][1])))
    return regions


def _checks(prefix, case, window, sorted_bam, expected=None, seed=1):
    """every file of the prefix against the restatement; returns the restatement's lists"""
    expected = expected if expected is not None else _restate(case.sorted, case.rows, window)
    sorted_position = {}
    for k, record in enumerate(sorted_bam.records):
        sorted_position.setdefault(record.bytes, []).append(k)
    for row, (wanted, (_, breakpoints)) in enumerate(zip(expected, case.rows)):
        path = "%s_%d.bam" % (prefix, row + 1)
        bam = read_bam.BamFile(path)
        # 1. the header of the --sorted-bam file
        assert bam.data[:bam.header_size] == sorted_bam.data[:sorted_bam.header_size] and bam.references == sorted_bam.references
        # 2. the restatement's records, in its order
        assert [record.bytes for record in bam.records] == [record.bytes for record in wanted], path
        # 3. a subsequence of the --sorted-bam file (byte-identical records take the places of the sorted file one after the other)
        at, taken = -1, {}
        for record in bam.records:
            places = sorted_position[record.bytes]
            taken[record.bytes] = taken.get(record.bytes, -1) + 1
            place = places[taken[record.bytes]]
            assert place > at, path
            at = place
        # 4. the blocks
        sizes = [len(payload) for _, payload in bam.blocks]
        header_blocks = 0
        while sum(sizes[:header_blocks]) < bam.header_size:
            header_blocks += 1
        assert sum(sizes[:header_blocks]) == bam.header_size and sizes[-1] == 0
        record_sizes, total = sizes[header_blocks:-1], sum(len(record.bytes) for record in wanted)
        assert all(size == PAYLOAD for size in record_sizes[:-1]) and all(0 < size <= PAYLOAD for size in record_sizes[-1:]) and sum(record_sizes) == total
        assert len(record_sizes) == (total + PAYLOAD - 1) // PAYLOAD
        assert all(read_bam.is_stored(bam.raw, offset) for offset, _ in bam.blocks[:-1])
        assert len(bam.raw) == bam.blocks[header_blocks][0] + total + FRAME * len(record_sizes) + 28
        # 5. the index
        bai = read_bam.BaiFile(path + ".bai")
        assert len(bai.references) == len(bam.references) and bai.n_no_coor == 0
        for reference, index in enumerate(bai.references):
            mine = [record for record in bam.records if record.ref == reference]
            if mine:
                assert index["pseudo"][2:] == (sum(1 for r in mine if not r.flag & 4), sum(1 for r in mine if r.flag & 4))
                assert bam.uncompressed_offset(index["pseudo"][0]) == mine[0].start and bam.uncompressed_offset(index["pseudo"][1]) == mine[-1].start + len(mine[-1].bytes)
            else:
                assert index["pseudo"] is None and not index["bins"] and not index["linear"]
        for reference, begin, end in _regions(bam.references, bam.records, breakpoints, window, seed + row):
            found, brute = read_bam.query(bam, bai, reference, begin, end), read_bam.brute_force(bam, reference, begin, end)
            assert [record.start for record in found] == [record.start for record in brute], (path, reference, begin, end)
    return expected


def _expected_names(prefix, n_rows):
    return sorted(os.path.basename(prefix) + "_%d.bam%s" % (row + 1, suffix) for row in range(n_rows) for suffix in ("", ".bai"))


def _host_write(case, window, prefix):
    from arriba_amd import _capi
    lib, info = _capi.host_library(), _capi.SupportingInfo()
    names = b"".join(case.names)
    offsets = np.zeros(len(case.names) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(name) for name in case.names], dtype=np.uint64) if case.names else 0
    rows, keep = case.abi_rows()
    status = lib.ahost_supporting_alignments(case.header, len(case.header), case.record_bytes, len(case.record_bytes), names, offsets.ctypes.data, len(case.names), ctypes.byref(rows), window, prefix.encode(), ctypes.byref(info))
    assert status == 0, lib.ahost_last_error()
    return info


@pytest.fixture(scope="module")
def sorted_files(cases, tmp_path_factory):
    """name -> the --sorted-bam file of the input as tools/read_bam.py reads it: made once"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _host_sorted(cases(name), str(tmp_path_factory.mktemp("sorted_" + name) / "sorted.bam"))
        return cache[name]
    return get


@pytest.fixture(scope="module")
def host_files(cases, tmp_path_factory):
    """(name, window) -> the prefix of the files ahost_supporting_alignments makes: computed once, compared against by every device test"""
    cache = {}

    def get(name, window):
        if (name, window) not in cache:
            cache[(name, window)] = str(tmp_path_factory.mktemp("host_%s_%d" % (name, window)) / "support")
            _host_write(cases(name), window, cache[(name, window)])
        return cache[(name, window)]
    return get


# ---- CPU tier -------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", DATASET_NAMES)
def test_host_writes_the_files_of_a_dataset(name, built, cases, sorted_files, tmp_path):
    case = cases(name)
    candidates = sum(len([record for record in case.sorted if record.name in set(names)]) for names, _ in case.rows)
    selected, in_both, large = {}, 0, 0
    for window in (1000000, 2000):
        prefix = str(tmp_path / ("w%d" % window) / "support")
        os.makedirs(os.path.dirname(prefix))
        info = _host_write(case, window, prefix)
        expected = _checks(prefix, case, window, sorted_files(name))
        selected[window] = sum(len(records) for records in expected)
        assert info.rows == len(case.rows) and info.records == selected[window] and info.uncompressed_bytes == sum(len(record.bytes) for records in expected for record in records)
        assert sorted(os.listdir(os.path.dirname(prefix))) == _expected_names(prefix, len(case.rows))
        if window == 1000000:
            in_both = sum(1 for records, (_, breakpoints) in zip(expected, case.rows) for record in records if all(_overlaps(record, ref, position, window) for ref, position in breakpoints))
            large = sum(1 for records in expected if sum(len(record.bytes) for record in records) > PAYLOAD)
    print("%s: %d rows, %d records of listed names, %d selected (W=1000000), %d selected (W=2000), %d in both windows, %d files larger than a block" % (name, len(case.rows), candidates, selected[1000000], selected[2000], in_both, large))
    # the window, the once-per-record rule and the block loop are all exercised
    assert selected[2000] < selected[1000000] < candidates
    assert large >= 1 and in_both >= 1


def test_hand_made_records(built, cases, sorted_files, tmp_path, monkeypatch):
    monkeypatch.delenv("ARRIBA_SUPPORT_HASH_BITS", raising=False)
    case = cases("hand_made")
    prefix = str(tmp_path / "plain" / "support")
    os.makedirs(os.path.dirname(prefix))
    _host_write(case, HAND_WINDOW, prefix)
    expected = _checks(prefix, case, HAND_WINDOW, sorted_files("hand_made"))
    names = [[record.name.decode() for record in records] for records in expected]
    # the restatement itself, on the cases it was built for
    assert sorted(names[0]) == sorted(["ends_on_first", "starts_on_last", "r1", "x", "y" * 254, "shared"]) and [r.ref for r in expected[0]] == [0] * 6
    assert names[1] == ["clamp_first", "clamp_in", "at_last_base"]
    assert names[2] == ["mates", "mates", "in_both", "twin", "twin", "shared"] and sorted(record.flag for record in expected[2][:2]) == [73, 133] and expected[2][3].bytes == expected[2][4].bytes
    assert names[3] == [] and names[4] == ["pad30k", "long_read"] and names[5] == ["exact"] and names[6] == ["g_big", "g"]
    files = [read_bam.BamFile("%s_%d.bam" % (prefix, row + 1)) for row in range(len(case.rows))]
    assert len(files[3].blocks) == 2 and not files[3].records                                                      # header and end-of-file block
    bai = read_bam.BaiFile("%s_4.bam.bai" % prefix)
    assert all(not index["bins"] and not index["linear"] and index["pseudo"] is None for index in bai.references)   # an index with empty references
    long_read, first = files[4].records[1], files[4].header_size
    assert (long_read.start + len(long_read.bytes) - 1 - first) // PAYLOAD - (long_read.start - first) // PAYLOAD == 2  # three blocks
    assert [len(payload) for _, payload in files[5].blocks[1:]] == [PAYLOAD, 0]                                    # ends exactly on a block boundary
    assert [len(payload) for _, payload in files[6].blocks[1:]] == [PAYLOAD, 40, 0]                                # a last block shorter than 64 bytes
    # forced collisions and long probe runs: identical files
    monkeypatch.setenv("ARRIBA_SUPPORT_HASH_BITS", "4")
    collided = str(tmp_path / "collided" / "support")
    os.makedirs(os.path.dirname(collided))
    _host_write(case, HAND_WINDOW, collided)
    for entry in _expected_names(prefix, len(case.rows)):
        assert open(os.path.join(os.path.dirname(prefix), entry), "rb").read() == open(os.path.join(os.path.dirname(collided), entry), "rb").read(), entry
    assert sorted(os.listdir(os.path.dirname(collided))) == _expected_names(collided, len(case.rows))


def test_zero_rows_give_no_file(built, cases, tmp_path):
    case = cases("hand_made")
    empty = Case(case.header, case.record_bytes, [], extra_names=[b"shared"])
    info = _host_write(empty, HAND_WINDOW, str(tmp_path / "support"))
    assert info.rows == 0 and info.records == 0 and os.listdir(str(tmp_path)) == []


def test_a_failure_leaves_nothing_of_the_prefix_behind(built, cases, tmp_path):
    """row 3 cannot be opened (a directory has its temporary name): the call fails with a message and the files of rows 1 and 2 are gone again"""
    from arriba_amd import _capi
    case = cases("hand_made")
    prefix = str(tmp_path / "support")
    os.mkdir(prefix + "_3.bam.tmp")
    lib = _capi.host_library()
    names = b"".join(case.names)
    offsets = np.zeros(len(case.names) + 1, np.uint64)
    offsets[1:] = np.cumsum([len(name) for name in case.names], dtype=np.uint64)
    rows, keep = case.abi_rows()
    assert lib.ahost_supporting_alignments(case.header, len(case.header), case.record_bytes, len(case.record_bytes), names, offsets.ctypes.data, len(case.names), ctypes.byref(rows), HAND_WINDOW, prefix.encode(), None) != 0
    assert b"support_3.bam.tmp" in lib.ahost_last_error() and os.listdir(str(tmp_path)) == ["support_3.bam.tmp"]


# ---- GPU tier -------------------------------------------------------------------------------------------------------------------------------------------------

def _same_files(mine, theirs, n_rows):
    assert sorted(os.listdir(os.path.dirname(mine))) == _expected_names(mine, n_rows)
    for row in range(n_rows):
        for suffix in (".bam", ".bam.bai"):
            assert open("%s_%d%s" % (mine, row + 1, suffix), "rb").read() == open("%s_%d%s" % (theirs, row + 1, suffix), "rb").read(), (row + 1, suffix)


def _set_knobs(monkeypatch, **knobs):
    for knob, value in knobs.items():
        if value is None:
            monkeypatch.delenv(knob, raising=False)
        else:
            monkeypatch.setenv(knob, value)


@pytest.mark.gpu
@pytest.mark.parametrize("name,window,ingest_windows,copy_window", [(name, window, ingest_windows, None) for name in DATASET_NAMES for window, ingest_windows in ((1000000, None), (2000, None), (1000000, "1048576,65536"))] + [("itd6k", 1000000, None, "131072")])
def test_device_files_are_the_host_files(name, window, ingest_windows, copy_window, built, dataset_files, cases, sorted_files, host_files, tmp_path, monkeypatch):
    from arriba_amd.pipeline import DevicePipeline, HostSession
    _set_knobs(monkeypatch, ARRIBA_INGEST_WINDOWS=ingest_windows, ARRIBA_SUPPORTING_WINDOW=copy_window, ARRIBA_SUPPORT_HASH_BITS=None)
    case, files = cases(name), dataset_files(name)
    pipeline = DevicePipeline(HostSession(files + ".fa", files + ".gtf"), bam=files + ".bam", piece_bytes=1 << 20)
    pool = pipeline.build_support_pool(names=case.names)
    prefix = str(tmp_path / "support")
    written = pipeline.write_supporting_alignments(prefix, case.pipeline_rows(), window)
    pipeline.close()
    assert pool["names"] == len(case.names) and pool["stream_records"] == len(case.sorted) and 0 < pool["pooled_records"] <= len(case.sorted)
    assert written["rows"] == len(case.rows) and (written["windows"] > 1 if copy_window else written["windows"] == 1)
    _same_files(prefix, host_files(name, window), len(case.rows))
    expected = _checks(prefix, case, window, sorted_files(name))
    assert written["records"] == sum(len(records) for records in expected)
    assert not [entry for entry in os.listdir(str(tmp_path)) if entry.endswith(".tmp")]


@pytest.mark.gpu
@pytest.mark.parametrize("hash_bits", [None, "4"])
def test_hand_made_file_through_the_device_ingest(hash_bits, built, dataset_files, cases, sorted_files, host_files, tmp_path, monkeypatch):
    """the ingest ignores these records (no chimeric read among them), so the names are an explicit list; windows of two blocks: the long read straddles two of them"""
    from arriba_amd.pipeline import DevicePipeline, HostSession
    _set_knobs(monkeypatch, ARRIBA_SUPPORTING_WINDOW="131072", ARRIBA_SUPPORT_HASH_BITS=None)
    case, files = cases("hand_made"), dataset_files("toy3k")
    theirs = host_files("hand_made", HAND_WINDOW)  # (made with the whole hash)
    _set_knobs(monkeypatch, ARRIBA_SUPPORT_HASH_BITS=hash_bits)
    sample = str(tmp_path / "hand.bam")
    _write_bgzf(sample, case.header + case.record_bytes, 0)
    pipeline = DevicePipeline(HostSession(files + ".fa", files + ".gtf"), bam=files + ".bam")
    pipeline._ingest_records(sample, False, 100, 64 << 20)  # (without the host's "no normal reads found": the stream is what matters here)
    pipeline.build_support_pool(names=case.names)
    os.mkdir(str(tmp_path / "out"))
    prefix = str(tmp_path / "out" / "support")
    written = pipeline.write_supporting_alignments(prefix, case.pipeline_rows(), HAND_WINDOW)
    empty = pipeline.write_supporting_alignments(str(tmp_path / "none"), {"ref": np.zeros((0, 2), np.int32), "breakpoint": np.zeros((0, 2), np.int32), "name_begin": np.zeros(1, np.uint64), "names": np.zeros(0, np.uint32)}, HAND_WINDOW)
    pipeline.close()
    assert written["windows"] > 1 and empty["rows"] == 0 and empty["records"] == 0  # (zero rows: no file at all)
    _same_files(prefix, theirs, len(case.rows))
    _checks(prefix, case, HAND_WINDOW, sorted_files("hand_made"))
    assert sorted(os.listdir(str(tmp_path))) == ["hand.bam", "out"]


@pytest.mark.gpu
@pytest.mark.parametrize("container", ["sam_text", "deflated_bgzf"])
def test_other_containers_give_the_same_records(container, built, dataset_files, cases, host_files, tmp_path):
    from arriba_amd.pipeline import DevicePipeline, HostSession
    from bam_to_sam import bam_to_sam
    case, files = cases("toy3k"), dataset_files("toy3k")
    sample = str(tmp_path / "sample.bam")
    if container == "sam_text":
        open(sample, "wb").write(bam_to_sam(open(files + ".bam", "rb").read())[0])
    else:
        _write_bgzf(sample, case.header + case.record_bytes, 6)
    pipeline = DevicePipeline(HostSession(files + ".fa", files + ".gtf"), bam=sample, piece_bytes=1 << 20)
    pipeline.build_support_pool(names=case.names)
    os.mkdir(str(tmp_path / "out"))
    prefix = str(tmp_path / "out" / "support")
    pipeline.write_supporting_alignments(prefix, case.pipeline_rows(), 2000)
    pipeline.close()
    theirs = host_files("toy3k", 2000)
    if container == "deflated_bgzf":
        _same_files(prefix, theirs, len(case.rows))
        return
    # the transcoder writes reg2bin where the generator of the dataset wrote a constant: the records of the text differ from the file's in those two bytes only
    for row in range(len(case.rows)):
        mine, wanted = read_bam.BamFile("%s_%d.bam" % (prefix, row + 1)), read_bam.BamFile("%s_%d.bam" % (theirs, row + 1))
        masked = [[bytes(record.bytes[:14]) + b"\0\0" + bytes(record.bytes[16:]) for record in bam.records] for bam in (mine, wanted)]
        assert masked[0] == masked[1], row + 1
        read_bam.BaiFile("%s_%d.bam.bai" % (prefix, row + 1))


def _command_line(prefix_of_dataset, outputs, extra):
    command = [os.path.join(conftest.ROOT, "arriba_amd", "lib", "arriba_gpu_workflow"), "-x", prefix_of_dataset + ".bam", "-g", prefix_of_dataset + ".gtf", "-a", prefix_of_dataset + ".fa", "-o", outputs[0], "-O", outputs[1], "-f", "blacklist"]
    return subprocess.run(["timeout", "-k", "10", "120"] + command + extra, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)


@pytest.mark.gpu
def test_command_line_writes_the_files_next_to_the_fusions(built, dataset_files, cases, sorted_files, tmp_path):
    files, golden, case = dataset_files("toy3k"), conftest.golden_dir("toy3k"), cases("toy3k")
    outputs = [str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv")]
    result = _command_line(files, outputs, ["--supporting-alignments", str(tmp_path / "support"), "--supporting-window", "2000", "--sorted-bam", str(tmp_path / "sorted.bam")])
    assert result.returncode == 0, result.stderr[-2000:]
    for mine, reference in zip(outputs, ("fusions.tsv.gz", "discarded.tsv.gz")):
        assert open(mine).read() == gzip.open(os.path.join(golden, reference), "rt").read(), reference
    written = Case(case.header, case.record_bytes, _rows_of_fusions(open(outputs[0]).read(), case.references))  # (the rows of the file the run itself wrote)
    assert len(written.rows) > 10
    assert sorted(os.listdir(str(tmp_path))) == sorted(["discarded.tsv", "fusions.tsv", "sorted.bam", "sorted.bam.bai"] + _expected_names("support", len(written.rows)))
    assert open(str(tmp_path / "sorted.bam"), "rb").read() == sorted_files("toy3k").raw
    _checks(str(tmp_path / "support"), written, 2000, sorted_files("toy3k"))


@pytest.mark.gpu
def test_host_ingest_steps_the_same_code(built, dataset_files, cases, sorted_files, tmp_path):
    """--host-ingest: the files come from the host stepping, with the names of the host's batch"""
    files, case = dataset_files("toy3k"), cases("toy3k")
    outputs = [str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv")]
    result = _command_line(files, outputs, ["--host-ingest", "--supporting-alignments", str(tmp_path / "support")])
    assert result.returncode == 0, result.stderr[-2000:]
    written = Case(case.header, case.record_bytes, _rows_of_fusions(open(outputs[0]).read(), case.references))
    assert len(written.rows) > 10 and sorted(os.listdir(str(tmp_path))) == sorted(["discarded.tsv", "fusions.tsv"] + _expected_names("support", len(written.rows)))
    _checks(str(tmp_path / "support"), written, 1000000, sorted_files("toy3k"))


@pytest.mark.gpu
def test_session_of_two_lanes_writes_every_sample_its_own_files(built, dataset_files, cases, sorted_files, tmp_path):
    """the next sample is submitted while the one before runs: the pool of a sample survives the hand-over of the stream to the sibling lane"""
    from arriba_amd.pipeline import WorkflowSession
    prefixes = {name: dataset_files(name) for name in ("toy3k", "itd6k")}
    session = WorkflowSession(prefixes["toy3k"] + ".fa", prefixes["toy3k"] + ".gtf", params={"disable_filters": ["blacklist"]})
    samples = []
    for k, name in enumerate(("toy3k", "itd6k", "toy3k")):  # (itd6k against the assembly of toy3k -- same contig names and lengths: its fusions mean nothing, its records are its own)
        os.mkdir(str(tmp_path / ("sample%d" % k)))
        samples.append((name, prefixes[name] + ".bam", str(tmp_path / ("sample%d" % k) / "fusions.tsv"), str(tmp_path / ("sample%d" % k) / "support")))
    session.submit(samples[0][1], supporting_alignments_prefix=samples[0][3])
    for k, (name, bam, output, prefix) in enumerate(samples):
        if k + 1 < len(samples):
            session.submit(samples[k + 1][1], supporting_alignments_prefix=samples[k + 1][3])  # fed, and its pool built, beside the stages of sample k
        session.sample(bam, output)
        assert session.timing["supporting_alignments"] > 0
    session.close()
    for name, bam, output, prefix in samples:
        case = cases(name)
        written = Case(case.header, case.record_bytes, _rows_of_fusions(open(output).read(), case.references))
        assert (written.rows or name != "toy3k") and sorted(os.listdir(os.path.dirname(prefix))) == sorted(["fusions.tsv"] + _expected_names(prefix, len(written.rows)))
        _checks(prefix, written, 1000000, sorted_files(name))
    assert open(samples[0][2]).read() == open(samples[2][2]).read()
    for entry in _expected_names(samples[0][3], 3):  # (the same sample twice, on the same lane, around a sample of the other lane)
        assert open(os.path.join(os.path.dirname(samples[0][3]), entry), "rb").read() == open(os.path.join(os.path.dirname(samples[2][3]), entry), "rb").read()


@pytest.mark.gpu
def test_refusals_and_the_off_switch(built, dataset_files, cases, sorted_files, tmp_path):
    """with the option off no kernel of it runs and no buffer of it exists; a part of a sample is refused before any launch; files without a pool are an error with a message"""
    from arriba_amd.pipeline import ArribaError, DevicePipeline, HostSession
    files, case = dataset_files("toy3k"), cases("toy3k")
    pipeline = DevicePipeline(HostSession(files + ".fa", files + ".gtf"), bam=files + ".bam")
    pipeline.set_profiling(True)
    pipeline.read_chimeric_alignments(files + ".bam")
    outputs = [str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv")]
    pipeline.run_workflow(outputs[0], outputs[1])
    assert not [launch for launch in pipeline.kernel_profile() if launch[0].startswith("support")] and pipeline.support_allocated_bytes() == 0
    with pytest.raises(ArribaError, match="there is no pool of supporting alignments"):
        pipeline.write_supporting_alignments(str(tmp_path / "none"), case.pipeline_rows(), 2000)
    # a part of a sample
    pipeline._ingest_records(files + ".bam", False, 100, 64 << 20, part=0, parts=2)
    with pytest.raises(ArribaError, match="supporting alignments of one sample over several GPUs are not supported"):
        pipeline.build_support_pool(names=case.names)
    assert not [launch for launch in pipeline.kernel_profile() if launch[0].startswith("support")] and pipeline.support_allocated_bytes() == 0
    # ... and the option on, through the stages of the pipeline: the names of the batch, the rows of the file just written
    pipeline.read_chimeric_alignments(files + ".bam")
    pipeline.run_workflow(str(tmp_path / "again.tsv"), None, supporting_alignments_prefix=str(tmp_path / "support"), supporting_alignments_window=2000)
    assert [launch for launch in pipeline.kernel_profile() if launch[0].startswith("support_mark_kernel")] and [launch for launch in pipeline.kernel_profile() if launch[0].startswith("supporting_gather_kernel")]
    assert pipeline.support_allocated_bytes() == 0  # (given back behind the files)
    pipeline.close()
    assert open(str(tmp_path / "again.tsv")).read() == open(outputs[0]).read()
    written = Case(case.header, case.record_bytes, _rows_of_fusions(open(outputs[0]).read(), case.references))
    assert sorted(os.listdir(str(tmp_path))) == sorted(["fusions.tsv", "discarded.tsv", "again.tsv"] + _expected_names("support", len(written.rows)))
    _checks(str(tmp_path / "support"), written, 2000, sorted_files("toy3k"))
