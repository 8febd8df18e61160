"""The ingest on the device (ingest_core.hpp, agpu_ingest.hip) against hand-dressed BAM records, judged by the UNMODIFIED reference.

Every other BAM file of the suite comes from tools/gen_synth, whose records have one shape (name `r%010d`: 12 bytes with the NUL; NH:C, HI:C, one fixed SA:Z; ~200 bytes).
tests/ingest_records_lib.py re-dresses the record stream of three small datasets -- new QNAMEs, new aux blocks, fixed fields / CIGAR / sequence kept -- and
tests/golden/ingest_records/<dataset>/ holds what the oracle build of the reference read from exactly those bytes (tools/make_ingest_records_golden.py; the SHA-256 of the
regenerated file is asserted, so the reference half never skips and never drifts).  Each check runs on the stepping harness (tests/emu, CPU tier) and on the kernels (gpu).

Classes of the dress (keys of the builder's table) and the code they are aimed at:

  names
    length_1 .. length_254, length_up_to_18 / 19_to_68 / 69_to_254   l_read_name % 4 takes all four values and records start on all 16 residues mod 16: load_record_at
                               (three 8-byte loads, ingest_core.hpp:107), the 16-byte staging copy (agpu_ingest.hip:178), find_byte (ingest_core.hpp:37: the 8-byte
                               turns, the overlapping last word, the byte loop below 8), the 8-byte name copy and the 4-byte sequence copy of write_fragment
    prefix                     one name a proper prefix of another: compare_names (ingest_core.hpp:1004) behind the common part, name_chunk (:999) of the shorter name
    difference_at_6 .. _16     first_difference (ingest_core.hpp:50): inside the first word, at its last byte, in the second, in the overlapping last word
    comma, X_and_X,1           commas in QNAMEs: IC_QNAME_COMMA guards the first-occurrence fast path of fragment_layout_kernel (agpu_ingest.hip:1475); "X,1" + ",1" vs "X" + ",1"
    inner_nul                  `abc\\0\\0\\0`: qname_length (ingest_core.hpp:259), name_key / qname_key128 (:272-287) stop at the first NUL, not at l_read_name
    (all)                      names in no order: the chunked string sort (names_were_sorted == 0)
  HI
    hi_C, hi_c, hi_c_negative, hi_s, hi_s_negative, hi_S, hi_i, hi_i_negative, hi_I, hi_I_above_2_31
                               the cases of scan_aux (ingest_core.hpp:224-231); decimal_digits (:976) with a sign and with ten digits; above 2^31: hit_index_to_keep ->
                               HIT_INDEX_UNKNOWN -> the second walk in hit_index_of (:244-248)
    hi_A, hi_Z, hi_f           `default: tags.hi = 0` (:231): the name ends in ",0"
    hi_mixed_types             one value, the types c C s S i I in turn over the records of a fragment: same_name / name_key on the value, not on the bytes
    two_hi_fields              the first HI counts (`!tags.has_hi`, :222)
    hi_behind_SA               the walk goes on behind SA (:235)
    hi_behind_B_<type>, hi_behind_B_count_0, hi_behind_A_f_d, hi_behind_Z, hi_behind_H
                               the sizes of the fields in front of HI (:207-218)
    decoy_in_Z, decoy_in_B     the bytes `HIC\\x05` and `SAZ` inside the value of another field: found only by a walk that loses its step
    secondary_without_hi       RECORD_MISSING_HI (agpu_ingest.hip:194) and the count of the reference's warning
  sequences
    odd_length_nibble          the unused low nibble of the last sequence byte set: `byte &= 0xF0` in write_fragment (ingest_core.hpp:1066)
  sizes
    record_20k, record_100k    records longer than a segment (the record chain: walk_segment, guess_segment, ingest_core.hpp:151-181) and than the margin of a window
                               (window_note, agpu_ingest.hip:858: the windows are abandoned); the 63 neighbours of record_20k are parsed from the stream
    piece_16384, piece_16385, piece_16384_plus_misalignment
                               `piece_end - piece_begin <= PARSE_WINDOW` (agpu_ingest.hip:176) on both sides of the border, and a piece that is too large only by the
                               bytes in front of its first record
    carrier                    two well-formed record headers at the start of an 8 KB segment, inside an array (repair_segment_run, ingest_core.hpp:187)

The reference (oracle/standin for htslib) refused none of the classes.
"""
import hashlib
import json
import os
import re
import struct

import pytest

import conftest
import datasets
import golden_io
import ingest_records_lib as lib
import parity

NAMES = sorted(lib.DATASETS)
SINGLE = ["length_1", "length_3", "inner_nul", "record_20k", "record_100k"] + ["length_%d" % n for n in lib.SPECIAL_LENGTHS]
DEALT = ["length_up_to_18", "length_19_to_68", "length_69_to_254", "comma", "prefix"] + ["difference_at_%d" % k for k in lib.DIFFERENCE_AT] + \
        ["hi_" + c for c in sorted(set(lib.HI_CLASSES))] + ["two_hi_fields", "hi_behind_SA", "hi_behind_B_count_0", "hi_behind_A_f_d", "hi_behind_Z", "hi_behind_H", "decoy_in_Z", "decoy_in_B", "odd_length_nibble"] + \
        ["hi_behind_B_" + t for t in lib.ARRAY_TYPES]
_cache = {}


@pytest.fixture(scope="module")
def dressed(built, tmp_path_factory):
    """name -> the re-dressed dataset: prefix of the files, the builder's table, the stream, the reference's read table and log"""
    def get(name):
        if name not in _cache:
            directory = str(tmp_path_factory.mktemp("dressed_" + name))
            base = datasets.generate(lib.DATASETS[name], directory, name="base")
            prefix, table = lib.write_dressed(base, os.path.join(directory, "dressed"))
            golden = os.path.join(conftest.ROOT, "tests", "golden", "ingest_records", name)
            stream = open(prefix + ".bam", "rb").read()
            assert hashlib.sha256(stream).hexdigest() == json.load(open(os.path.join(golden, "meta.json")))["bam_sha256"], "the re-dressed file drifted from tests/golden/ingest_records/%s; rerun tools/make_ingest_records_golden.py" % name
            _cache[name] = {"prefix": prefix, "table": table, "stream": stream, "golden": golden, "reads": golden_io.read_reads(golden_io.find_dump(golden, "reads", "annotated")),
                            "log": open(os.path.join(golden, "reference.log")).read()}
        return _cache[name]
    return get


def _host_batch(d):
    """the batch of the host ingest (computed once per dataset)"""
    import test_host_and_device_logic as cpu_tier
    if "host" not in d:
        host = parity.open_session(d["prefix"])
        columns = cpu_tier._batch_columns(host)
        columns["coverage"] = int(host._lib.ahost_coverage_checksum(host._session))
        d["host"] = (host, columns, host.detect_strandedness())
    return d["host"]


def _device_batch(d, api, path=None, piece_bytes=1 << 20):
    import test_host_and_device_logic as cpu_tier
    from arriba_amd.pipeline import DevicePipeline, HostSession
    session = HostSession(d["prefix"] + ".fa", d["prefix"] + ".gtf")
    pipeline = DevicePipeline(session, api=api, bam=path or d["prefix"] + ".bam", piece_bytes=piece_bytes)
    return session, pipeline, cpu_tier._device_batch_columns(session, pipeline)


def _logged(log, pattern):
    match = re.search(r"WARNING: (\d+) " + pattern, log)
    return int(match.group(1)) if match else 0


def check_rows_against_reference(pipeline, d, reads=None):
    """parity.check_ingest restated over the rows gathered from the device: names in order, n_aln, single-end, and per alignment strand, first-in-pair, supplementary,
    contig, start, end, CIGAR string and decoded sequence -- all exact; the two warnings of the reference's log"""
    rows, _ = pipeline.batch_rows()
    whole = reads is None
    reads = d["reads"] if whole else reads
    text, offsets = rows["names"].tobytes().decode("latin-1"), rows["name_offset"]
    names = [text[offsets[i]:offsets[i + 1]] for i in range(rows["n"])]
    assert len(names) == len(reads)
    different = [(i, a, b["name"]) for i, (a, b) in enumerate(zip(names, reads)) if a != b["name"]]
    assert not different, (len(different), different[:5])
    ops, codes = "MIDNSHP=XB", "=ACMGRSVTWYHKDBN"
    wrong = []
    for i, read in enumerate(reads):
        mine = [int(rows["n_aln"][i]), int(rows["fbits"][i]) & 1]
        theirs = [len(read["alignments"]), read["single_end"]]
        for slot, alignment in enumerate(read["alignments"]):
            bits = int(rows["abits%d" % slot][i])
            offset, count = int(rows["cigar_offset%d" % slot][i]), int(rows["cigar_count%d" % slot][i])
            mine += [bits & 1, (bits >> 1) & 1, (bits >> 2) & 1, int(rows["contig%d" % slot][i]), int(rows["start%d" % slot][i]), int(rows["end%d" % slot][i]),
                     "".join("%d%s" % (c >> 4, ops[c & 15]) for c in rows["cigar_pool"][offset:offset + count])]
            theirs += [alignment["strand"], alignment["first_in_pair"], alignment["supplementary"], alignment["contig"], alignment["start"], alignment["end"], alignment["cigar"]]
            if slot < 2:
                length, at = int(rows["seq_length%d" % slot][i]), int(rows["seq_offset%d" % slot][i]) * 4
                packed = rows["seq_pool"][at:at + (length + 1) // 2]
                if length & 1:
                    mine.append(int(packed[-1]) & 15)  # the unused nibble of the pool is zero, whatever the record holds
                    theirs.append(0)
                mine.append("".join(codes[(int(packed[b >> 1]) >> ((~b & 1) << 2)) & 15] for b in range(length)))
                theirs.append(alignment["sequence"])
        if mine != theirs:
            wrong.append((read["name"], [(a, b) for a, b in zip(mine, theirs) if a != b][:3]))
    assert not wrong, (len(wrong), wrong[:5])
    result = pipeline.ingest_result
    if not whole:  # (some names of the file were left out: the counts of the log are not this file's)
        return len(reads)
    assert int(result.missing_hi_tag) == _logged(d["log"], "secondary alignments lack the 'HI' tag")
    assert int(result.malformed_count) == _logged(d["log"], "SAM records were malformed")
    return len(reads)


def check_device_ingest(d, api):
    """one ingest on the device (harness or kernels): the reference's read table, the host ingest's batch"""
    host, expected, strandedness = _host_batch(d)
    session, pipeline, columns = _device_batch(d, api)
    assert check_rows_against_reference(pipeline, d) >= 2000
    different = [key for key in expected if expected[key] != columns[key]]
    assert not different, different
    assert pipeline.ingest_result.names_were_sorted == 0
    assert pipeline.detect_strandedness() == strandedness
    return columns


def check_verdicts_on_the_order_of_the_names(d, api, directory):
    """The dress comes in no order, so that the string sort runs -- and whatever compare_names says about two neighbours, some other pair is out of order.  Here its
    verdict decides.  The same records with their names ascending: names_were_sorted == 1 (no neighbour judged out of order, whatever the lengths and the alignment
    of the two names), with the commas (the first-occurrence fast path of fragment_layout_kernel must stand back: IC_QNAME_COMMA) and without them (it runs).  Then
    one pair of neighbours exchanged -- a name and its proper prefix, names that first differ at byte 6 .. 16: were that pair judged in order, the batch would be out
    of order.  The reference keeps its reads in a std::map: its read table is that of the dressed file (checked once against a run of the reference)."""
    stream, runs = d["stream"], lib.name_runs(d["stream"])
    fragments = {lib.fragment_qname(read["name"]) for read in d["reads"]}
    without_commas = [read for read in d["reads"] if "," not in lib.fragment_qname(read["name"])]
    assert len(d["reads"]) - 10 >= len(without_commas) >= 2000
    path = os.path.join(directory, "ordered.bam")

    def ingest(variant):
        with open(path, "wb") as out:
            out.write(variant)
        return _device_batch(d, api, path)[1]
    pipeline = ingest(lib.in_name_order(stream, runs))
    assert pipeline.ingest_result.names_were_sorted == 1
    check_rows_against_reference(pipeline, d, reads=d["reads"])
    pipeline = ingest(lib.in_name_order(stream, runs, without_commas=True))
    assert pipeline.ingest_result.names_were_sorted == 1
    check_rows_against_reference(pipeline, d, reads=without_commas)
    for kind in ["prefix"] + ["difference_at_%d" % k for k in lib.DIFFERENCE_AT]:
        variants = (lib.in_name_order(stream, runs, without_commas=True, swap=pair) for pair in d["table"][kind + "_pairs"] if pair[0] in fragments and pair[1] in fragments)
        pipeline = ingest(next(variant for variant in variants if variant is not None))
        assert pipeline.ingest_result.names_were_sorted == 0, kind
        check_rows_against_reference(pipeline, d, reads=without_commas)


def false_start_file(d, directory):
    """the stream with nothing but the carrier of the two false record starts in a new place (as test_device_ingest_survives_a_false_record_start builds it): a second
    carrier, so that the repair pass has two runs of segments to settle"""
    stream = d["stream"]
    base = lib.first_record_offset(stream)
    cut = base
    while cut < base + 100000:
        cut += 4 + struct.unpack_from("<I", stream, cut)[0]
    fake = struct.pack("<IiiBBHHHiiii", 40, 0, 5, 2, 0, 0, 0, 0, 0, -1, -1, 0) + b"y\0" + b"\0" * 6
    carrier_head = 4 + 32 + 2 + 8
    pad = (base - cut - carrier_head) % lib.SEGMENT_BYTES
    body = b"\xAA" * pad + fake + fake + b"\xFF" * 64
    carrier = struct.pack("<iiBBHHHiiii", -1, -1, 2, 0, 0, 0, 4, 0, -1, -1, 0) + b"x\0" + b"ZZBC" + struct.pack("<I", len(body)) + body
    assert (cut + carrier_head + pad - base) % lib.SEGMENT_BYTES == 0
    path = os.path.join(directory, "false_start.bam")
    with open(path, "wb") as out:
        out.write(stream[:cut] + struct.pack("<I", len(carrier)) + carrier + stream[cut:])
    return path


# ---- CPU tier ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_dress_holds_every_class_among_the_fragments_of_the_reference(name, dressed):
    """nothing passes by being absent: every class of the dress is counted among the fragments of the reference's read table (and the secondaries it skipped), the
    sizes are recomputed from the record offsets"""
    d = dressed(name)
    table, stream = d["table"], d["stream"]
    fragments = {lib.fragment_qname(read["name"]) for read in d["reads"]}
    assert len(d["reads"]) >= 2000
    counts = {key: len(fragments.intersection(table.get(key, ()))) for key in SINGLE + DEALT}
    print(name, counts)
    assert all(counts[key] >= 1 for key in SINGLE), {key: counts[key] for key in SINGLE}
    assert all(counts[key] >= 10 for key in DEALT), {key: counts[key] for key in DEALT if counts[key] < 10}
    assert {"X", "X,1"} <= fragments and "abc" in fragments
    for kind in ["prefix"] + ["difference_at_%d" % k for k in lib.DIFFERENCE_AT]:
        pairs = [pair for pair in table[kind + "_pairs"] if pair[0] in fragments and pair[1] in fragments]
        assert len(pairs) >= 10, (kind, len(pairs))
        for a, b in pairs:
            if kind == "prefix":
                assert b.startswith(a) and len(b) > len(a)
            else:
                assert len(a) == len(b) and [i for i in range(len(a)) if a[i] != b[i]][0] == int(kind.rsplit("_", 1)[1])
    if name == "odd_length3k":
        missing = _logged(d["log"], "secondary alignments lack the 'HI' tag")
        assert missing >= 10 and len(table["secondary_without_hi"]) >= 10
    assert _logged(d["log"], "SAM records were malformed") >= 1
    # names, alignments and sizes as the records of the stream have them
    records = lib.parse_records(stream)
    of_fragments = [r for r in records if lib.qname_of(r).decode("latin-1") in fragments]
    assert {len(r["name"]) % 4 for r in of_fragments} == {0, 1, 2, 3} and {r["offset"] % 16 for r in of_fragments} == set(range(16))
    assert {len(lib.qname_of(r)) for r in of_fragments} >= {1, 2, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 253, 254}
    assert any(r["name"] == b"abc\0\0\0" for r in of_fragments)
    order = [lib.qname_of(r) for r in records]
    assert order != sorted(order)
    size = {lib.qname_of(r).decode("latin-1"): 0 for r in records}
    for r, following in zip(records, records[1:] + [{"offset": len(stream)}]):
        size[lib.qname_of(r).decode("latin-1")] = max(size[lib.qname_of(r).decode("latin-1")], following["offset"] - r["offset"])
    assert 2 * lib.SEGMENT_BYTES < size[table["record_20k"][0]] < 32768 and size[table["record_100k"][0]] > 100 * 1024
    if name == "odd_length3k":
        nibbles = [r for r in of_fragments if r["l_seq"] & 1 and r["body"][4 * r["n_cigar"] + (r["l_seq"] + 1) // 2 - 1] & 15]
        assert len(nibbles) >= 1000
    pieces = lib.piece_sizes(stream)
    layout = table["layout"]
    assert pieces[layout["piece_16384"] // 64][0] == lib.PARSE_WINDOW
    assert pieces[layout["piece_16385"] // 64][0] == lib.PARSE_WINDOW + 1
    piece, misalignment = pieces[layout["piece_16384_plus_misalignment"] // 64]
    assert misalignment > 0 and piece == lib.PARSE_WINDOW + misalignment
    in_lds = sum(1 for piece, _ in pieces if piece <= lib.PARSE_WINDOW)
    assert in_lds >= 50 and len(pieces) - in_lds >= 4, (in_lds, len(pieces))  # both branches of record_parse_kernel get whole groups: at least the four built to be too large
    big = next(i for i, r in enumerate(records) if lib.qname_of(r).decode() == table["record_20k"][0] and len(r["aux"]) > 20000)
    group = pieces[big // 64]
    assert group[0] > lib.PARSE_WINDOW and group[0] - size[table["record_20k"][0]] < lib.PARSE_WINDOW  # an otherwise small group
    carrier = records[layout["carrier"]]
    assert carrier["name"] == b"x\0" and carrier["flag"] == 4
    at = stream.index(struct.pack("<IiiBB", 40, 0, 5, 2, 0), carrier["offset"])
    assert (at - lib.first_record_offset(stream)) % lib.SEGMENT_BYTES == 0 and at + 88 < carrier["offset"] + 4 + struct.unpack_from("<I", stream, carrier["offset"])[0]


@pytest.mark.parametrize("name", NAMES)
def test_host_ingest_reads_the_dressed_records_as_the_reference(name, dressed):
    d = dressed(name)
    host, columns, _ = _host_batch(d)
    assert parity.check_ingest(host, d["golden"]) >= 2000


@pytest.mark.parametrize("name", NAMES)
def test_device_logic_reads_the_dressed_records_as_the_reference(name, dressed, emu_api):
    check_device_ingest(dressed(name), emu_api)


def test_device_logic_survives_false_record_starts_among_dressed_records(dressed, emu_api, tmp_path):
    d = dressed("plain3k")
    expected = check_device_ingest(d, emu_api)
    assert _device_batch(d, emu_api, false_start_file(d, str(tmp_path)))[2] == expected


def test_device_logic_judges_the_order_of_dressed_names(dressed, emu_api, tmp_path):
    check_verdicts_on_the_order_of_the_names(dressed("plain3k"), emu_api, str(tmp_path))


# ---- GPU tier ----------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_device_ingest_reads_the_dressed_records_as_the_reference(name, dressed):
    check_device_ingest(dressed(name), None)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_device_ingest_of_dressed_records_in_every_container_and_window(name, dressed, tmp_path, monkeypatch):
    """the same stream raw, as stored and as deflated BGZF, and the front of the ingest in one window, behind the last piece, and in windows of 1 MB that end 64 KB
    or one byte in front of what has arrived: the same batch every time"""
    import test_host_and_device_logic as cpu_tier
    d = dressed(name)
    monkeypatch.delenv("ARRIBA_INGEST_WINDOWS", raising=False)
    expected = _device_batch(d, None)[2]
    host_columns = _host_batch(d)[1]
    assert [key for key in host_columns if host_columns[key] != expected[key]] == [] and expected["n"] >= 2000
    for container, level in (("stored", 0), ("deflated", 6)):
        path = str(tmp_path / (container + ".bam"))
        cpu_tier._write_bgzf(path, d["stream"], level)
        assert _device_batch(d, None, path)[2] == expected, container
    # pieces (of a raw file: so many bytes of the stream each) of which one ends inside the 100 KB record, 74-90 KB behind its start: the window made then ends 64 KB in
    # front of the piece's end -- behind the start of the record -- and its chain cannot follow the record to its end (walk_segment: OFFSET_BROKEN).  window_note
    # abandons the windows, agpu_ingest_finish does the whole stream the other way and reports no window.
    records = lib.parse_records(d["stream"])
    start = next(r["offset"] for r in records if len(r["aux"]) > 100 * 1024)
    pieces = (start + 90 * 1024) >> 20
    straddling = (start + 90 * 1024) // pieces & ~4095
    assert 1 <= pieces <= 4 and straddling >= 1 << 20 and start + 73 * 1024 < pieces * straddling < start + 100 * 1024
    for knob, piece_bytes in (("0", 1 << 20), ("1048576,65536", 1 << 20), ("1048576,1", 1 << 20), ("1048576,65536", straddling)):
        monkeypatch.setenv("ARRIBA_INGEST_WINDOWS", knob)
        session, pipeline, columns = _device_batch(d, None, piece_bytes=piece_bytes)
        assert columns == expected, (knob, piece_bytes)
        print(name, "ARRIBA_INGEST_WINDOWS=" + knob, "pieces of", piece_bytes, "windows:", pipeline.ingest_result.windows)
        if piece_bytes != 1 << 20:
            assert pipeline.ingest_result.windows == 0
        if knob == "0":
            assert pipeline.ingest_result.windows == 0


@pytest.mark.gpu
def test_device_ingest_survives_false_record_starts_among_dressed_records(dressed, tmp_path):
    """test_device_ingest_survives_a_false_record_start on the kernels (batch equality only: the count of repair passes is a hook of the harness)"""
    d = dressed("plain3k")
    expected = _device_batch(d, None)[2]
    assert expected["n"] >= 2000 and _device_batch(d, None, false_start_file(d, str(tmp_path)))[2] == expected


@pytest.mark.gpu
def test_device_ingest_judges_the_order_of_dressed_names(dressed, tmp_path):
    check_verdicts_on_the_order_of_the_names(dressed("plain3k"), None, str(tmp_path))
