"""--mark-duplicates: flag 0x400 of the records of --sorted-bam set on duplicate templates and cleared on all others (the rule: DESIGN.md 4.14 -- Picard's for one library without
optical duplicates and UMIs).

Neither Picard nor samtools is here to test against; the rule is the project's specification.  tests/golden/mark_duplicates/hand_made.sam and .expected (QNAME, tab, 0 or 1) are a
pair worked out by hand, one small group per case of the rule; tests/markdup_lib.py restates the rule in plain Python dicts, test_restatement_equals_the_committed_file holds it to
that pair, and only therefore it is the independent side for inputs made at test time.  The CPU tier runs arriba_amd/csrc/device/markdup_core.hpp stepped on the host
(ahost_markdup, ahost_sorted_bam_file_marked); the GPU tier the kernels of agpu_markdup.hip and the patch in the gather of agpu_sorted_bam.hip, whose BAM and BAI files must equal
the host's byte for byte.  All expectations are exact."""
import ctypes
import gzip
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import conftest
import markdup_lib as lib

GOLDEN = os.path.join(conftest.ROOT, "tests", "golden", "mark_duplicates")
WORKFLOW = os.path.join(conftest.ROOT, "arriba_amd", "lib", "arriba_gpu_workflow")
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
SEEDED = ["seed%d" % (2000 + k) for k in range(50)]
PAYLOAD, BLOCK = 0xff00, 0xff00 + 31
COUNTED = ("templates", "pairs", "fragments", "duplicate_pairs", "duplicate_fragments", "records_flagged", "records_changed")
KERNELS = ("markdup_name_kernel", "markdup_end_kernel", "markdup_template_kernel", "markdup_flag_kernel")


def _golden(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


def _write_bgzf(path, payload, level=0):
    with open(path, "wb") as out:
        for at in range(0, len(payload), PAYLOAD):
            piece = payload[at:at + PAYLOAD]
            deflater = zlib.compressobj(level, zlib.DEFLATED, -15)
            body = deflater.compress(piece) + deflater.flush()
            out.write(struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(body) + 25) + body + struct.pack("<II", zlib.crc32(piece), len(piece)))
        out.write(EOF_BLOCK)


def _hot_bytes(case):
    """the records of the hot case without 210 000 calls of the record writer: three kinds of records that differ in their names and qualities only"""
    references, records = case
    made = {}
    out = []
    for record in records:
        kind = (record["flag"], record["qual"])
        if kind not in made:
            made[kind] = lib.bam_record(references, record)
        template = made[kind]
        out.append(template[:36] + record["qname"].encode() + template[36 + len(record["qname"]):])
    return b"".join(out)


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """name -> (case, path of its input BAM file, marks of the restatement per record): made once"""
    directory = tmp_path_factory.mktemp("markdup_inputs")
    cache = {}

    def get(name):
        if name not in cache:
            record_bytes = None
            if name == "hand_made":
                case = lib.parse_sam(_golden("hand_made.sam"))
            elif name == "hot":
                case, survivor = lib.hot_case()
                record_bytes = _hot_bytes(case)
            elif name == "one_record":
                case = lib.one_record_case()
            elif name == "unmapped":
                case = lib.unmapped_case()
            elif name.startswith("straddle"):
                case, number = lib.straddle_case(int(name[8:], 16))
            else:
                case = lib.random_case(int(name[4:]))
            if record_bytes is None:
                record_bytes = lib.bam_records(case)
            path = str(directory / (name + ".bam"))
            _write_bgzf(path, lib.bam_header(case[0]) + record_bytes)
            cache[name] = (case, path, lib.restate(case), record_bytes)
        return cache[name]
    return get


def _host():
    from arriba_amd import _capi
    return _capi, _capi.host_library()


def _host_marks(record_bytes, n_records):
    from arriba_amd.pipeline import markdup_counts_of
    _capi, host = _host()
    flags, counts = np.zeros(max(n_records, 1), np.uint8), _capi.MarkdupCounts()
    assert host.ahost_markdup(record_bytes, len(record_bytes), flags.ctypes.data, n_records, ctypes.byref(counts)) == 0, host.ahost_last_error()
    return [int(flag) for flag in flags[:n_records]], markdup_counts_of(counts)


@pytest.fixture(scope="module")
def host_files(cases, tmp_path_factory):
    """(name, level, marked) -> path of the file of ahost_sorted_bam_file_marked (with its .bai): made once, compared against by every test"""
    directory = tmp_path_factory.mktemp("markdup_host")
    cache = {}

    def get(name, level=0, marked=True):
        key = (name, level, marked)
        if key not in cache:
            _capi, host = _host()
            path = str(directory / ("%s.%d.%d.bam" % key))
            assert host.ahost_sorted_bam_file_marked(cases(name)[1].encode(), path.encode(), level, int(marked), None) == 0, host.ahost_last_error()
            cache[key] = path
        return cache[key]
    return get


def _same_files(path, expected):
    assert open(path, "rb").read() == open(expected, "rb").read(), path
    assert open(path + ".bai", "rb").read() == open(expected + ".bai", "rb").read(), path


def _marks_of_file(path):
    """QNAME -> set of the 0x400 bits of its records in the file"""
    marks = {}
    for _, qname, flag in lib.file_records(open(path, "rb").read()):
        marks.setdefault(qname, set()).add(1 if flag & lib.DUPLICATE else 0)
    return marks


# ---- CPU tier -----------------------------------------------------------------------------------------------------------------------------------------------------

def _expected():
    return dict((line.split("\t")[0], int(line.split("\t")[1])) for line in _golden("hand_made.expected").decode().split("\n") if line)


def test_restatement_equals_the_committed_file():
    """the restatement of the rule against the pair that was worked out by hand"""
    case = lib.parse_sam(_golden("hand_made.sam"))
    expected = _expected()
    assert set(expected) == set(record["qname"] for record in case[1]) and len(case[1]) == 77
    duplicates = lib.duplicate_names(case)
    assert {qname: int(qname in duplicates) for qname in expected} == expected
    # the two mates of p16a lie more than 40 records apart; input marks are on survivors and on duplicates
    numbers = [k for k, record in enumerate(case[1]) if record["qname"] == "p16a"]
    assert numbers[1] - numbers[0] >= 40
    marked_in_input = set(record["qname"] for record in case[1] if record["flag"] & lib.DUPLICATE)
    assert {expected[qname] for qname in marked_in_input} == {0, 1}


def test_host_gives_the_committed_marks(built, cases):
    case, path, restated, record_bytes = cases("hand_made")
    marks, counts = _host_marks(record_bytes, len(case[1]))
    expected = _expected()
    assert [mark // 4 for mark in marks] == [expected[record["qname"]] for record in case[1]] and set(marks) == {0, 4}
    assert {key: counts[key] for key in ("templates", "records_flagged", "records_changed")} == lib.counts(case)
    assert counts["templates"] == 57 and counts["pairs"] == 12 and counts["fragments"] == 42 and counts["duplicate_pairs"] == 5 and counts["duplicate_fragments"] == 22


@pytest.mark.parametrize("name", ["seeded", "hot", "one_record", "unmapped"])
def test_host_equals_the_restatement(name, built, cases):
    flagged = 0
    for each in (SEEDED if name == "seeded" else [name]):
        case, path, restated, record_bytes = cases(each)
        marks, counts = _host_marks(record_bytes, len(case[1]))
        assert [mark // 4 for mark in marks] == restated, each
        assert {key: counts[key] for key in ("templates", "records_flagged", "records_changed")} == lib.counts(case), each
        flagged += counts["records_flagged"]
        if name == "seeded":
            assert 200 <= len(case[1]) <= 400 and counts["duplicate_pairs"] > 0 and counts["duplicate_fragments"] > 0, each
    if name == "hot":
        survivor = lib.hot_case()[1]
        assert counts["pairs"] == counts["fragments"] == 70001 and counts["duplicate_pairs"] == 70000 and counts["duplicate_fragments"] == 70001
        assert [record["qname"] for record, mark in zip(case[1], marks) if not mark] == [survivor, survivor]
    if name in ("one_record", "unmapped"):
        assert flagged == 0 and counts["records_changed"] == (2 if name == "unmapped" else 0)


def _blocks_of(path):
    data = open(path, "rb").read()
    payload, blocks = lib.inflate_bgzf(data)
    return data, payload, blocks


@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("name", ["hand_made", "seed2000", "straddlefeff", "straddleff00"])
def test_invariants_of_the_output_file(name, level, built, cases, host_files):
    """the index is that of the run without the option; the inflated payloads differ only in mask 0x04 of byte 19 of records; every CRC is that of its payload; the marks in the
    file are those of the restatement"""
    case, path, restated, record_bytes = cases(name)
    marked, plain = host_files(name, level, True), host_files(name, level, False)
    if level == 0:  # (deflated blocks have sizes of their own, and the virtual offsets of the index follow them: only stored files share their index)
        assert open(marked + ".bai", "rb").read() == open(plain + ".bai", "rb").read()
    _, payload, blocks = _blocks_of(marked)
    _, plain_payload, _ = _blocks_of(plain)
    for piece, (crc, size) in blocks:
        assert zlib.crc32(piece) == crc and len(piece) == size
    assert len(payload) == len(plain_payload)
    flag_bytes = set(at + 19 for at, _, _ in lib.file_records(open(plain, "rb").read()))
    different = [at for at in np.flatnonzero(np.frombuffer(payload, np.uint8) != np.frombuffer(plain_payload, np.uint8))]
    assert set(different) <= flag_bytes and all((payload[at] ^ plain_payload[at]) == 0x04 for at in different)
    assert len(different) == lib.counts(case)["records_changed"] > 0
    duplicates = lib.duplicate_names(case)
    assert _marks_of_file(marked) == {record["qname"]: {int(record["qname"] in duplicates)} for record in case[1]}
    if level == 0 and not name.startswith("straddle"):  # the plain file is the file of the entry that has no marks
        _capi, host = _host()
        assert host.ahost_sorted_bam_file_level(path.encode(), (plain + ".again").encode(), 0, None) == 0
        assert open(plain + ".again", "rb").read() == open(plain, "rb").read()
    if name.startswith("straddle"):  # byte 19 of a duplicate record is the last payload byte of the first block / the first of the second
        target = int(name[8:], 16)
        records = lib.file_records(open(marked, "rb").read())
        stream_begin = records[0][0]  # (the header has a block of its own: the first record begins the second block)
        assert stream_begin == len(blocks[0][0]) < PAYLOAD
        hit = [flag for at, qname, flag in records if at - stream_begin + 19 == target]
        assert len(hit) == 1 and hit[0] & lib.DUPLICATE
        assert len(blocks) >= 3 and len(blocks[1][0]) == PAYLOAD


def _harness(target):
    directory = os.path.join(conftest.ROOT, "tests", "emu")
    subprocess.run(["make", "-s", "-C", directory, target], check=True)
    return os.path.join(directory, target)


def test_host_ingest_through_the_command_line(built, emu_api, dataset_files, cases, tmp_path):
    """--host-ingest --sorted-bam --mark-duplicates: the C++ driver (over the host stepping harness, where there is no GPU) writes the file of ahost_sorted_bam_file_marked, the log
    line, and the fusions of the run without the option"""
    prefix = dataset_files("toy3k")
    _capi, host = _host()
    expected = str(tmp_path / "expected.bam")
    assert host.ahost_sorted_bam_file_marked((prefix + ".bam").encode(), expected.encode(), 0, 1, None) == 0, host.ahost_last_error()
    command = [_harness("workflow_on_harness"), "-x", prefix + ".bam", "-g", prefix + ".gtf", "-a", prefix + ".fa", "-o", str(tmp_path / "fusions.tsv"), "-f", "blacklist", "--host-ingest", "--sorted-bam", str(tmp_path / "sorted.bam"), "--mark-duplicates"]
    result = subprocess.run(command, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert result.returncode == 0, result.stderr[-2000:]
    _same_files(str(tmp_path / "sorted.bam"), expected)
    assert "Marking duplicates in the sorted BAM file (templates=" in result.stdout and "records_flagged=" in result.stdout
    assert open(str(tmp_path / "fusions.tsv")).read() == gzip.open(os.path.join(conftest.golden_dir("toy3k"), "fusions.tsv.gz"), "rt").read()


def test_cpp_driver_on_the_harness_says_that_it_has_no_device_library(built, emu_api, dataset_files, tmp_path):
    """the test-only build of the C++ driver against the host stepping harness has no twin of the kernels of agpu_markdup.hip: it links all the same and says so before the feed"""
    prefix = dataset_files("toy3k")
    command = [_harness("workflow_on_harness"), "-x", prefix + ".bam", "-g", prefix + ".gtf", "-a", prefix + ".fa", "-o", str(tmp_path / "fusions.tsv"), "-f", "blacklist", "--sorted-bam", str(tmp_path / "sorted.bam"), "--mark-duplicates"]
    result = subprocess.run(command, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert result.returncode != 0 and "--mark-duplicates needs the device library (agpu_sorted_bam_set_mark_duplicates)" in result.stderr
    assert os.listdir(str(tmp_path)) == []


def _refused(arguments):
    result = subprocess.run(["timeout", "-k", "10", "60", WORKFLOW] + arguments, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert result.returncode not in (0, 124, 137), result.stderr[-2000:]
    return result.stderr


def test_command_line_refusals(built, dataset_files, tmp_path):
    prefix = dataset_files("toy3k")
    common = ["-x", prefix + ".bam", "-g", prefix + ".gtf", "-a", prefix + ".fa", "-o", str(tmp_path / "fusions.tsv"), "-f", "blacklist"]
    assert "--mark-duplicates needs --sorted-bam" in _refused(common + ["--mark-duplicates"])
    assert "--mark-duplicates and -u exclude each other" in _refused(common + ["--sorted-bam", str(tmp_path / "out.bam"), "--mark-duplicates", "-u"])
    assert not os.listdir(str(tmp_path))
    usage = subprocess.run([WORKFLOW, "-h"], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True).stdout
    assert "--mark-duplicates" in usage


def test_refusals_of_the_session_come_before_the_feed(built, emu_api, dataset_files, tmp_path):
    """the driver itself (over the harness) refuses the option without a sorted file and together with -u before a byte of the file is read"""
    from arriba_amd import _capi
    prefix = dataset_files("toy3k")
    driver = ctypes.CDLL(_harness("libworkflow_on_harness.so"))
    driver.arriba_workflow_open.restype = ctypes.c_void_p
    driver.arriba_workflow_last_error.restype = ctypes.c_char_p
    for with_u, wanted in ((False, "--mark-duplicates needs --sorted-bam"), (True, "--mark-duplicates and -u exclude each other")):
        options = _capi.WorkflowOptions()
        driver.arriba_workflow_default_options(ctypes.byref(options))
        options.assembly_file, options.gene_annotation_file = (prefix + ".fa").encode(), (prefix + ".gtf").encode()
        options.device.external_duplicate_marking = int(with_u)
        session = ctypes.c_void_p(driver.arriba_workflow_open(ctypes.byref(options)))
        assert session, driver.arriba_workflow_last_error()
        assert driver.arriba_workflow_sorted_bam_mark_duplicates(session, 1) == 0
        if with_u:
            assert driver.arriba_workflow_sorted_bam(session, str(tmp_path / "sorted.bam").encode()) == 0
        status = driver.arriba_workflow_sample(session, str(tmp_path / "no_such_file.bam").encode(), str(tmp_path / "fusions.tsv").encode(), None, None, None)
        message = driver.arriba_workflow_last_error().decode()
        driver.arriba_workflow_close(session)
        assert status != 0 and wanted in message, message
    assert os.listdir(str(tmp_path)) == []


# ---- GPU tier -----------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pipeline(dataset_files):
    """one device pipeline on the reference data of toy3k for every case that is ingested here (the contigs of a case join those of the session)"""
    from arriba_amd.pipeline import DevicePipeline, HostSession
    prefix = dataset_files("toy3k")
    made = DevicePipeline(HostSession(prefix + ".fa", prefix + ".gtf", interesting_contigs="1 2 3 4"), bam=prefix + ".bam")
    yield made
    made.close()


KNOBS = [{}, {"ARRIBA_MARKDUP_HASH_BITS": "4"}, {"ARRIBA_SORTED_BAM_WINDOW": str(BLOCK)}, {"ARRIBA_WAVE_CHUNK": "16"}, {"compression": 1}]
SMALL = ["hand_made", "one_record", "unmapped", "straddlefeff", "straddleff00"]


def _device_file(pipeline, cases, name, path, compression=0):
    pipeline._ingest_records(cases(name)[1], False, 100, 64 << 20)  # (without the host's "no normal reads found": the stream is what matters here)
    written = pipeline.write_sorted_bam(path, compression=compression, mark_duplicates=True)
    assert pipeline.markdup_allocated_bytes() == 0 and not os.path.exists(path + ".tmp")
    return written, pipeline.markdup_counts


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["small", "seeded"])
@pytest.mark.parametrize("knobs", KNOBS, ids=["no_knobs", "hash_bits_4", "window_of_one_block", "wave_chunk_16", "compression_1"])
def test_device_file_is_the_host_file(knobs, group, built, pipeline, cases, host_files, tmp_path, monkeypatch):
    """BAM and BAI of agpu_sorted_bam_* with the marks on equal the host stepping's byte for byte and the counts are equal: the committed case, a file of one record, a file with
    no mapped record, the two straddle files; 50 seeded inputs; with four bits of the hash (every probe run is long and every hit is decided by the bytes); with windows of a single
    block; with wave chunks of 16; at compression level 1, which must inflate to the stored payload"""
    for knob in ("ARRIBA_MARKDUP_HASH_BITS", "ARRIBA_SORTED_BAM_WINDOW", "ARRIBA_WAVE_CHUNK"):
        if knob in knobs:
            monkeypatch.setenv(knob, knobs[knob])
        else:
            monkeypatch.delenv(knob, raising=False)
    level = knobs.get("compression", 0)
    for name in (SMALL if group == "small" else SEEDED):
        case, sample, restated, record_bytes = cases(name)
        path = str(tmp_path / (name + ".bam"))
        written, counts = _device_file(pipeline, cases, name, path, level)
        _same_files(path, host_files(name, level))
        host_counts = _host_marks(record_bytes, len(case[1]))[1]
        print(name, {key: counts[key] for key in COUNTED + ("peak_bytes",)})
        assert {key: counts[key] for key in COUNTED} == {key: host_counts[key] for key in COUNTED}, name
        assert counts["peak_bytes"] > 0, name
        if "ARRIBA_SORTED_BAM_WINDOW" in knobs:
            assert written["windows"] == (len(record_bytes) + PAYLOAD - 1) // PAYLOAD, name
        if level == 1:
            assert lib.inflate_bgzf(open(path, "rb").read())[0] == lib.inflate_bgzf(open(host_files(name, 0), "rb").read())[0], name
        if name == "hand_made":
            expected = _expected()
            assert _marks_of_file(path) == {qname: {mark} for qname, mark in expected.items()}


@pytest.mark.gpu
def test_hot_key_leaves_exactly_one_template(built, pipeline, cases, host_files, tmp_path):
    """70 001 pairs at one key plus 70 001 fragments on its forward end"""
    case, sample, restated, record_bytes = cases("hot")
    path = str(tmp_path / "hot.bam")
    written, counts = _device_file(pipeline, cases, "hot", path)
    _same_files(path, host_files("hot"))
    assert counts["pairs"] == counts["fragments"] == 70001 and counts["duplicate_pairs"] == 70000 and counts["duplicate_fragments"] == 70001 and counts["records_flagged"] == 3 * 70001 - 2
    survivors = [qname for qname, marks in _marks_of_file(path).items() if marks != {1}]
    assert survivors == [lib.hot_case()[1]]


@pytest.mark.gpu
def test_off_means_off(built, dataset_files, host_files, cases, tmp_path):
    """with the option off no kernel of agpu_markdup.hip is in the kernel profile, no buffer of it exists and the file is the file without marks; with it on they are there, and
    the option holds for one begin ... end"""
    from arriba_amd.pipeline import DevicePipeline, HostSession
    prefix = dataset_files("toy3k")
    made = DevicePipeline(HostSession(prefix + ".fa", prefix + ".gtf"), bam=prefix + ".bam")
    made.set_profiling(True)
    made.read_chimeric_alignments(prefix + ".bam")
    made.write_sorted_bam(str(tmp_path / "off.bam"))
    names = {launch[0] for launch in made.kernel_profile()}
    assert "sorted_bam_gather_kernel" in names and not [name for name in names if name.startswith("markdup")] and made.markdup_allocated_bytes() == 0
    made.write_sorted_bam(str(tmp_path / "on.bam"), mark_duplicates=True)
    names = {launch[0] for launch in made.kernel_profile()}
    assert set(KERNELS) <= names and made.markdup_allocated_bytes() == 0 and made.markdup_counts["templates"] > 1000
    made.write_sorted_bam(str(tmp_path / "again.bam"))
    _same_files(str(tmp_path / "again.bam"), str(tmp_path / "off.bam"))
    _capi, host = _host()
    for marked, name in ((0, "off.bam"), (1, "on.bam")):
        expected = str(tmp_path / ("host_" + name))
        assert host.ahost_sorted_bam_file_marked((prefix + ".bam").encode(), expected.encode(), 0, marked, None) == 0, host.ahost_last_error()
        _same_files(str(tmp_path / name), expected)
    # behind a begin, the switch is refused
    info = _capi.SortedBamInfo()
    made._check(made.api.sorted_bam_begin(made.ctx, ctypes.byref(info)))
    assert made.api.sorted_bam_set_mark_duplicates(made.ctx, 1) != 0 and b"it comes before agpu_sorted_bam_begin" in made.api.last_error()
    made._check(made.api.sorted_bam_end(made.ctx))
    made.close()


def _command_line(sample, prefix, outputs, extra):
    command = [WORKFLOW, "-x", sample, "-g", prefix + ".gtf", "-a", prefix + ".fa", "-o", outputs[0], "-O", outputs[1], "-f", "blacklist"]
    return subprocess.run(["timeout", "-k", "10", "120"] + command + extra, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)


@pytest.fixture(scope="module")
def without_the_option(dataset_files, tmp_path_factory):
    """fusions.tsv and discarded.tsv of toy3k from a run of the command line without --mark-duplicates"""
    directory = tmp_path_factory.mktemp("plain")
    outputs = [str(directory / "fusions.tsv"), str(directory / "discarded.tsv")]
    result = _command_line(dataset_files("toy3k") + ".bam", dataset_files("toy3k"), outputs, ["--sorted-bam", str(directory / "sorted.bam")])
    assert result.returncode == 0, result.stderr[-2000:]
    return [open(path, "rb").read() for path in outputs] + [str(directory / "sorted.bam")]


@pytest.mark.gpu
def test_command_line_writes_the_file_and_the_log_line(built, dataset_files, without_the_option, tmp_path):
    """toy3k: the marked file of the host stepping, its index that of the run without the option, the counts in the log; fusions.tsv and discarded.tsv are byte-identical with and
    without the option"""
    prefix = dataset_files("toy3k")
    outputs = [str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv")]
    result = _command_line(prefix + ".bam", prefix, outputs, ["--sorted-bam", str(tmp_path / "sorted.bam"), "--mark-duplicates"])
    assert result.returncode == 0, result.stderr[-2000:]
    _capi, host = _host()
    counts = _capi.MarkdupCounts()
    assert host.ahost_sorted_bam_file_marked_counts((prefix + ".bam").encode(), str(tmp_path / "host.bam").encode(), 0, 1, None, ctypes.byref(counts)) == 0, host.ahost_last_error()
    _same_files(str(tmp_path / "sorted.bam"), str(tmp_path / "host.bam"))
    line = "Marking duplicates in the sorted BAM file (templates=%d, pairs=%d, fragments=%d, duplicate_pairs=%d, duplicate_fragments=%d, records_flagged=%d, records_changed=%d)" % tuple(getattr(counts, key) for key in COUNTED)
    assert line in result.stdout
    assert [open(path, "rb").read() for path in outputs] == without_the_option[:2]
    assert open(str(tmp_path / "sorted.bam.bai"), "rb").read() == open(without_the_option[2] + ".bai", "rb").read()
    assert sorted(os.listdir(str(tmp_path))) == ["discarded.tsv", "fusions.tsv", "host.bam", "host.bam.bai", "sorted.bam", "sorted.bam.bai"]


@pytest.mark.gpu
def test_session_of_two_lanes_with_the_option_per_sample(built, dataset_files, without_the_option, tmp_path):
    """the option on for one sample and off for the next: each file is the host's, and no buffer of the option is left on either lane"""
    from arriba_amd.pipeline import WorkflowSession
    prefix = dataset_files("toy3k")
    session = WorkflowSession(prefix + ".fa", prefix + ".gtf", params={"disable_filters": ["blacklist"]})
    session.submit(prefix + ".bam", sorted_bam_file=str(tmp_path / "first.bam"), mark_duplicates=True)
    session.submit(prefix + ".bam", sorted_bam_file=str(tmp_path / "second.bam"), mark_duplicates=False)
    session.sample(prefix + ".bam", str(tmp_path / "first.tsv"))
    session.sample(prefix + ".bam", str(tmp_path / "second.tsv"))
    for context in session._lane_contexts():
        count = ctypes.c_uint64(1)
        assert session.api.markdup_allocated_bytes(context, ctypes.byref(count)) == 0 and count.value == 0
    session.close()
    _capi, host = _host()
    assert host.ahost_sorted_bam_file_marked((prefix + ".bam").encode(), str(tmp_path / "host.bam").encode(), 0, 1, None) == 0, host.ahost_last_error()
    _same_files(str(tmp_path / "first.bam"), str(tmp_path / "host.bam"))
    _same_files(str(tmp_path / "second.bam"), without_the_option[2])
    assert open(str(tmp_path / "first.bam"), "rb").read() != open(str(tmp_path / "second.bam"), "rb").read()
    for name in ("first.tsv", "second.tsv"):
        assert open(str(tmp_path / name), "rb").read() == without_the_option[0]


@pytest.mark.gpu
def test_the_session_refuses_before_any_launch(built, dataset_files, tmp_path):
    from arriba_amd.pipeline import ArribaError, WorkflowSession
    prefix = dataset_files("toy3k")
    session = WorkflowSession(prefix + ".fa", prefix + ".gtf", params={"disable_filters": ["blacklist"]})
    with pytest.raises(ArribaError, match="--mark-duplicates needs --sorted-bam"):
        session.sample(prefix + ".bam", str(tmp_path / "fusions.tsv"), mark_duplicates=True)
    session.close()
    session = WorkflowSession(prefix + ".fa", prefix + ".gtf", params={"disable_filters": ["blacklist"], "external_duplicate_marking": 1})
    with pytest.raises(ArribaError, match="--mark-duplicates and -u exclude each other"):
        session.sample(prefix + ".bam", str(tmp_path / "fusions.tsv"), sorted_bam_file=str(tmp_path / "sorted.bam"), mark_duplicates=True)
    session.close()
    assert os.listdir(str(tmp_path)) == []
