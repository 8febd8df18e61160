"""--coverage: the per-base alignment depth of the records of -x as bedGraph text (the rule: DESIGN.md 4.13).

No reference program writes this file; the rule is the project's.  tests/golden/coverage/hand_made.sam and .bedgraph are a pair a reader can check by eye; tests/coverage_lib.py
restates the rule in plain Python and numpy, test_restatement_equals_the_committed_file holds it to that pair, and only therefore it is the independent side for inputs made at
test time.  The CPU tier runs arriba_amd/csrc/device/depth_core.hpp stepped on the host (ahost_depth_track, ahost_depth_line, ahost_depth_file); the GPU tier the kernels of
agpu_depth.hip, whose file must equal the host's byte for byte and whose statistics must equal the host's."""
import ctypes
import gzip
import os
import struct
import subprocess
import sys
import zlib

import pytest

import conftest
import coverage_lib as lib
import virus_expression_lib as bam

sys.path.insert(0, os.path.join(conftest.ROOT, "tools"))

GOLDEN = os.path.join(conftest.ROOT, "tests", "golden", "coverage")
WORKFLOW = os.path.join(conftest.ROOT, "arriba_amd", "lib", "arriba_gpu_workflow")
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
SEEDED = ["seed%d" % (1000 + k) for k in range(50)]
COUNTED = ("records", "segments", "runs", "covered_positions", "aligned_bases", "max_depth", "text_bytes")  # what the device and the host must agree on
RESTATED = ("records", "runs", "covered_positions", "aligned_bases", "max_depth", "text_bytes")            # ... and what the restatement counts as well


def _golden(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


def _split(stream):
    assert stream[:4] == b"BAM\x01"
    at = 8 + struct.unpack_from("<i", stream, 4)[0]
    n_ref = struct.unpack_from("<i", stream, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", stream, at)[0]
    return stream[:at], stream[at:]


def _write_bgzf(path, payload, level):
    with open(path, "wb") as out:
        for at in range(0, len(payload), 0xff00):
            piece = payload[at:at + 0xff00]
            deflater = zlib.compressobj(level, zlib.DEFLATED, -15)
            body = deflater.compress(piece) + deflater.flush()
            out.write(struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(body) + 25) + body + struct.pack("<II", zlib.crc32(piece), len(piece)))
        out.write(EOF_BLOCK)


@pytest.fixture(scope="module")
def toy3k(dataset_files):
    """(prefix, uncompressed BAM stream, SAM text) of the dataset"""
    from bam_to_sam import bam_to_sam
    prefix = dataset_files("toy3k")
    return prefix, gzip.open(prefix + ".bam", "rb").read(), bam_to_sam(open(prefix + ".bam", "rb").read())[0]


@pytest.fixture(scope="module")
def cases(toy3k):
    """name -> (BAM header, record bytes, (text, counts) of the restatement): the committed case, 50 seeded ones, the hot one, the empty one, toy3k; made once"""
    cache = {}

    def get(name):
        if name not in cache:
            if name == "toy3k":
                header, record_bytes = _split(toy3k[1])
                case = bam.parse_sam(toy3k[2])
            elif name == "hot":
                case = lib.hot_case()
                header = bam.bam_header(case[0])
                first = bam.bam_record(case[0], case[1][0])  # (the others differ from it in the digits of their names only)
                assert first[36:42] == b"h00000"
                record_bytes = b"".join(first[:36] + b"h%05d" % k + first[42:] for k in range(len(case[1]) - 1)) + bam.bam_record(case[0], case[1][-1])
            else:
                case = bam.parse_sam(_golden("hand_made.sam")) if name == "hand_made" else lib.empty_case() if name == "empty" else lib.random_case(int(name[4:]))
                header, record_bytes = bam.bam_header(case[0]), bam.bam_records(case)
            cache[name] = (header, record_bytes, lib.restate(case))
        return cache[name]
    return get


# ---- the host side ------------------------------------------------------------------------------------------------------------------------------------------------

def _host():
    from arriba_amd import _capi
    return _capi, _capi.host_library()


def _host_track(header, record_bytes):
    """-> (text, statistics) of ahost_depth_track"""
    from arriba_amd.pipeline import depth_stats_of
    _capi, host = _host()
    contigs, stats = _capi.DepthContigs(), _capi.DepthStats()
    assert host.ahost_depth_contigs_of(header, len(header), ctypes.byref(contigs)) == 0, host.ahost_last_error()
    text, size = ctypes.c_void_p(), ctypes.c_uint64()
    assert host.ahost_depth_track(record_bytes, len(record_bytes), ctypes.byref(contigs), ctypes.byref(text), ctypes.byref(size), ctypes.byref(stats)) == 0, host.ahost_last_error()
    return ctypes.string_at(text, size.value), depth_stats_of(stats)


@pytest.fixture(scope="module")
def host_side(cases):
    """name -> what the host stepping gives: computed once, compared against by every test"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _host_track(*cases(name)[:2])
        return cache[name]
    return get


# ---- CPU tier -----------------------------------------------------------------------------------------------------------------------------------------------------

def test_restatement_equals_the_committed_file():
    """the brute-force restatement of the rule against the pair that is checked by eye"""
    case = bam.parse_sam(_golden("hand_made.sam"))
    text, counts = lib.restate(case)
    assert text == _golden("hand_made.bedgraph")
    assert 3 <= len(case[0]) <= 6 and all(50 <= length <= 5000 for _, length in case[0])
    assert counts == {"records": 22, "runs": 21, "covered_positions": 291, "aligned_bases": 391, "max_depth": 2, "text_bytes": len(text)}
    assert len(_golden("hand_made.sam")) < 100000 and len(text) < 100000


def test_host_gives_the_committed_bytes(built, cases, host_side):
    text, stats = host_side("hand_made")
    assert text == _golden("hand_made.bedgraph")
    assert {key: stats[key] for key in RESTATED} == cases("hand_made")[2][1]
    # b8 has no reference and flag 73 (bit 0x4 clear); with flag 0 the device ingest would refuse the sample as damaged, the host steps it: it does not count either
    case = bam.parse_sam(_golden("hand_made.sam").replace(b"b8\t73\t", b"b8\t0\t"))
    assert [record[1] for record in case[1] if record[0] == "b8"] == [0] and _host_track(bam.bam_header(case[0]), bam.bam_records(case))[0] == text
    assert stats["segments"] == 23  # (22 records, one segment each -- 5M3D5M and 4M2I4M1P2M are one -- but 10M5N10M, which has two)


@pytest.mark.parametrize("name", ["seeded", "hot", "empty", "toy3k"])
def test_host_equals_the_restatement(name, built, cases, host_side):
    runs = 0
    for case in (SEEDED if name == "seeded" else [name]):
        text, stats = host_side(case)
        expected_text, expected = cases(case)[2]
        assert text == expected_text, case
        assert {key: stats[key] for key in RESTATED} == expected, case
        runs += stats["runs"]
    if name == "hot":
        assert text == b"hot1\t1000\t1001\t70000\nhot1\t1001\t1064\t70001\nhot1\t1064\t1065\t1\n" and stats["max_depth"] == 70001 > 1 << 16
    assert (runs == 0 and text == b"") if name == "empty" else runs >= 3


def test_line_formatter_around_every_digit_boundary(built):
    """ahost_depth_line, which steps depth_line of depth_core.hpp: positions and depths around every power of ten, 2^31 - 1 and 2^32 - 1 (no contig of that size is allocated)"""
    _capi, host = _host()
    values = sorted(set([0, 1, (1 << 31) - 1, 1 << 31, (1 << 32) - 2, (1 << 32) - 1] + [10 ** k + d for k in range(1, 10) for d in (-1, 0, 1)]))
    out, size = ctypes.create_string_buffer(64), ctypes.c_uint32()
    for k, value in enumerate(values):
        for start, end, depth in ((value, values[-1 - k], values[(k * 7) % len(values)]), (values[(k * 5) % len(values)], value, 1), (0, 1, value)):
            assert host.ahost_depth_line(b"chrUn_1", start, end, depth, out, 64, ctypes.byref(size)) == 0, host.ahost_last_error()
            assert out.raw[:size.value] == b"chrUn_1\t%d\t%d\t%d\n" % (start, end, depth)
    assert host.ahost_depth_line(b"a_name_that_is_long", 1, 2, 3, out, 8, ctypes.byref(size)) != 0 and size.value == 26


def test_the_file_interface(built, toy3k, cases, tmp_path):
    """ahost_depth_file reads BAM and SAM text itself and leaves no temporary file"""
    from arriba_amd import _capi
    host = _capi.host_library()
    prefix, stream, text = toy3k
    open(str(tmp_path / "sample.sam"), "wb").write(text)
    expected = cases("toy3k")[2]
    assert expected[1]["runs"] > 100
    for source in (prefix + ".bam", str(tmp_path / "sample.sam")):
        path, stats = str(tmp_path / "track.bedgraph"), _capi.DepthStats()
        assert host.ahost_depth_file(source.encode(), path.encode(), ctypes.byref(stats)) == 0, host.ahost_last_error()
        assert open(path, "rb").read() == expected[0] and stats.runs == expected[1]["runs"]
        os.remove(path)
    assert host.ahost_depth_file((prefix + ".bam").encode(), str(tmp_path / "missing" / "track.bedgraph").encode(), None) != 0
    assert sorted(os.listdir(str(tmp_path))) == ["sample.sam"]


def _harness(target):
    directory = os.path.join(conftest.ROOT, "tests", "emu")
    subprocess.run(["make", "-s", "-C", directory, target], check=True)
    return os.path.join(directory, target)


@pytest.mark.parametrize("container", ["bam", "sam_text"])
def test_host_ingest_through_the_command_line(container, built, emu_api, toy3k, cases, tmp_path):
    """--host-ingest --coverage: the C++ driver (over the host stepping harness, where there is no GPU) writes the track of the restatement"""
    prefix, stream, text = toy3k
    sample = prefix + ".bam"
    if container == "sam_text":
        sample = str(tmp_path / "sample.sam")
        open(sample, "wb").write(text)
    command = [_harness("workflow_on_harness"), "-x", sample, "-g", prefix + ".gtf", "-a", prefix + ".fa", "-o", str(tmp_path / "fusions.tsv"), "-f", "blacklist", "--host-ingest", "--coverage", str(tmp_path / "track.bedgraph")]
    result = subprocess.run(command, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert result.returncode == 0, result.stderr[-2000:]
    assert open(str(tmp_path / "track.bedgraph"), "rb").read() == cases("toy3k")[2][0]
    assert not os.path.exists(str(tmp_path / "track.bedgraph.tmp"))
    assert open(str(tmp_path / "fusions.tsv")).read() == gzip.open(os.path.join(conftest.golden_dir("toy3k"), "fusions.tsv.gz"), "rt").read()


def test_a_path_in_a_missing_directory_is_refused_at_the_command_line(built, toy3k, tmp_path):
    prefix = toy3k[0]
    command = [WORKFLOW, "-x", prefix + ".bam", "-g", prefix + ".gtf", "-a", prefix + ".fa", "-o", str(tmp_path / "fusions.tsv"), "-f", "blacklist", "--coverage", str(tmp_path / "missing" / "track.bedgraph")]
    result = subprocess.run(command, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=60)
    assert result.returncode == 1 and "parent directory of output file" in result.stderr and "track.bedgraph" in result.stderr
    assert os.listdir(str(tmp_path)) == []
    assert "--coverage FILE" in subprocess.run([WORKFLOW, "-h"], stdout=subprocess.PIPE, universal_newlines=True, timeout=60).stdout


def test_cpp_driver_on_the_harness_says_that_it_has_no_device_library(built, emu_api, toy3k, tmp_path):
    """the test-only build of the C++ driver against the host stepping harness has no twin of the kernels of agpu_depth.hip: it links all the same and says so before the feed"""
    prefix = toy3k[0]
    command = [_harness("workflow_on_harness"), "-x", prefix + ".bam", "-g", prefix + ".gtf", "-a", prefix + ".fa", "-o", str(tmp_path / "fusions.tsv"), "-f", "blacklist", "--coverage", str(tmp_path / "track.bedgraph")]
    result = subprocess.run(command, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert result.returncode != 0 and "--coverage needs the device library (agpu_depth_begin)" in result.stderr
    assert not os.path.exists(str(tmp_path / "track.bedgraph")) and not os.path.exists(str(tmp_path / "track.bedgraph.tmp"))


def test_a_sample_over_ranks_is_refused_before_the_feed(built, emu_api, toy3k, tmp_path):
    """one sample over several ranks: the wording of the three sibling options, before a byte of the file is fed (the driver over the harness, a communicator of one rank that does nothing)"""
    from arriba_amd import _capi
    prefix = toy3k[0]
    driver = ctypes.CDLL(_harness("libworkflow_on_harness.so"))
    driver.arriba_workflow_open.restype = ctypes.c_void_p
    driver.arriba_workflow_last_error.restype = ctypes.c_char_p
    options = _capi.WorkflowOptions()
    driver.arriba_workflow_default_options(ctypes.byref(options))
    options.assembly_file, options.gene_annotation_file = (prefix + ".fa").encode(), (prefix + ".gtf").encode()
    session = ctypes.c_void_p(driver.arriba_workflow_open(ctypes.byref(options)))
    assert session, driver.arriba_workflow_last_error()
    nothing = lambda *arguments: 0  # noqa: E731
    communicator = _capi.WorkflowCommunicator(0, 1, None, _capi.ALL_GATHER(nothing), _capi.ALL_REDUCE_INT64(nothing), _capi.ALL_REDUCE_MAX_BYTES(nothing), None)
    assert driver.arriba_workflow_set_communicator(session, ctypes.byref(communicator)) == 0
    assert driver.arriba_workflow_coverage(session, str(tmp_path / "track.bedgraph").encode()) == 0
    status = driver.arriba_workflow_sample(session, (prefix + ".bam").encode(), str(tmp_path / "fusions.tsv").encode(), None, None, None)
    message = driver.arriba_workflow_last_error().decode()
    driver.arriba_workflow_close(session)
    assert status != 0 and "a coverage track of one sample over several GPUs is not supported" in message
    assert os.listdir(str(tmp_path)) == []


# ---- GPU tier -----------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pipeline(toy3k):
    """one device pipeline on the reference data of toy3k for every case that is ingested here (the contigs of a case join those of the session)"""
    from arriba_amd.pipeline import DevicePipeline, HostSession
    prefix = toy3k[0]
    made = DevicePipeline(HostSession(prefix + ".fa", prefix + ".gtf", interesting_contigs="1 2 3 4"), bam=prefix + ".bam")  # (only an interesting contig needs a sequence in the assembly)
    yield made
    made.close()


KNOBS = [{}, {"ARRIBA_INGEST_WINDOWS": "1048576,65536"}, {"ARRIBA_DEPTH_WINDOW": "997"}, {"ARRIBA_DEPTH_TEXT_WINDOW": "4096"}]


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["committed_and_hot", "seeded"])
@pytest.mark.parametrize("knobs", KNOBS, ids=["no_knobs", "ingest_windows", "position_windows", "text_windows"])
def test_device_file_is_the_host_file(knobs, group, built, pipeline, cases, host_side, tmp_path, monkeypatch):
    """the file of agpu_depth_* equals the host stepping byte for byte and the statistics are equal: the committed case, the empty one, toy3k and the hot case; 50 seeded inputs;
    with the ingest cut into windows; with windows of 997 positions, which runs cross at odd places; with staging windows of 4096 bytes, which lines straddle"""
    for knob in ("ARRIBA_INGEST_WINDOWS", "ARRIBA_DEPTH_WINDOW", "ARRIBA_DEPTH_TEXT_WINDOW"):
        if knob in knobs:
            monkeypatch.setenv(knob, knobs[knob])
        else:
            monkeypatch.delenv(knob, raising=False)
    for name in (["hand_made", "empty", "toy3k", "hot"] if group == "committed_and_hot" else SEEDED):
        header, record_bytes, restated = cases(name)
        sample = str(tmp_path / (name + ".bam"))
        _write_bgzf(sample, header + record_bytes, 0)
        pipeline._ingest_records(sample, False, 100, 64 << 20)  # (without the host's "no normal reads found": the stream is what matters here)
        os.remove(sample)
        path = str(tmp_path / (name + ".bedgraph"))
        stats = pipeline.write_coverage(path)
        text, expected = host_side(name)
        print(name, {key: stats[key] for key in COUNTED + ("position_windows", "text_windows", "peak_bytes")})
        assert open(path, "rb").read() == text and not os.path.exists(path + ".tmp"), name
        assert {key: stats[key] for key in COUNTED} == {key: expected[key] for key in COUNTED}, name
        assert pipeline.depth_allocated_bytes() == 0 and stats["peak_bytes"] > 0, name
        slots = sum(struct.unpack_from("<I", header, at)[0] + 1 for at in _length_fields(header))
        if "ARRIBA_DEPTH_WINDOW" in knobs:
            assert stats["position_windows"] == (slots + 996) // 997 > 1, name
        else:
            assert stats["position_windows"] == 1, name
        if "ARRIBA_DEPTH_TEXT_WINDOW" in knobs:
            assert stats["text_windows"] == (len(text) + 4095) // 4096, name
            assert stats["text_windows"] > 1 or name in ("hand_made", "empty", "hot"), name  # (those three have fewer than 4096 bytes of text)
        else:
            assert stats["text_windows"] == (1 if text else 0), name
        if name == "hand_made":
            assert text == _golden("hand_made.bedgraph")


def _length_fields(header):
    """where the l_ref words of a BAM header lie"""
    at = 8 + struct.unpack_from("<i", header, 4)[0]
    n_ref = struct.unpack_from("<i", header, at)[0]
    at += 4
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", header, at)[0]
        yield at + 4 + l_name
        at += 8 + l_name


@pytest.fixture(scope="module")
def without_the_option(toy3k, tmp_path_factory):
    """fusions.tsv and discarded.tsv of toy3k from a run of the command line without --coverage"""
    directory = tmp_path_factory.mktemp("plain")
    outputs = [str(directory / "fusions.tsv"), str(directory / "discarded.tsv")]
    result = _command_line(toy3k[0] + ".bam", toy3k[0], outputs, [])
    assert result.returncode == 0, result.stderr[-2000:]
    return [open(path, "rb").read() for path in outputs]


def _command_line(sample, prefix, outputs, extra):
    command = [WORKFLOW, "-x", sample, "-g", prefix + ".gtf", "-a", prefix + ".fa", "-o", outputs[0], "-O", outputs[1], "-f", "blacklist"]
    return subprocess.run(["timeout", "-k", "10", "120"] + command + extra, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)


@pytest.mark.gpu
@pytest.mark.parametrize("container", ["stored_bgzf", "deflated_bgzf", "sam_text"])
def test_command_line_writes_the_track_next_to_the_fusions(container, built, toy3k, cases, host_side, without_the_option, tmp_path):
    prefix, stream, text = toy3k
    os.mkdir(str(tmp_path / "in")); os.mkdir(str(tmp_path / "out"))
    sample = str(tmp_path / "in" / "sample.bam")
    if container == "sam_text":
        open(sample, "wb").write(text)
    else:
        _write_bgzf(sample, stream, 0 if container == "stored_bgzf" else 6)
    outputs = [str(tmp_path / "out" / "fusions.tsv"), str(tmp_path / "out" / "discarded.tsv")]
    result = _command_line(sample, prefix, outputs, ["--coverage", str(tmp_path / "out" / "track.bedgraph")])
    assert result.returncode == 0, result.stderr[-2000:]
    track = open(str(tmp_path / "out" / "track.bedgraph"), "rb").read()
    assert track == host_side("toy3k")[0] == cases("toy3k")[2][0]
    assert [open(path, "rb").read() for path in outputs] == without_the_option
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["discarded.tsv", "fusions.tsv", "track.bedgraph"]


@pytest.mark.gpu
def test_session_writes_the_track_of_the_sample_that_asked_for_it(built, toy3k, host_side, without_the_option, tmp_path):
    """two samples in one session, the option on the first only: the second leaves no file, and no buffer of the option is left on either lane"""
    from arriba_amd.pipeline import WorkflowSession
    prefix = toy3k[0]
    session = WorkflowSession(prefix + ".fa", prefix + ".gtf", params={"disable_filters": ["blacklist"]})
    os.mkdir(str(tmp_path / "first")); os.mkdir(str(tmp_path / "second"))
    session.submit(prefix + ".bam", coverage_file=str(tmp_path / "first" / "track.bedgraph"))
    session.submit(prefix + ".bam")
    session.sample(prefix + ".bam", str(tmp_path / "first" / "fusions.tsv"))
    assert session.timing["coverage"] > 0
    session.sample(prefix + ".bam", str(tmp_path / "second" / "fusions.tsv"))
    assert session.timing["coverage"] == 0
    for context in session._lane_contexts():
        count = ctypes.c_uint64(1)
        assert session.api.depth_allocated_bytes(context, ctypes.byref(count)) == 0 and count.value == 0
    session.close()
    assert sorted(os.listdir(str(tmp_path / "first"))) == ["fusions.tsv", "track.bedgraph"] and os.listdir(str(tmp_path / "second")) == ["fusions.tsv"]
    assert open(str(tmp_path / "first" / "track.bedgraph"), "rb").read() == host_side("toy3k")[0]
    for directory in ("first", "second"):
        assert open(str(tmp_path / directory / "fusions.tsv"), "rb").read() == without_the_option[0]


@pytest.mark.gpu
def test_refusals_and_the_off_switch(built, toy3k, host_side, tmp_path, monkeypatch):
    """with the option off no kernel whose name begins with depth_ is in the kernel profile and no buffer of it exists; before an ingest, for a part of a sample and behind the
    begin of the next ingest agpu_depth_begin is refused with a message"""
    from arriba_amd import _capi
    from arriba_amd.pipeline import ArribaError, DevicePipeline, HostSession
    prefix = toy3k[0]
    api, params, info = _capi.bind_device_api(_capi.device_library(), "agpu_"), _capi.Params(), _capi.DepthInfo()
    api.default_params(ctypes.byref(params))
    fresh = api.create(0, ctypes.byref(params))
    assert fresh, api.last_error()
    refused = api.depth_begin(fresh, None, None, None, 0, ctypes.byref(info))  # before an ingest
    message = api.last_error()
    api.destroy(fresh)
    assert refused != 0 and b"agpu_depth_begin: the record stream of the last ingest is not on the device any more" in message
    made = DevicePipeline(HostSession(prefix + ".fa", prefix + ".gtf"), bam=prefix + ".bam")
    made.set_profiling(True)
    made.read_chimeric_alignments(prefix + ".bam")
    made.run_workflow(str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv"))
    assert made.kernel_profile() and not [launch for launch in made.kernel_profile() if launch[0].startswith("depth")] and made.depth_allocated_bytes() == 0
    # ... and on, through the stages of the pipeline
    made.read_chimeric_alignments(prefix + ".bam")
    made.run_workflow(str(tmp_path / "again.tsv"), None, coverage_file=str(tmp_path / "track.bedgraph"))
    names = set(launch[0] for launch in made.kernel_profile())
    assert {"depth_mark_kernel", "depth_flag_kernel", "depth_emit_kernel", "depth_line_kernel", "depth_text_kernel"} <= names
    assert made.depth_allocated_bytes() == 0
    assert open(str(tmp_path / "track.bedgraph"), "rb").read() == host_side("toy3k")[0] and open(str(tmp_path / "again.tsv")).read() == open(str(tmp_path / "fusions.tsv")).read()
    # a part of a sample
    made._ingest_records(prefix + ".bam", False, 100, 64 << 20, part=0, parts=2)
    with pytest.raises(ArribaError, match="a coverage track of one sample over several GPUs is not supported"):
        made.write_coverage(str(tmp_path / "part.bedgraph"))
    # the stream was given back behind the ingest
    monkeypatch.setenv("ARRIBA_RELEASE_INGEST_BUFFERS", "1")
    made.read_chimeric_alignments(prefix + ".bam")
    monkeypatch.delenv("ARRIBA_RELEASE_INGEST_BUFFERS")
    with pytest.raises(ArribaError, match="agpu_depth_begin: the record stream of the last ingest is not on the device any more"):
        made.write_coverage(str(tmp_path / "gone.bedgraph"))
    assert made.depth_allocated_bytes() == 0
    # the next read_chimeric_alignments has begun
    made.read_chimeric_alignments(prefix + ".bam")
    host, handle, config = made.session._lib, made.session._session, _capi.IngestConfig()
    assert host.ahost_bam_open(handle, (prefix + ".bam").encode(), 0, 100, ctypes.byref(config)) == 0
    made._check(made.api.ingest_begin(made.ctx, ctypes.byref(config)))
    with pytest.raises(ArribaError, match="an ingest is under way|not on the device any more"):
        made.write_coverage(str(tmp_path / "second.bedgraph"))
    host.ahost_bam_close(handle)
    made.close()
    assert sorted(os.listdir(str(tmp_path))) == ["again.tsv", "discarded.tsv", "fusions.tsv", "track.bedgraph"]
