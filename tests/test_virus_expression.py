"""--virus-expression: the table of the reference's scripts/quantify_virus_expression.sh (default parameters) from the record stream of -x.

The expected side of every committed case is the file the script itself wrote (tests/golden/virus_expression/*.tsv, made by tools/make_virus_golden.py; nothing of the script is
in the repository).  tests/virus_expression_lib.py restates the rule of DESIGN.md 4.11 in plain Python; test_restatement_equals_every_committed_table holds it to those files, and
only therefore it is the independent side for inputs made at test time.  The CPU tier runs arriba_amd/csrc/device/virus_core.hpp stepped on the host (ahost_virus_expression) and
the host's arithmetic and formatting (ahost_virus_expression_table); the GPU tier the kernels of agpu_virus.hip, whose counters must equal the host's exactly."""
import ctypes
import gzip
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

import conftest
import virus_expression_lib as lib

sys.path.insert(0, os.path.join(conftest.ROOT, "tools"))

GOLDEN = os.path.join(conftest.ROOT, "tests", "golden", "virus_expression")
FIXTURES = ["hand_made"] + ["random%d" % k for k in range(1, 9)]
WORKFLOW = os.path.join(conftest.ROOT, "arriba_amd", "lib", "arriba_gpu_workflow")
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def _golden(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


def _fixture_case(name):
    return lib.parse_sam(_golden(name + ".sam"))


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
def streams(toy3k):
    """name -> (BAM header, record bytes): the committed cases, 50 seeded ones, toy3k"""
    cache = {}

    def get(name):
        if name not in cache:
            if name == "toy3k":
                cache[name] = _split(toy3k[1])
            else:
                case = _fixture_case(name) if name in FIXTURES else lib.random_case(int(name[4:]), 150)
                cache[name] = (lib.bam_header(case[0]), lib.bam_records(case))
        return cache[name]
    return get


SEEDED = ["seed%d" % (1000 + k) for k in range(50)]


# ---- the host side ------------------------------------------------------------------------------------------------------------------------------------------------

def _host():
    from arriba_amd import _capi
    return _capi, _capi.host_library()


def _host_counters(header, record_bytes, viral=None):
    """-> (counters dict, contigs dict, table bytes) of ahost_virus_expression + _table"""
    from arriba_amd.pipeline import virus_contigs_of, virus_counters_of
    _capi, host = _host()
    contigs, counters = _capi.VirusContigs(), _capi.VirusCounters()
    assert host.ahost_virus_contigs_of(header, len(header), viral, ctypes.byref(contigs)) == 0, host.ahost_last_error()
    assert host.ahost_virus_expression(record_bytes, len(record_bytes), ctypes.byref(contigs), ctypes.byref(counters)) == 0, host.ahost_last_error()
    text, size = ctypes.c_void_p(), ctypes.c_uint64()
    assert host.ahost_virus_expression_table(ctypes.byref(counters), ctypes.byref(contigs), ctypes.byref(text), ctypes.byref(size)) == 0, host.ahost_last_error()
    return virus_counters_of(counters), virus_contigs_of(contigs), ctypes.string_at(text, size.value)


def _same_counters(mine, theirs):
    assert mine["total"] == theirs["total"]
    for key in ("reads", "covered", "kmer_count", "active", "shared"):
        assert np.array_equal(mine[key], theirs[key]), key


def _equals_restatement(counters, contigs, expected):
    """the counters of the C side against those of the restatement (dicts by index of the contig in the header)"""
    assert counters["total"] == expected["total"] and list(contigs["viral_ref"]) == expected["viral"]
    for slot, v in enumerate(expected["viral"]):
        assert (counters["reads"][slot], counters["covered"][slot], counters["kmer_count"][slot]) == (expected["reads"].get(v, 0), expected["covered"].get(v, 0), expected["kmer_count"].get(v, 0)), contigs["names"][slot]
    active = [expected["viral"][slot] for slot in counters["active"]]
    assert sorted(active) == sorted(expected["reads"])
    for a, i in enumerate(active):
        for b, j in enumerate(active):
            assert counters["shared"][a, b] == (expected["shared"][(i, j)] if i != j else 0)


# ---- CPU tier -----------------------------------------------------------------------------------------------------------------------------------------------------

def test_restatement_equals_every_committed_table(toy3k):
    """the restatement of the rule against the files the script wrote; and the generator of the cases has not drifted from the committed inputs"""
    cases = lib.fixture_cases()
    for name in FIXTURES:
        assert lib.sam_text(cases[name]) == _golden(name + ".sam"), name
        assert lib.restate(_fixture_case(name))[0] == _golden(name + ".tsv"), name
    case = lib.parse_sam(toy3k[2])
    assert lib.restate(case)[0] == _golden("toy3k.tsv") and lib.restate(case, r"^GL")[0] == _golden("toy3k_GL.tsv")
    rows = _golden("toy3k.tsv").decode().split("\n")[1:-1]
    assert rows == ["NC_001526.4\t7900\t3249\t0.411266\t57\t515.997"]  # (the second virus, AC_000007.1, falls to the 5 % rule)
    assert len(_golden("hand_made.tsv").split(b"\n")) == 15 and all(len(_golden(name + ".sam")) < 100000 for name in FIXTURES)


@pytest.mark.parametrize("name", FIXTURES + ["toy3k"])
def test_host_gives_the_committed_bytes(name, built, streams, toy3k):
    header, record_bytes = streams(name)
    counters, contigs, table = _host_counters(header, record_bytes)
    assert table == _golden(name + ".tsv")
    _equals_restatement(counters, contigs, lib.restate(lib.parse_sam(toy3k[2]) if name == "toy3k" else _fixture_case(name))[1])


def test_host_equals_the_restatement_on_seeded_inputs(built, streams):
    rows = 0
    for name in SEEDED:
        counters, contigs, table = _host_counters(*streams(name))
        expected_table, expected = lib.restate(lib.random_case(int(name[4:]), 150))
        assert table == expected_table, name
        _equals_restatement(counters, contigs, expected)
        rows += table.count(b"\n") - 1
    assert rows > 50


def test_other_patterns_and_the_file_interface(built, toy3k, tmp_path):
    """-v 'GL*' is VIRAL_CONTIGS='^GL' of the script; ahost_virus_expression_file reads BAM and SAM text itself and leaves no temporary file"""
    from arriba_amd.pipeline import HostSession
    prefix, stream, text = toy3k
    assert _host_counters(*_split(stream), viral=b"GL*")[2] == _golden("toy3k_GL.tsv")
    open(str(tmp_path / "sample.sam"), "wb").write(text)
    for viral, expected in ((None, "toy3k.tsv"), ("GL*", "toy3k_GL.tsv")):
        session = HostSession(prefix + ".fa", prefix + ".gtf", viral_contigs=viral)
        for source in (prefix + ".bam", str(tmp_path / "sample.sam")):
            path = str(tmp_path / "table.tsv")
            assert session._lib.ahost_virus_expression_file(session._session, source.encode(), path.encode()) == 0, session._lib.ahost_last_error()
            assert open(path, "rb").read() == _golden(expected)
            os.remove(path)
        assert session._lib.ahost_virus_expression_file(session._session, (prefix + ".bam").encode(), str(tmp_path / "missing" / "table.tsv").encode()) != 0
        session.close()
    assert sorted(os.listdir(str(tmp_path))) == ["sample.sam"]


def test_more_viral_contigs_than_a_key_can_name_are_refused(built):
    _capi, host = _host()
    header = lib.bam_header([("NC_%d" % k, 100) for k in range(65536)])
    contigs, counters = _capi.VirusContigs(), _capi.VirusCounters()
    assert host.ahost_virus_contigs_of(header, len(header), None, ctypes.byref(contigs)) == 0 and contigs.n_viruses == 65536
    assert host.ahost_virus_expression(b"", 0, ctypes.byref(contigs), ctypes.byref(counters)) != 0 and b"65536 viral contigs" in host.ahost_last_error()


def _harness(target):
    directory = os.path.join(conftest.ROOT, "tests", "emu")
    subprocess.run(["make", "-s", "-C", directory, target], check=True)
    return os.path.join(directory, target)


@pytest.mark.parametrize("container", ["bam", "sam_text"])
def test_host_ingest_through_the_command_line(container, built, emu_api, toy3k, tmp_path):
    """--host-ingest --virus-expression: the C++ driver (over the host stepping harness, where there is no GPU) writes the committed table"""
    prefix, stream, text = toy3k
    sample = prefix + ".bam"
    if container == "sam_text":
        sample = str(tmp_path / "sample.sam")
        open(sample, "wb").write(text)
    command = [_harness("workflow_on_harness"), "-x", sample, "-g", prefix + ".gtf", "-a", prefix + ".fa", "-o", str(tmp_path / "fusions.tsv"), "-f", "blacklist", "--host-ingest", "--virus-expression", str(tmp_path / "virus.tsv")]
    result = subprocess.run(command, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert result.returncode == 0, result.stderr[-2000:]
    assert open(str(tmp_path / "virus.tsv"), "rb").read() == _golden("toy3k.tsv")
    assert not os.path.exists(str(tmp_path / "virus.tsv.tmp"))
    assert open(str(tmp_path / "fusions.tsv")).read() == gzip.open(os.path.join(conftest.golden_dir("toy3k"), "fusions.tsv.gz"), "rt").read()


def test_a_path_in_a_missing_directory_is_refused_at_the_command_line(built, toy3k, tmp_path):
    prefix = toy3k[0]
    command = [WORKFLOW, "-x", prefix + ".bam", "-g", prefix + ".gtf", "-a", prefix + ".fa", "-o", str(tmp_path / "fusions.tsv"), "-f", "blacklist", "--virus-expression", str(tmp_path / "missing" / "virus.tsv")]
    result = subprocess.run(command, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=60)
    assert result.returncode == 1 and "parent directory of output file" in result.stderr and "virus.tsv" in result.stderr
    assert os.listdir(str(tmp_path)) == []
    assert "--virus-expression FILE" in subprocess.run([WORKFLOW, "-h"], stdout=subprocess.PIPE, universal_newlines=True, timeout=60).stdout


def test_cpp_driver_on_the_harness_says_that_it_has_no_device_library(built, emu_api, toy3k, tmp_path):
    """the test-only build of the C++ driver against the host stepping harness has no twin of the kernels of agpu_virus.hip: it links all the same and says so before the feed"""
    prefix = toy3k[0]
    command = [_harness("workflow_on_harness"), "-x", prefix + ".bam", "-g", prefix + ".gtf", "-a", prefix + ".fa", "-o", str(tmp_path / "fusions.tsv"), "-f", "blacklist", "--virus-expression", str(tmp_path / "virus.tsv")]
    result = subprocess.run(command, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert result.returncode != 0 and "--virus-expression needs the device library (agpu_virus_expression)" in result.stderr
    assert not os.path.exists(str(tmp_path / "virus.tsv")) and not os.path.exists(str(tmp_path / "virus.tsv.tmp"))


def test_a_sample_over_ranks_is_refused_before_the_feed(built, emu_api, toy3k, tmp_path):
    """one sample over several ranks: the wording of --sorted-bam, before a byte of the file is fed (the driver over the harness, a communicator of one rank that does nothing)"""
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
    assert driver.arriba_workflow_virus_expression(session, str(tmp_path / "virus.tsv").encode()) == 0
    status = driver.arriba_workflow_sample(session, (prefix + ".bam").encode(), str(tmp_path / "fusions.tsv").encode(), None, None, None)
    message = driver.arriba_workflow_last_error().decode()
    driver.arriba_workflow_close(session)
    assert status != 0 and "a virus expression table of one sample over several GPUs is not supported" in message
    assert os.listdir(str(tmp_path)) == []


# ---- GPU tier -----------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pipeline(toy3k):
    """one device pipeline on the reference data of toy3k for every case that is ingested here (the contigs of a case join those of the session; what -v names does not depend on -i)"""
    from arriba_amd.pipeline import DevicePipeline, HostSession
    prefix = toy3k[0]
    made = DevicePipeline(HostSession(prefix + ".fa", prefix + ".gtf", interesting_contigs="1 2 3 4"), bam=prefix + ".bam")  # (only an interesting contig needs a sequence in the assembly)
    yield made
    made.close()


@pytest.fixture(scope="module")
def host_side(streams):
    """name -> what the host stepping gives: computed once, compared against by every device test"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _host_counters(*streams(name))
        return cache[name]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["committed", "seeded"])
@pytest.mark.parametrize("knobs", [{}, {"ARRIBA_INGEST_WINDOWS": "1048576,65536"}, {"ARRIBA_VIRUS_KMER_WINDOW": "700"}], ids=["one_window", "ingest_windows", "kmer_rounds"])
def test_device_counters_are_the_host_counters(knobs, group, built, pipeline, streams, host_side, tmp_path, monkeypatch):
    """total, reads, covered, kmer_count and the shared matrix of agpu_virus_expression equal the host stepping exactly: every committed case and toy3k, 20 seeded inputs;
    with the ingest cut into windows; with a k-mer window so small that the set is sorted and merged in several rounds"""
    for knob in ("ARRIBA_INGEST_WINDOWS", "ARRIBA_VIRUS_KMER_WINDOW"):
        if knob in knobs:
            monkeypatch.setenv(knob, knobs[knob])
        else:
            monkeypatch.delenv(knob, raising=False)
    most_rounds = 0
    for name in (FIXTURES + ["toy3k"] if group == "committed" else SEEDED[:20]):
        header, record_bytes = streams(name)
        sample = str(tmp_path / (name + ".bam"))
        _write_bgzf(sample, header + record_bytes, 0)
        pipeline._ingest_records(sample, False, 100, 64 << 20)  # (without the host's "no normal reads found": the stream is what matters here)
        path = str(tmp_path / (name + ".tsv"))
        counters = pipeline.write_virus_expression(path)
        expected, contigs, table = host_side(name)
        _same_counters(counters, expected)
        assert open(path, "rb").read() == table and not os.path.exists(path + ".tmp"), name
        assert counters["kmer_keys"] == (expected["kmer_keys"]) and counters["candidates"] == expected["candidates"], name
        assert counters["kmer_rounds"] == (counters["kmer_keys"] + 699) // 700 if "ARRIBA_VIRUS_KMER_WINDOW" in knobs else counters["kmer_rounds"] <= 1, name
        assert pipeline.virus_allocated_bytes() == 0 and counters["peak_bytes"] > 0, name
        most_rounds = max(most_rounds, counters["kmer_rounds"])
        if name in FIXTURES or name == "toy3k":
            assert table == _golden(name + ".tsv"), name
    assert most_rounds >= (3 if "ARRIBA_VIRUS_KMER_WINDOW" in knobs else 1)


@pytest.fixture(scope="module")
def without_the_option(toy3k, tmp_path_factory):
    """fusions.tsv and discarded.tsv of toy3k from a run of the command line without --virus-expression"""
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
def test_command_line_writes_the_table_next_to_the_fusions(container, built, toy3k, without_the_option, tmp_path):
    prefix, stream, text = toy3k
    os.mkdir(str(tmp_path / "in")); os.mkdir(str(tmp_path / "out"))
    sample = str(tmp_path / "in" / "sample.bam")
    if container == "sam_text":
        open(sample, "wb").write(text)
    else:
        _write_bgzf(sample, stream, 0 if container == "stored_bgzf" else 6)
    outputs = [str(tmp_path / "out" / "fusions.tsv"), str(tmp_path / "out" / "discarded.tsv")]
    result = _command_line(sample, prefix, outputs, ["--virus-expression", str(tmp_path / "out" / "virus.tsv")])
    assert result.returncode == 0, result.stderr[-2000:]
    assert open(str(tmp_path / "out" / "virus.tsv"), "rb").read() == _golden("toy3k.tsv")
    assert [open(path, "rb").read() for path in outputs] == without_the_option
    assert open(outputs[0]).read() == gzip.open(os.path.join(conftest.golden_dir("toy3k"), "fusions.tsv.gz"), "rt").read()
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["discarded.tsv", "fusions.tsv", "virus.tsv"]


@pytest.mark.gpu
def test_other_patterns_on_the_device(built, toy3k, tmp_path):
    """-v 'GL*' through the command line: the table the script gives with VIRAL_CONTIGS='^GL'"""
    prefix = toy3k[0]
    outputs = [str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv")]
    result = _command_line(prefix + ".bam", prefix, outputs, ["-v", "GL*", "--virus-expression", str(tmp_path / "virus.tsv")])
    assert result.returncode == 0, result.stderr[-2000:]
    assert open(str(tmp_path / "virus.tsv"), "rb").read() == _golden("toy3k_GL.tsv")


@pytest.mark.gpu
def test_session_writes_the_table_of_the_sample_that_asked_for_it(built, toy3k, without_the_option, tmp_path):
    """two samples in one session, the option on the first only: the second leaves no file, and no buffer of the option is left on either lane"""
    from arriba_amd.pipeline import WorkflowSession
    prefix = toy3k[0]
    session = WorkflowSession(prefix + ".fa", prefix + ".gtf", params={"disable_filters": ["blacklist"]})
    os.mkdir(str(tmp_path / "first")); os.mkdir(str(tmp_path / "second"))
    session.submit(prefix + ".bam", virus_expression_file=str(tmp_path / "first" / "virus.tsv"))
    session.submit(prefix + ".bam")
    session.sample(prefix + ".bam", str(tmp_path / "first" / "fusions.tsv"))
    assert session.timing["virus_expression"] > 0
    session.sample(prefix + ".bam", str(tmp_path / "second" / "fusions.tsv"))
    assert session.timing["virus_expression"] == 0
    for context in session._lane_contexts():
        count = ctypes.c_uint64(1)
        assert session.api.virus_allocated_bytes(context, ctypes.byref(count)) == 0 and count.value == 0
    session.close()
    assert sorted(os.listdir(str(tmp_path / "first"))) == ["fusions.tsv", "virus.tsv"] and os.listdir(str(tmp_path / "second")) == ["fusions.tsv"]
    assert open(str(tmp_path / "first" / "virus.tsv"), "rb").read() == _golden("toy3k.tsv")
    for directory in ("first", "second"):
        assert open(str(tmp_path / directory / "fusions.tsv"), "rb").read() == without_the_option[0]


@pytest.mark.gpu
def test_refusals_and_the_off_switch(built, toy3k, tmp_path):
    """with the option off no kernel of agpu_virus.hip is in the kernel profile and no buffer of it exists; a part of a sample and a stream that is gone are refused with a message"""
    from arriba_amd import _capi
    from arriba_amd.pipeline import ArribaError, DevicePipeline, HostSession
    prefix = toy3k[0]
    made = DevicePipeline(HostSession(prefix + ".fa", prefix + ".gtf"), bam=prefix + ".bam")
    made.set_profiling(True)
    made.read_chimeric_alignments(prefix + ".bam")
    made.run_workflow(str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv"))
    assert made.kernel_profile() and not [launch for launch in made.kernel_profile() if launch[0].startswith("virus")] and made.virus_allocated_bytes() == 0
    # ... and on, through the stages of the pipeline
    made.read_chimeric_alignments(prefix + ".bam")
    made.run_workflow(str(tmp_path / "again.tsv"), None, virus_expression_file=str(tmp_path / "virus.tsv"))
    names = set(launch[0] for launch in made.kernel_profile())
    assert {"virus_scan_kernel", "virus_candidate_kernel", "virus_kmer_emit_kernel", "virus_shared_kernel", "virus_covered_kernel"} <= names
    assert made.virus_allocated_bytes() == 0
    assert open(str(tmp_path / "virus.tsv"), "rb").read() == _golden("toy3k.tsv") and open(str(tmp_path / "again.tsv")).read() == open(str(tmp_path / "fusions.tsv")).read()
    # a part of a sample
    made._ingest_records(prefix + ".bam", False, 100, 64 << 20, part=0, parts=2)
    with pytest.raises(ArribaError, match="a virus expression table of one sample over several GPUs is not supported"):
        made.write_virus_expression(str(tmp_path / "part.tsv"))
    # the next read_chimeric_alignments has begun
    made.read_chimeric_alignments(prefix + ".bam")
    host, handle, config = made.session._lib, made.session._session, _capi.IngestConfig()
    assert host.ahost_bam_open(handle, (prefix + ".bam").encode(), 0, 100, ctypes.byref(config)) == 0
    made._check(made.api.ingest_begin(made.ctx, ctypes.byref(config)))
    with pytest.raises(ArribaError, match="an ingest is under way|not on the device any more"):
        made.write_virus_expression(str(tmp_path / "second.tsv"))
    host.ahost_bam_close(handle)
    made.close()
    assert sorted(os.listdir(str(tmp_path))) == ["again.tsv", "discarded.tsv", "fusions.tsv", "virus.tsv"]
