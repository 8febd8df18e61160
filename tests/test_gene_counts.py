"""--gene-counts: reads per gene of the records of -x in three columns, the file STAR writes as ReadsPerGene.out.tab (the rule: DESIGN.md 4.15).

No program of the reference writes this file; the rule is the project's.  tests/golden/gene_counts/hand_made.{fa,gtf,sam,tab} are a case a reader can check by eye, one template
per line of the rule; tests/gene_counts_lib.py restates the rule in plain Python with sets of positions, test_restatement_equals_the_committed_file holds it to that case, and only
therefore it is the independent side for inputs made at test time.  The CPU tier runs arriba_amd/csrc/device/genecount_core.hpp stepped on the host (ahost_gene_counts_*); the GPU
tier the kernels of agpu_genecount.hip, whose file must equal the host's byte for byte and whose statistics must equal the host's."""
import ctypes
import gzip
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import conftest
import gene_counts_lib as lib

sys.path.insert(0, os.path.join(conftest.ROOT, "tools"))

GOLDEN = lib.GOLDEN
WORKFLOW = os.path.join(conftest.ROOT, "arriba_amd", "lib", "arriba_gpu_workflow")
SEEDED = ["seed%d" % (1500 + k) for k in range(50)]
COUNTED = ("records", "templates", "without_primary", "ends", "blocks")  # what the device, the host and the restatement must agree on


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


def _invariant(text, stats):
    """every column sums to templates - without_primary; the file has a line per gene and four more"""
    rows = [line.split(b"\t") for line in text.split(b"\n")[:-1]]
    assert [row[0] for row in rows[:4]] == [name.encode() for name in lib.SPECIAL] and all(len(row) == 4 for row in rows)
    for c in (1, 2, 3):
        assert sum(int(row[c]) for row in rows) == stats["templates"] - stats["without_primary"]
    return rows


@pytest.fixture(scope="module")
def annotation():
    return lib.load_annotation()


@pytest.fixture(scope="module")
def cases(annotation):
    """name -> (BAM header, record bytes, (text, counts, stats) of the restatement) on the committed annotation: made once"""
    cache = {}

    def get(name):
        if name not in cache:
            if name == "hand_made":
                case = lib.parse_sam(_golden("hand_made.sam"))
            elif name.startswith("seed"):
                case = lib.random_case(int(name[4:]), annotation)
            else:
                case = {"hot": lib.hot_case, "wavefront": lib.wavefront_case, "empty": lib.empty_case, "aux": lib.aux_case, "no_records": lib.no_records_case}[name](annotation)
            cache[name] = (lib.bam_header(case[0]), lib.bam_records(case), lib.restate(annotation, case))
        return cache[name]
    return get


# ---- the host side ------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def committed_session(built):
    from arriba_amd.pipeline import HostSession
    session = HostSession(os.path.join(GOLDEN, "hand_made.fa"), os.path.join(GOLDEN, "hand_made.gtf"), interesting_contigs=lib.COMMITTED_CONTIGS)
    yield session
    session.close()


def _gene_ids(session):
    n_genes, ids, size = ctypes.c_uint32(), ctypes.c_void_p(), ctypes.c_uint64()
    assert session._lib.ahost_gene_counts_genes(session._session, ctypes.byref(n_genes), ctypes.byref(ids), ctypes.byref(size)) == 0
    names = ctypes.string_at(ids, size.value).decode().split("\n")[:-1]
    assert len(names) == n_genes.value
    return names


def _host_counts(session, header, record_bytes):
    """-> (text, statistics) of ahost_gene_counts_of + ahost_gene_counts_text"""
    from arriba_amd import _capi
    from arriba_amd.pipeline import gene_count_stats_of
    host, handle = session._lib, session._session
    counts, stats = np.zeros((3, len(_gene_ids(session)) + 4), dtype=np.uint64), _capi.GeneCountStats()
    assert host.ahost_gene_counts_of(handle, header, len(header), record_bytes, len(record_bytes), counts.ctypes.data, counts.size, ctypes.byref(stats)) == 0, host.ahost_last_error()
    text, size = ctypes.c_void_p(), ctypes.c_uint64()
    assert host.ahost_gene_counts_text(handle, counts.ctypes.data, counts.size, ctypes.byref(text), ctypes.byref(size)) == 0, host.ahost_last_error()
    return ctypes.string_at(text, size.value), gene_count_stats_of(stats)


@pytest.fixture(scope="module")
def host_side(cases, committed_session):
    """name -> what the host stepping gives: computed once, compared against by every test"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _host_counts(committed_session, *cases(name)[:2])
        return cache[name]
    return get


@pytest.fixture(scope="module")
def toy3k(dataset_files):
    """(prefix, uncompressed BAM stream, SAM text) of the dataset"""
    from bam_to_sam import bam_to_sam
    prefix = dataset_files("toy3k")
    return prefix, gzip.open(prefix + ".bam", "rb").read(), bam_to_sam(open(prefix + ".bam", "rb").read())[0]


@pytest.fixture(scope="module")
def toy3k_host(toy3k):
    """(text, statistics) of the host stepping on toy3k, against toy3k's own annotation"""
    from arriba_amd.pipeline import HostSession
    prefix = toy3k[0]
    session = HostSession(prefix + ".fa", prefix + ".gtf", interesting_contigs="1 2 3 4")
    result = _host_counts(session, *_split(toy3k[1]))
    session.close()
    return result


# ---- CPU tier -----------------------------------------------------------------------------------------------------------------------------------------------------

def test_restatement_equals_the_committed_file(annotation):
    """the brute-force restatement of the rule against the case that is checked by eye"""
    case = lib.parse_sam(_golden("hand_made.sam"))
    text, counts, stats = lib.restate(annotation, case)
    assert text == _golden("hand_made.tab")
    assert stats == {"records": 43, "templates": 33, "without_primary": 1, "ends": 36, "blocks": 31}
    assert [name for name, _ in case[0]] == ["g1", "g2", "g3", "orphan"] and set(annotation["lengths"]) == {"g1", "g2", "g3"}
    assert all(len(_golden("hand_made." + kind)) < 100000 for kind in ("fa", "gtf", "sam", "tab"))
    assert counts["GZ"] == [0, 0, 0] and len(annotation["genes"]) == len(set(annotation["genes"])) == 15
    _invariant(text, stats)


def test_host_gives_the_committed_bytes(built, cases, host_side, committed_session, annotation, tmp_path):
    text, stats = host_side("hand_made")
    assert text == _golden("hand_made.tab")
    assert {key: stats[key] for key in COUNTED} == cases("hand_made")[2][2]
    assert _gene_ids(committed_session) == annotation["genes"]
    # ... and through the project's own reader of SAM text, which chooses the types of the NH fields
    path, counted = str(tmp_path / "counts.tab"), _stats()
    host = committed_session._lib
    assert host.ahost_gene_counts_file(committed_session._session, os.path.join(GOLDEN, "hand_made.sam").encode(), path.encode(), ctypes.byref(counted)) == 0, host.ahost_last_error()
    assert open(path, "rb").read() == text and counted.blocks == 31 and os.listdir(str(tmp_path)) == ["counts.tab"]


def _stats():
    from arriba_amd import _capi
    return _capi.GeneCountStats()


def test_the_corners_of_the_nh_walk(built, cases, host_side):
    """NH:Z in front of NH:i counts as 1 (the first field named NH decides); a B array longer than its record, a field of an unknown type and a Z field without its end in front of
    NH:i:5 end the walk (1); NH:i:5 alone and behind a well-formed B array is multimapping.  The numbers are written out here, not taken from the restatement"""
    text, stats = host_side("aux")
    assert text == cases("aux")[2][0]
    rows = dict((row[0], row[1:]) for row in _invariant(text, stats))
    assert rows[b"N_multimapping"] == [b"2", b"2", b"2"] and rows[b"GK"] == [b"4", b"4", b"0"] and rows[b"N_noFeature"] == [b"0", b"0", b"4"]
    assert stats["templates"] == 6 and stats["ends"] == 6 and stats["blocks"] == 4


@pytest.mark.parametrize("name", ["seeded", "hot", "empty", "wavefront", "no_records"])
def test_host_equals_the_restatement(name, built, cases, host_side, committed_session, annotation):
    totals = None
    for case in (SEEDED if name == "seeded" else [name]):
        text, stats = host_side(case)
        expected_text, expected_counts, expected = cases(case)[2]
        assert (len(cases(case)[1]) > 0) == (name != "no_records") and expected["records"] <= (400 if name == "seeded" else 1 << 20)
        assert text == expected_text, case
        assert {key: stats[key] for key in COUNTED} == expected, case
        rows = _invariant(text, stats)
        assert len(rows) == len(annotation["genes"]) + 4
        table = np.array([[int(x) for x in row[1:]] for row in rows])
        totals = table if totals is None else totals + table
    if name == "seeded":  # the seeded set as a whole exercises the rule
        assert (totals[:4] > 0).all(), totals[:4]
        assert ((totals[4:] > 0).sum(axis=0) >= 10).all(), totals[4:]
        assert not (totals[:, 0] == totals[:, 1]).all() and not (totals[:, 0] == totals[:, 2]).all() and not (totals[:, 1] == totals[:, 2]).all()
    if name == "hot":
        assert b"\nGK\t70001\t70001\t0\n" in text and 70001 > 1 << 16 and stats["templates"] == 70065
        assert b"\nGA\t22\t" in text and b"\nGB\t21\t" in text and b"\nGJ\t21\t" in text
    if name == "wavefront":
        assert stats["templates"] == 65
    if name == "empty":
        assert totals.sum() == 0 and stats["without_primary"] == stats["templates"] == 2
        # ... and no record at all
        header = cases("empty")[0]
        text, stats = _host_counts(committed_session, header, b"")
        assert text == expected_text and stats["records"] == 0 and len(text.split(b"\n")) == len(annotation["genes"]) + 5
    if name == "no_records":
        assert totals.sum() == 0 and stats["records"] == stats["templates"] == 0 and len(rows) == len(annotation["genes"]) + 4


def test_the_file_interface(built, toy3k, toy3k_host, tmp_path):
    """ahost_gene_counts_file reads BAM and SAM text itself and leaves no temporary file"""
    from arriba_amd.pipeline import HostSession
    prefix, stream, text = toy3k
    session = HostSession(prefix + ".fa", prefix + ".gtf", interesting_contigs="1 2 3 4")
    host, handle = session._lib, session._session
    open(str(tmp_path / "sample.sam"), "wb").write(text)
    expected, expected_stats = toy3k_host
    rows = _invariant(expected, expected_stats)
    assert sum(1 for row in rows[4:] if int(row[1]) > 0) >= 3 and expected_stats["blocks"] > 1000
    for source in (prefix + ".bam", str(tmp_path / "sample.sam")):
        path, stats = str(tmp_path / "counts.tab"), _stats()
        assert host.ahost_gene_counts_file(handle, source.encode(), path.encode(), ctypes.byref(stats)) == 0, host.ahost_last_error()
        assert open(path, "rb").read() == expected and stats.blocks == expected_stats["blocks"]
        os.remove(path)
    assert host.ahost_gene_counts_file(handle, (prefix + ".bam").encode(), str(tmp_path / "missing" / "counts.tab").encode(), None) != 0
    session.close()
    assert sorted(os.listdir(str(tmp_path))) == ["sample.sam"]


def _harness(target):
    directory = os.path.join(conftest.ROOT, "tests", "emu")
    subprocess.run(["make", "-s", "-C", directory, target], check=True)
    return os.path.join(directory, target)


def test_host_ingest_through_the_command_line(built, emu_api, toy3k, toy3k_host, tmp_path):
    """--host-ingest --gene-counts: the C++ driver (over the host stepping harness, where there is no GPU) writes the table of the host stepping, and fusions.tsv is the golden one"""
    prefix = toy3k[0]
    command = [_harness("workflow_on_harness"), "-x", prefix + ".bam", "-g", prefix + ".gtf", "-a", prefix + ".fa", "-o", str(tmp_path / "fusions.tsv"), "-f", "blacklist", "--host-ingest", "--gene-counts", str(tmp_path / "counts.tab")]
    result = subprocess.run(command, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert result.returncode == 0, result.stderr[-2000:]
    assert open(str(tmp_path / "counts.tab"), "rb").read() == toy3k_host[0]
    assert not os.path.exists(str(tmp_path / "counts.tab.tmp"))
    assert "Counting reads per gene (records=" in result.stdout
    assert open(str(tmp_path / "fusions.tsv")).read() == gzip.open(os.path.join(conftest.golden_dir("toy3k"), "fusions.tsv.gz"), "rt").read()


def test_a_path_in_a_missing_directory_is_refused_at_the_command_line(built, toy3k, tmp_path):
    prefix = toy3k[0]
    command = [WORKFLOW, "-x", prefix + ".bam", "-g", prefix + ".gtf", "-a", prefix + ".fa", "-o", str(tmp_path / "fusions.tsv"), "-f", "blacklist", "--gene-counts", str(tmp_path / "missing" / "counts.tab")]
    result = subprocess.run(command, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=60)
    assert result.returncode == 1 and "parent directory of output file" in result.stderr and "counts.tab" in result.stderr
    assert os.listdir(str(tmp_path)) == []
    assert "--gene-counts FILE" in subprocess.run([WORKFLOW, "-h"], stdout=subprocess.PIPE, universal_newlines=True, timeout=60).stdout


def test_cpp_driver_on_the_harness_says_that_it_has_no_device_library(built, emu_api, toy3k, tmp_path):
    """the test-only build of the C++ driver against the host stepping harness has no twin of the kernels of agpu_genecount.hip: it links all the same and says so before the feed"""
    prefix = toy3k[0]
    command = [_harness("workflow_on_harness"), "-x", prefix + ".bam", "-g", prefix + ".gtf", "-a", prefix + ".fa", "-o", str(tmp_path / "fusions.tsv"), "-f", "blacklist", "--gene-counts", str(tmp_path / "counts.tab")]
    result = subprocess.run(command, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert result.returncode != 0 and "--gene-counts needs the device library (agpu_gene_counts)" in result.stderr
    assert not os.path.exists(str(tmp_path / "counts.tab")) and not os.path.exists(str(tmp_path / "counts.tab.tmp"))


def test_a_sample_over_ranks_is_refused_before_the_feed(built, emu_api, toy3k, tmp_path):
    """one sample over several ranks: refused before a byte of the file is fed (the driver over the harness, a communicator of one rank that does nothing)"""
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
    driver.arriba_workflow_gene_counts.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    assert driver.arriba_workflow_gene_counts(session, str(tmp_path / "counts.tab").encode()) == 0
    status = driver.arriba_workflow_sample(session, (prefix + ".bam").encode(), str(tmp_path / "fusions.tsv").encode(), None, None, None)
    message = driver.arriba_workflow_last_error().decode()
    driver.arriba_workflow_close(session)
    assert status != 0 and "ERROR: gene counts of one sample over several GPUs are not supported" in message
    assert os.listdir(str(tmp_path)) == []


# ---- GPU tier -----------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pipeline(committed_session, cases, tmp_path_factory):
    """one device pipeline on the committed annotation for every case that is ingested here"""
    sample = str(tmp_path_factory.mktemp("committed") / "hand_made.bam")
    lib.write_bgzf(sample, cases("hand_made")[0] + cases("hand_made")[1], 0)
    made = lib.stream_pipeline(committed_session, sample)
    yield made
    made.close()


@pytest.fixture(scope="module")
def toy3k_pipeline(toy3k):
    from arriba_amd.pipeline import DevicePipeline, HostSession
    prefix = toy3k[0]
    made = DevicePipeline(HostSession(prefix + ".fa", prefix + ".gtf", interesting_contigs="1 2 3 4"), bam=prefix + ".bam")
    yield made
    made.close()


KNOBS = [{}, {"ARRIBA_INGEST_WINDOWS": "1048576,65536"}, {"ARRIBA_GENECOUNT_HASH_BITS": "4"}]


def _set(knobs, monkeypatch):
    for knob in ("ARRIBA_INGEST_WINDOWS", "ARRIBA_GENECOUNT_HASH_BITS"):
        if knob in knobs:
            monkeypatch.setenv(knob, knobs[knob])
        else:
            monkeypatch.delenv(knob, raising=False)


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["committed_and_hot", "seeded"])
@pytest.mark.parametrize("knobs", KNOBS, ids=["no_knobs", "ingest_windows", "hash_collisions"])
def test_device_file_is_the_host_file(knobs, group, built, pipeline, cases, host_side, tmp_path, monkeypatch):
    """the file of agpu_gene_counts equals the host stepping byte for byte and the statistics are equal: the committed case, the empty one, the hot one, 65 templates, the corners of the NH
    walk and a file that holds a header and no record; 50 seeded inputs; with the ingest cut into windows; with four bits of the hash of a read name, so that every name is found at
    the end of a probe run"""
    _set(knobs, monkeypatch)
    for name in (["hand_made", "empty", "hot", "wavefront", "aux", "no_records"] if group == "committed_and_hot" else SEEDED):
        header, record_bytes, restated = cases(name)
        sample = str(tmp_path / (name + ".bam"))
        lib.write_bgzf(sample, header + record_bytes, 0)
        pipeline.read_chimeric_alignments(sample)
        os.remove(sample)
        path = str(tmp_path / (name + ".tab"))
        stats = pipeline.write_gene_counts(path)
        text, expected = host_side(name)
        print(name, stats)
        assert open(path, "rb").read() == text and not os.path.exists(path + ".tmp"), name
        assert {key: stats[key] for key in COUNTED} == {key: expected[key] for key in COUNTED}, name
        assert pipeline.gene_counts_allocated_bytes() == 0 and stats["peak_bytes"] > 0, name
        _invariant(text, stats)
        if name == "hand_made":
            assert text == _golden("hand_made.tab")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", KNOBS, ids=["no_knobs", "ingest_windows", "hash_collisions"])
def test_device_equals_host_on_toy3k(knobs, built, toy3k, toy3k_pipeline, toy3k_host, tmp_path, monkeypatch):
    _set(knobs, monkeypatch)
    toy3k_pipeline.read_chimeric_alignments(toy3k[0] + ".bam")
    path = str(tmp_path / "counts.tab")
    stats = toy3k_pipeline.write_gene_counts(path)
    text, expected = toy3k_host
    assert open(path, "rb").read() == text and os.listdir(str(tmp_path)) == ["counts.tab"]
    assert {key: stats[key] for key in COUNTED} == {key: expected[key] for key in COUNTED}
    assert toy3k_pipeline.gene_counts_allocated_bytes() == 0
    _invariant(text, stats)


@pytest.fixture(scope="module")
def without_the_option(toy3k, tmp_path_factory):
    """fusions.tsv and discarded.tsv of toy3k from a run of the command line without --gene-counts"""
    directory = tmp_path_factory.mktemp("plain")
    outputs = [str(directory / "fusions.tsv"), str(directory / "discarded.tsv")]
    result = _command_line(toy3k[0] + ".bam", toy3k[0], outputs, [])
    assert result.returncode == 0, result.stderr[-2000:]
    assert "Counting reads per gene" not in result.stdout
    return [open(path, "rb").read() for path in outputs]


def _command_line(sample, prefix, outputs, extra):
    command = [WORKFLOW, "-x", sample, "-g", prefix + ".gtf", "-a", prefix + ".fa", "-o", outputs[0], "-O", outputs[1], "-f", "blacklist"]
    return subprocess.run(["timeout", "-k", "10", "120"] + command + extra, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)


@pytest.mark.gpu
@pytest.mark.parametrize("container", ["stored_bgzf", "deflated_bgzf", "sam_text"])
def test_command_line_writes_the_table_next_to_the_fusions(container, built, toy3k, toy3k_host, without_the_option, tmp_path):
    prefix, stream, text = toy3k
    os.mkdir(str(tmp_path / "in")); os.mkdir(str(tmp_path / "out"))
    sample = str(tmp_path / "in" / "sample.bam")
    if container == "sam_text":
        open(sample, "wb").write(text)
    else:
        lib.write_bgzf(sample, stream, 0 if container == "stored_bgzf" else 6)
    outputs = [str(tmp_path / "out" / "fusions.tsv"), str(tmp_path / "out" / "discarded.tsv")]
    result = _command_line(sample, prefix, outputs, ["--gene-counts", str(tmp_path / "out" / "counts.tab")])
    assert result.returncode == 0, result.stderr[-2000:]
    assert open(str(tmp_path / "out" / "counts.tab"), "rb").read() == toy3k_host[0]
    assert "Counting reads per gene (records=%d, " % toy3k_host[1]["records"] in result.stdout
    assert [open(path, "rb").read() for path in outputs] == without_the_option
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["counts.tab", "discarded.tsv", "fusions.tsv"]


@pytest.mark.gpu
def test_session_writes_the_table_of_the_sample_that_asked_for_it(built, toy3k, toy3k_host, without_the_option, tmp_path):
    """two samples in one session, the option on the first only: the second leaves no file, and no buffer of the option is left on either lane"""
    from arriba_amd.pipeline import WorkflowSession
    prefix = toy3k[0]
    session = WorkflowSession(prefix + ".fa", prefix + ".gtf", params={"disable_filters": ["blacklist"]})
    os.mkdir(str(tmp_path / "first")); os.mkdir(str(tmp_path / "second"))
    session.submit(prefix + ".bam", gene_counts_file=str(tmp_path / "first" / "counts.tab"))
    session.submit(prefix + ".bam")
    session.sample(prefix + ".bam", str(tmp_path / "first" / "fusions.tsv"))
    assert session.timing["gene_counts"] > 0
    session.sample(prefix + ".bam", str(tmp_path / "second" / "fusions.tsv"))
    assert session.timing["gene_counts"] == 0
    for context in session._lane_contexts():
        count = ctypes.c_uint64(1)
        assert session.api.gene_counts_allocated_bytes(context, ctypes.byref(count)) == 0 and count.value == 0
    session.close()
    assert sorted(os.listdir(str(tmp_path / "first"))) == ["counts.tab", "fusions.tsv"] and os.listdir(str(tmp_path / "second")) == ["fusions.tsv"]
    assert open(str(tmp_path / "first" / "counts.tab"), "rb").read() == toy3k_host[0]
    for directory in ("first", "second"):
        assert open(str(tmp_path / directory / "fusions.tsv"), "rb").read() == without_the_option[0]


@pytest.mark.gpu
def test_refusals_and_the_off_switch(built, toy3k, toy3k_host, tmp_path, monkeypatch):
    """with the option off no kernel whose name begins with genecount is in the kernel profile and no buffer of it exists; before an ingest, for a part of a sample and behind the
    begin of the next ingest agpu_gene_counts is refused with a message"""
    from arriba_amd import _capi
    from arriba_amd.pipeline import ArribaError, DevicePipeline, HostSession
    prefix = toy3k[0]
    api, params = _capi.bind_device_api(_capi.device_library(), "agpu_"), _capi.Params()
    api.default_params(ctypes.byref(params))
    fresh = api.create(0, ctypes.byref(params))
    assert fresh, api.last_error()
    room = np.zeros(3 * 4, dtype=np.uint64)
    refused = api.gene_counts(fresh, None, 0, room.ctypes.data, None)  # before an ingest
    message = api.last_error()
    api.destroy(fresh)
    assert refused != 0 and b"agpu_gene_counts: the record stream of the last ingest is not on the device any more" in message
    made = DevicePipeline(HostSession(prefix + ".fa", prefix + ".gtf"), bam=prefix + ".bam")
    made.set_profiling(True)
    made.read_chimeric_alignments(prefix + ".bam")
    made.run_workflow(str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv"))
    assert made.kernel_profile() and not [launch for launch in made.kernel_profile() if launch[0].startswith("genecount")] and made.gene_counts_allocated_bytes() == 0
    # ... and on, through the stages of the pipeline
    made.read_chimeric_alignments(prefix + ".bam")
    made.run_workflow(str(tmp_path / "again.tsv"), None, gene_counts_file=str(tmp_path / "counts.tab"))
    names = set(launch[0] for launch in made.kernel_profile())
    assert {"genecount_name_kernel", "genecount_assign_kernel"} <= names
    assert made.gene_counts_allocated_bytes() == 0
    assert open(str(tmp_path / "counts.tab"), "rb").read() == toy3k_host[0] and open(str(tmp_path / "again.tsv")).read() == open(str(tmp_path / "fusions.tsv")).read()
    # a part of a sample
    made._ingest_records(prefix + ".bam", False, 100, 64 << 20, part=0, parts=2)
    with pytest.raises(ArribaError, match="gene counts of one sample over several GPUs are not supported"):
        made.write_gene_counts(str(tmp_path / "part.tab"))
    # the stream was given back behind the ingest
    monkeypatch.setenv("ARRIBA_RELEASE_INGEST_BUFFERS", "1")
    made.read_chimeric_alignments(prefix + ".bam")
    monkeypatch.delenv("ARRIBA_RELEASE_INGEST_BUFFERS")
    with pytest.raises(ArribaError, match="agpu_gene_counts: the record stream of the last ingest is not on the device any more"):
        made.write_gene_counts(str(tmp_path / "gone.tab"))
    assert made.gene_counts_allocated_bytes() == 0
    # the next read_chimeric_alignments has begun
    made.read_chimeric_alignments(prefix + ".bam")
    host, handle, config = made.session._lib, made.session._session, _capi.IngestConfig()
    assert host.ahost_bam_open(handle, (prefix + ".bam").encode(), 0, 100, ctypes.byref(config)) == 0
    made._check(made.api.ingest_begin(made.ctx, ctypes.byref(config)))
    with pytest.raises(ArribaError, match="an ingest is under way|not on the device any more"):
        made.write_gene_counts(str(tmp_path / "second.tab"))
    host.ahost_bam_close(handle)
    made.close()
    assert sorted(os.listdir(str(tmp_path))) == ["again.tsv", "counts.tab", "discarded.tsv", "fusions.tsv"]
