"""--splice-junctions: the table of splice junctions of the records of -x, the file STAR writes as SJ.out.tab (the rule: DESIGN.md 4.16).

No program of the reference writes this file; the rule is the project's.  tests/golden/splice_junctions/hand_made.{fa,gtf,sam,tab} are a case a reader can check by eye, one
template per clause of the rule; tests/splice_junctions_lib.py restates the rule in plain Python with dicts and sets, test_restatement_equals_the_committed_file holds it to that
case, and only therefore it is the independent side for inputs made at test time.  The CPU tier runs arriba_amd/csrc/device/junction_core.hpp stepped on the host
(ahost_splice_junctions_*); the GPU tier the kernels of agpu_junctions.hip, whose file must equal the host's byte for byte and whose statistics must equal the host's."""
import ctypes
import os
import subprocess

import pytest

import conftest
import splice_junctions_lib as lib

GOLDEN = lib.GOLDEN
WORKFLOW = os.path.join(conftest.ROOT, "arriba_amd", "lib", "arriba_gpu_workflow")
SEEDED = ["seed%d" % (1600 + k) for k in range(50)]
COUNTED = lib.COUNTED  # what the device, the host and the restatement must agree on
MADE = {"hot": lib.hot_case, "wavefront": lib.wavefront_case, "long_cigar": lib.long_cigar_case, "aux": lib.aux_case, "no_n": lib.no_n_case, "no_records": lib.no_records_case, "empty": lib.empty_case}
HAND_MADE_STATS = {"records": 29, "contributing": 26, "crossings": 23, "pairs": 21, "junctions": 16, "annotated": 5}


def _golden(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


def _invariant(text, stats):
    """columns 7 and 8 sum to `pairs`, the file has `junctions` lines of nine fields, every line counts a template, and the lines ascend by (reference, s, e)"""
    rows = [line.split(b"\t") for line in text.split(b"\n")[:-1]]
    assert text == b"" or text.endswith(b"\n")
    assert len(rows) == stats["junctions"] and all(len(row) == 9 for row in rows)
    assert sum(int(row[6]) + int(row[7]) for row in rows) == stats["pairs"] <= stats["crossings"]
    assert all(int(row[6]) + int(row[7]) >= 1 and int(row[8]) >= 1 and int(row[1]) <= int(row[2]) for row in rows)
    assert sum(int(row[5]) for row in rows) == stats["annotated"]
    order = {name.encode(): k for k, (name, _) in enumerate(lib.HEADER)}
    keys = [(order[row[0]], int(row[1]), int(row[2])) for row in rows]
    assert keys == sorted(set(keys))
    return rows


@pytest.fixture(scope="module")
def annotation():
    return lib.load_annotation()


@pytest.fixture(scope="module")
def cases(annotation):
    """name -> (BAM header, record bytes, (text, stats) of the restatement, the case) on the committed annotation: made once"""
    cache = {}

    def get(name):
        if name not in cache:
            if name == "hand_made":
                case = lib.parse_sam(_golden("hand_made.sam"))
            elif name.startswith("seed"):
                case = lib.random_case(int(name[4:]), annotation)
            else:
                case = MADE[name]()
            cache[name] = (lib.bam_header(case[0]), lib.bam_records(case), lib.restate(annotation, case), case)
        return cache[name]
    return get


# ---- the host side ------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def committed_session(built):
    from arriba_amd.pipeline import HostSession
    session = HostSession(os.path.join(GOLDEN, "hand_made.fa"), os.path.join(GOLDEN, "hand_made.gtf"), interesting_contigs=lib.COMMITTED_CONTIGS)
    yield session
    session.close()


def _stats():
    from arriba_amd import _capi
    return _capi.JunctionStats()


def _host_junctions(session, header, record_bytes):
    """-> (text, statistics) of ahost_splice_junctions_of + ahost_splice_junctions_text"""
    from arriba_amd import _capi
    from arriba_amd.pipeline import junction_stats_of
    host, handle = session._lib, session._session
    rows, n_rows, stats, contigs = ctypes.POINTER(_capi.JunctionRow)(), ctypes.c_uint64(), _stats(), _capi.DepthContigs()
    assert host.ahost_splice_junctions_of(handle, header, len(header), record_bytes, len(record_bytes), ctypes.byref(rows), ctypes.byref(n_rows), ctypes.byref(stats)) == 0, host.ahost_last_error()
    assert host.ahost_depth_contigs_of(header, len(header), ctypes.byref(contigs)) == 0, host.ahost_last_error()
    text, size = ctypes.c_void_p(), ctypes.c_uint64()
    assert host.ahost_splice_junctions_text(ctypes.byref(contigs), rows, n_rows.value, ctypes.byref(text), ctypes.byref(size)) == 0, host.ahost_last_error()
    return ctypes.string_at(text, size.value), junction_stats_of(stats)


@pytest.fixture(scope="module")
def host_side(cases, committed_session):
    """name -> what the host stepping gives: computed once, compared against by every test"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = _host_junctions(committed_session, *cases(name)[:2])
        return cache[name]
    return get


# ---- CPU tier -----------------------------------------------------------------------------------------------------------------------------------------------------

def test_restatement_equals_the_committed_file(annotation):
    """the restatement of the rule against the case that is checked by eye"""
    case = lib.parse_sam(_golden("hand_made.sam"))
    text, stats = lib.restate(annotation, case)
    assert text == _golden("hand_made.tab")
    assert stats == HAND_MADE_STATS
    assert case[0] == lib.HEADER and set(annotation["sequences"]) == {"j1", "j2", "j3"} and len(annotation["sequences"]["j3"]) == 200 < dict(lib.HEADER)["j3"]
    assert all(len(_golden("hand_made." + kind)) < 100000 for kind in ("fa", "gtf", "sam", "tab"))
    rows = _invariant(text, stats)
    assert set(int(row[4]) for row in rows) == set(range(7)) and set(int(row[3]) for row in rows) == {0, 1, 2}
    assert [row for row in rows if row[4] == b"0" and row[5] == b"1" and row[3] == b"0"], "the annotated intron of genes of both strands"


def test_host_gives_the_committed_bytes(built, cases, host_side, committed_session, tmp_path):
    text, stats = host_side("hand_made")
    assert text == _golden("hand_made.tab")
    assert {key: stats[key] for key in COUNTED} == HAND_MADE_STATS == cases("hand_made")[2][1]
    # ... and through the project's own readers of SAM text and of BAM, which leave no temporary file
    host = committed_session._lib
    sample = str(tmp_path / "hand_made.bam")
    lib.write_bgzf(sample, cases("hand_made")[0] + cases("hand_made")[1], 6)
    for source in (os.path.join(GOLDEN, "hand_made.sam"), sample):
        path, counted = str(tmp_path / "junctions.tab"), _stats()
        assert host.ahost_splice_junctions_file(committed_session._session, source.encode(), path.encode(), ctypes.byref(counted)) == 0, host.ahost_last_error()
        assert open(path, "rb").read() == text and counted.pairs == 21 and sorted(os.listdir(str(tmp_path))) == ["hand_made.bam", "junctions.tab"]
        os.remove(path)
    assert host.ahost_splice_junctions_file(committed_session._session, sample.encode(), str(tmp_path / "missing" / "junctions.tab").encode(), None) != 0
    assert sorted(os.listdir(str(tmp_path))) == ["hand_made.bam"]


def test_the_corners_of_the_nh_walk(built, cases, host_side):
    """NH:Z in front of NH:i counts as 1 (the first field named NH decides); a B array longer than its record, a field of an unknown type and a Z field without its end in front of
    NH:i:5 end the walk (1); NH:i:5 alone and behind a well-formed B array is multimapping.  The numbers are written out here, not taken from the restatement"""
    text, stats = host_side("aux")
    assert text == cases("aux")[2][0] == b"j1\t61\t80\t2\t2\t0\t4\t2\t10\n"
    assert stats["contributing"] == 6 and stats["crossings"] == 6 and stats["pairs"] == 6
    _invariant(text, stats)


@pytest.mark.parametrize("name", ["seeded", "hot", "wavefront", "long_cigar", "no_n", "no_records", "empty"])
def test_host_equals_the_restatement(name, built, cases, host_side):
    """file and statistics, and the sum invariant: the total of columns 7 and 8 equals `pairs`, the number of lines `junctions`"""
    seen = {"motif": set(), "strand": set(), "annotated": set(), "multimapping": 0, "shared": 0}
    for case in (SEEDED if name == "seeded" else [name]):
        text, stats = host_side(case)
        expected_text, expected = cases(case)[2]
        assert expected["records"] <= (400 if name == "seeded" else 1 << 17)
        assert text == expected_text, case
        assert {key: stats[key] for key in COUNTED} == expected, case
        for row in _invariant(text, stats):
            seen["motif"].add(int(row[4])); seen["strand"].add(int(row[3])); seen["annotated"].add(int(row[5]))
            seen["multimapping"] += int(row[7]); seen["shared"] += int(row[6]) + int(row[7]) > 1
    if name == "seeded":  # the seeded set as a whole exercises the rule
        assert seen["motif"] == set(range(7)) and seen["strand"] == {0, 1, 2} and seen["annotated"] == {0, 1} and seen["multimapping"] > 100 and seen["shared"] > 400
        assert any(cases(case)[2][1]["pairs"] < cases(case)[2][1]["crossings"] for case in SEEDED)
    if name == "hot":
        assert text.startswith(b"j1\t21\t40\t1\t1\t1\t69931\t70\t9\n") and 69931 > 1 << 16 and stats["pairs"] == 70065 and stats["crossings"] == 80066
    if name == "wavefront":
        assert text == b"j1\t61\t80\t2\t2\t0\t64\t1\t10\n"
    if name == "long_cigar":
        assert stats["junctions"] == 301 and stats["crossings"] == 306 and b"orphan\t103\t105\t0\t0\t0\t0\t1\t2\n" in text
    if name == "no_n":
        assert text == b"" and stats["contributing"] == 26 and stats["crossings"] == 0
    if name in ("no_records", "empty"):
        assert text == b"" and stats["records"] == 0


def _harness(target):
    directory = os.path.join(conftest.ROOT, "tests", "emu")
    subprocess.run(["make", "-s", "-C", directory, target], check=True)
    return os.path.join(directory, target)


def _arguments(sample, outputs, extra):
    return ["-x", sample, "-g", os.path.join(GOLDEN, "hand_made.gtf"), "-a", os.path.join(GOLDEN, "hand_made.fa"), "-i", lib.COMMITTED_CONTIGS, "-o", outputs[0], "-O", outputs[1], "-f", "blacklist"] + extra


def test_host_ingest_through_the_command_line(built, emu_api, tmp_path):
    """--host-ingest --splice-junctions: the C++ driver (over the host stepping harness, where there is no GPU) writes the committed table, and fusions.tsv is the one of a run
    without the option"""
    sample = os.path.join(GOLDEN, "hand_made.sam")
    files = {}
    for option in ([], ["--splice-junctions", str(tmp_path / "junctions.tab")]):
        outputs = [str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv")]
        result = subprocess.run([_harness("workflow_on_harness")] + _arguments(sample, outputs, ["--host-ingest"] + option), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
        assert result.returncode == 0, result.stderr[-2000:]
        assert ("Finding splice junctions (records=29, contributing=26, crossings=23, pairs=21, junctions=16, annotated=5)" in result.stdout) == bool(option)
        files[bool(option)] = [open(path, "rb").read() for path in outputs]
    assert open(str(tmp_path / "junctions.tab"), "rb").read() == _golden("hand_made.tab")
    assert files[True] == files[False] and sorted(os.listdir(str(tmp_path))) == ["discarded.tsv", "fusions.tsv", "junctions.tab"]


def test_a_path_in_a_missing_directory_is_refused_at_the_command_line(built, tmp_path):
    command = [WORKFLOW] + _arguments(os.path.join(GOLDEN, "hand_made.sam"), [str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv")], ["--splice-junctions", str(tmp_path / "missing" / "junctions.tab")])
    result = subprocess.run(command, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=60)
    assert result.returncode == 1 and "parent directory of output file" in result.stderr and "junctions.tab" in result.stderr
    assert os.listdir(str(tmp_path)) == []
    assert "--splice-junctions FILE" in subprocess.run([WORKFLOW, "-h"], stdout=subprocess.PIPE, universal_newlines=True, timeout=60).stdout


def test_cpp_driver_on_the_harness_says_that_it_has_no_device_library(built, emu_api, tmp_path):
    """the test-only build of the C++ driver against the host stepping harness has no twin of the kernels of agpu_junctions.hip: it links all the same and says so before the feed"""
    command = [_harness("workflow_on_harness")] + _arguments(os.path.join(GOLDEN, "hand_made.sam"), [str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv")], ["--splice-junctions", str(tmp_path / "junctions.tab")])
    result = subprocess.run(command, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert result.returncode != 0 and "--splice-junctions needs the device library (agpu_splice_junctions)" in result.stderr
    assert not os.path.exists(str(tmp_path / "junctions.tab")) and not os.path.exists(str(tmp_path / "junctions.tab.tmp"))


def test_a_sample_over_ranks_is_refused_before_the_feed(built, emu_api, tmp_path):
    """one sample over several ranks: refused before a byte of the file is fed (the driver over the harness, a communicator of one rank that does nothing)"""
    from arriba_amd import _capi
    driver = ctypes.CDLL(_harness("libworkflow_on_harness.so"))
    driver.arriba_workflow_open.restype = ctypes.c_void_p
    driver.arriba_workflow_last_error.restype = ctypes.c_char_p
    options = _capi.WorkflowOptions()
    driver.arriba_workflow_default_options(ctypes.byref(options))
    assert options.splice_junctions_file is None
    options.assembly_file, options.gene_annotation_file, options.interesting_contigs = os.path.join(GOLDEN, "hand_made.fa").encode(), os.path.join(GOLDEN, "hand_made.gtf").encode(), lib.COMMITTED_CONTIGS.encode()
    session = ctypes.c_void_p(driver.arriba_workflow_open(ctypes.byref(options)))
    assert session, driver.arriba_workflow_last_error()
    nothing = lambda *arguments: 0  # noqa: E731
    communicator = _capi.WorkflowCommunicator(0, 1, None, _capi.ALL_GATHER(nothing), _capi.ALL_REDUCE_INT64(nothing), _capi.ALL_REDUCE_MAX_BYTES(nothing), None)
    assert driver.arriba_workflow_set_communicator(session, ctypes.byref(communicator)) == 0
    driver.arriba_workflow_splice_junctions.argtypes = [ctypes.c_void_p, ctypes.c_char_p]
    assert driver.arriba_workflow_splice_junctions(session, str(tmp_path / "junctions.tab").encode()) == 0
    status = driver.arriba_workflow_sample(session, os.path.join(GOLDEN, "hand_made.sam").encode(), str(tmp_path / "fusions.tsv").encode(), None, None, None)
    message = driver.arriba_workflow_last_error().decode()
    driver.arriba_workflow_close(session)
    assert status != 0 and "ERROR: splice junctions of one sample over several GPUs are not supported" in message
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


KNOBS = [{}, {"ARRIBA_INGEST_WINDOWS": "1048576,65536"}, {"ARRIBA_JUNCTION_HASH_BITS": "4"}]


def _set(knobs, monkeypatch):
    for knob in ("ARRIBA_INGEST_WINDOWS", "ARRIBA_JUNCTION_HASH_BITS"):
        if knob in knobs:
            monkeypatch.setenv(knob, knobs[knob])
        else:
            monkeypatch.delenv(knob, raising=False)


def _device_junctions(pipeline, cases, name, tmp_path):
    """the case through an ingest and agpu_splice_junctions -> (the bytes of the file, the statistics)"""
    header, record_bytes = cases(name)[:2]
    sample = str(tmp_path / (name + ".bam"))
    lib.write_bgzf(sample, header + record_bytes, 0)
    pipeline.read_chimeric_alignments(sample)
    os.remove(sample)
    path = str(tmp_path / (name + ".tab"))
    stats = pipeline.write_splice_junctions(path)
    text = open(path, "rb").read()
    assert not os.path.exists(path + ".tmp") and pipeline.splice_junctions_allocated_bytes() == 0, name
    os.remove(path)
    return text, stats


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["committed_and_made", "seeded"])
@pytest.mark.parametrize("knobs", KNOBS, ids=["no_knobs", "ingest_windows", "hash_collisions"])
def test_device_file_is_the_host_file(knobs, group, built, pipeline, cases, host_side, tmp_path, monkeypatch):
    """the file of agpu_splice_junctions equals the host stepping byte for byte and the statistics are equal: the committed case, the hot junction (70 001 templates over one intron),
    65 templates, one record with 300 N operations beside records with none, the corners of the NH walk, an input without any N, a header without records; 50 seeded inputs in one
    session; with the ingest cut into windows; with four bits of the hash of a read name, so that every insert collides"""
    _set(knobs, monkeypatch)
    peak = {}
    for name in (["hand_made", "hot", "wavefront", "long_cigar", "aux", "no_n", "no_records"] if group == "committed_and_made" else SEEDED):
        text, stats = _device_junctions(pipeline, cases, name, tmp_path)
        expected_text, expected = host_side(name)
        print(name, stats)
        assert text == expected_text, name
        assert {key: stats[key] for key in COUNTED} == {key: expected[key] for key in COUNTED}, name
        assert (stats["peak_bytes"] > 0) == (stats["records"] > 0), name
        _invariant(text, stats)
        peak[name] = stats["peak_bytes"]
        if name == "hand_made":
            assert text == _golden("hand_made.tab")
    if group == "committed_and_made":  # the same records and names without any N: no name table, no tuple buffer
        assert 0 < peak["no_n"] < peak["hand_made"]


@pytest.mark.gpu
def test_device_on_the_empty_input(built, pipeline, cases, host_side, tmp_path):
    """no reference and no record"""
    text, stats = _device_junctions(pipeline, cases, "empty", tmp_path)
    assert text == b"" == host_side("empty")[0] and {key: stats[key] for key in COUNTED} == dict.fromkeys(COUNTED, 0) and stats["peak_bytes"] == 0


def _command_line(sample, outputs, extra):
    return subprocess.run(["timeout", "-k", "10", "120", WORKFLOW] + _arguments(sample, outputs, extra), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)


@pytest.fixture(scope="module")
def without_the_option(tmp_path_factory):
    """fusions.tsv and discarded.tsv of the committed case from a run of the command line without --splice-junctions"""
    directory = tmp_path_factory.mktemp("plain")
    outputs = [str(directory / "fusions.tsv"), str(directory / "discarded.tsv")]
    result = _command_line(os.path.join(GOLDEN, "hand_made.sam"), outputs, [])
    assert result.returncode == 0, result.stderr[-2000:]
    assert "Finding splice junctions" not in result.stdout
    return [open(path, "rb").read() for path in outputs]


@pytest.mark.gpu
@pytest.mark.parametrize("container", ["stored_bgzf", "deflated_bgzf", "sam_text", "host_ingest"])
def test_command_line_writes_the_table_next_to_the_fusions(container, built, cases, without_the_option, tmp_path):
    """the committed case as BAM and as SAM text, and with --host-ingest: the committed table, and the other outputs as without the option"""
    os.mkdir(str(tmp_path / "in")); os.mkdir(str(tmp_path / "out"))
    sample = str(tmp_path / "in" / "sample.bam")
    if container in ("sam_text", "host_ingest"):
        sample = os.path.join(GOLDEN, "hand_made.sam")
    else:
        lib.write_bgzf(sample, cases("hand_made")[0] + cases("hand_made")[1], 0 if container == "stored_bgzf" else 6)
    outputs = [str(tmp_path / "out" / "fusions.tsv"), str(tmp_path / "out" / "discarded.tsv")]
    result = _command_line(sample, outputs, ["--splice-junctions", str(tmp_path / "out" / "junctions.tab")] + (["--host-ingest"] if container == "host_ingest" else []))
    assert result.returncode == 0, result.stderr[-2000:]
    assert open(str(tmp_path / "out" / "junctions.tab"), "rb").read() == _golden("hand_made.tab")
    assert "Finding splice junctions (records=29, contributing=26, crossings=23, pairs=21, junctions=16, annotated=5)" in result.stdout
    assert [open(path, "rb").read() for path in outputs] == without_the_option
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["discarded.tsv", "fusions.tsv", "junctions.tab"]


@pytest.mark.gpu
def test_session_writes_the_table_of_the_sample_that_asked_for_it(built, without_the_option, tmp_path):
    """two samples in a queue, the option on the second only: the first leaves no file, and no buffer of the option is left on either lane"""
    from arriba_amd.pipeline import WorkflowSession
    sample = os.path.join(GOLDEN, "hand_made.sam")
    session = WorkflowSession(os.path.join(GOLDEN, "hand_made.fa"), os.path.join(GOLDEN, "hand_made.gtf"), interesting_contigs=lib.COMMITTED_CONTIGS, params={"disable_filters": ["blacklist"]})
    os.mkdir(str(tmp_path / "first")); os.mkdir(str(tmp_path / "second"))
    session.submit(sample)
    session.submit(sample, splice_junctions_file=str(tmp_path / "second" / "junctions.tab"))
    session.sample(sample, str(tmp_path / "first" / "fusions.tsv"))
    assert session.timing["splice_junctions"] == 0
    session.sample(sample, str(tmp_path / "second" / "fusions.tsv"))
    assert session.timing["splice_junctions"] > 0
    for context in session._lane_contexts():
        count = ctypes.c_uint64(1)
        assert session.api.splice_junctions_allocated_bytes(context, ctypes.byref(count)) == 0 and count.value == 0
    session.close()
    assert os.listdir(str(tmp_path / "first")) == ["fusions.tsv"] and sorted(os.listdir(str(tmp_path / "second"))) == ["fusions.tsv", "junctions.tab"]
    assert open(str(tmp_path / "second" / "junctions.tab"), "rb").read() == _golden("hand_made.tab")
    for directory in ("first", "second"):
        assert open(str(tmp_path / directory / "fusions.tsv"), "rb").read() == without_the_option[0]


@pytest.mark.gpu
def test_refusals_and_the_off_switch(built, cases, tmp_path, monkeypatch):
    """with the option off no kernel whose name begins with junction is in the kernel profile and no buffer of it exists; before an ingest, for a part of a sample, with the stream
    given back and behind the begin of the next ingest agpu_splice_junctions is refused with a message"""
    from arriba_amd import _capi
    from arriba_amd.pipeline import ArribaError, DevicePipeline, HostSession
    api, params = _capi.bind_device_api(_capi.device_library(), "agpu_"), _capi.Params()
    api.default_params(ctypes.byref(params))
    fresh = api.create(0, ctypes.byref(params))
    assert fresh, api.last_error()
    rows, n_rows = ctypes.POINTER(_capi.JunctionRow)(), ctypes.c_uint64()
    refused = api.splice_junctions(fresh, None, 0, ctypes.byref(rows), ctypes.byref(n_rows), None)  # before an ingest
    message = api.last_error()
    api.destroy(fresh)
    assert refused != 0 and b"agpu_splice_junctions: the record stream of the last ingest is not on the device any more" in message
    sample = os.path.join(GOLDEN, "hand_made.sam")
    made = DevicePipeline(HostSession(os.path.join(GOLDEN, "hand_made.fa"), os.path.join(GOLDEN, "hand_made.gtf"), interesting_contigs=lib.COMMITTED_CONTIGS), bam=sample)
    made.set_profiling(True)
    made.read_chimeric_alignments(sample)
    made.run_workflow(str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv"))
    assert made.kernel_profile() and not [launch for launch in made.kernel_profile() if launch[0].startswith("junction")] and made.splice_junctions_allocated_bytes() == 0
    # ... and on, through the stages of the pipeline
    made.read_chimeric_alignments(sample)
    made.run_workflow(str(tmp_path / "again.tsv"), None, splice_junctions_file=str(tmp_path / "junctions.tab"))
    names = set(launch[0] for launch in made.kernel_profile())
    assert {"junction_count_kernel", "junction_name_kernel", "junction_emit_kernel", "junction_head_kernel", "junction_reduce_kernel", "junction_intron_kernel", "junction_class_kernel"} <= names
    assert made.splice_junctions_allocated_bytes() == 0
    assert open(str(tmp_path / "junctions.tab"), "rb").read() == _golden("hand_made.tab") and open(str(tmp_path / "again.tsv")).read() == open(str(tmp_path / "fusions.tsv")).read()
    # a part of a sample (which only a BAM file has)
    os.mkdir(str(tmp_path / "in"))
    lib.write_bgzf(str(tmp_path / "in" / "hand_made.bam"), cases("hand_made")[0] + cases("hand_made")[1], 0)
    made._ingest_records(str(tmp_path / "in" / "hand_made.bam"), False, 100, 64 << 20, part=0, parts=2)
    with pytest.raises(ArribaError, match="splice junctions of one sample over several GPUs are not supported"):
        made.write_splice_junctions(str(tmp_path / "part.tab"))
    # the stream was given back behind the ingest: no ingest kept
    monkeypatch.setenv("ARRIBA_RELEASE_INGEST_BUFFERS", "1")
    made.read_chimeric_alignments(sample)
    monkeypatch.delenv("ARRIBA_RELEASE_INGEST_BUFFERS")
    with pytest.raises(ArribaError, match="agpu_splice_junctions: the record stream of the last ingest is not on the device any more"):
        made.write_splice_junctions(str(tmp_path / "gone.tab"))
    assert made.splice_junctions_allocated_bytes() == 0
    # the next read_chimeric_alignments has begun
    made.read_chimeric_alignments(sample)
    host, handle, config = made.session._lib, made.session._session, _capi.IngestConfig()
    assert host.ahost_bam_open(handle, sample.encode(), 0, 100, ctypes.byref(config)) == 0
    made._check(made.api.ingest_begin(made.ctx, ctypes.byref(config)))
    with pytest.raises(ArribaError, match="an ingest is under way|not on the device any more"):
        made.write_splice_junctions(str(tmp_path / "second.tab"))
    host.ahost_bam_close(handle)
    made.close()
    assert sorted(os.listdir(str(tmp_path))) == ["again.tsv", "discarded.tsv", "fusions.tsv", "in", "junctions.tab"]
