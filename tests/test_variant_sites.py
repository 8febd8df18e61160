"""--variant-sites: the positions at which the records of -x show a base that differs from -a, with their base counts (the rule: DESIGN.md 4.21).

No program of the reference writes this file; the rule is the project's.  tests/golden/variant_sites/hand_made.{sam,tsv} (on tests/golden/allele_counts/hand_made.{fa,gtf}) are a
case a reader can check by eye; tests/variant_sites_lib.py restates the rule in plain Python with dicts, test_restatement_equals_the_committed_file holds it to that case, and only
therefore it is the independent side for inputs made at test time.  The CPU tier runs variant_core.hpp and allele_core.hpp stepped on the host (ahost_variant_sites_*); the GPU
tier the kernels of agpu_variants.hip, whose file must equal the host's and the restatement's byte for byte."""
import ctypes
import os
import subprocess

import pytest

import conftest
import variant_sites_lib as lib

GOLDEN = lib.GOLDEN
FASTA, GTF = os.path.join(lib.ALLELE_GOLDEN, "hand_made.fa"), os.path.join(lib.ALLELE_GOLDEN, "hand_made.gtf")
SAM = os.path.join(GOLDEN, "hand_made.sam")
WORKFLOW = os.path.join(conftest.ROOT, "arriba_amd", "lib", "arriba_gpu_workflow")
COUNTED = lib.COUNTED
CASES = ["hand_made"] + list(lib.MADE)
HAND_MADE_STATS = {"records": 22, "contributing": 21, "events": 13, "runs": 7, "candidates": 5, "reported": 4}
HAND_MADE_LINE = "Finding variant sites (records=22, contributing=21, events=13, runs=7, candidates=5, reported=4)"
HAND_MADE_OPTIONS = ["--variant-min-mapq", "20", "--variant-min-baseq", "13", "--variant-min-alt", "2", "--variant-min-percent", "50"]
SEVERAL_GPUS = "variant sites of one sample over several GPUs are not supported"


def _golden(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


def _thresholds(case):
    return case["min_mapq"], case["min_baseq"], case["min_alt"], case["min_percent"]


@pytest.fixture(scope="module")
def assembly():
    return lib.load_assembly()


@pytest.fixture(scope="module")
def cases(assembly):
    """name -> (BAM header, record bytes, (text, stats) of the restatement, the case): made once"""
    cache = {}

    def get(name):
        if name not in cache:
            case = lib.committed_case() if name == "hand_made" else lib.MADE[name](assembly)
            cache[name] = (lib.bam_header(case["references"]), lib.bam_records(case), lib.restate(assembly, case), case)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def committed_session(built):
    from arriba_amd.pipeline import HostSession
    session = HostSession(FASTA, GTF, interesting_contigs=lib.COMMITTED_CONTIGS)
    yield session
    session.close()


def _host_sites(session, header, record_bytes, case):
    """-> (text, statistics) of ahost_variant_sites_of + ahost_variant_sites_text"""
    from arriba_amd import _capi
    from arriba_amd.pipeline import variant_stats_of
    host, handle = session._lib, session._session
    rows, n_rows, stats, contigs = ctypes.POINTER(_capi.VariantRow)(), ctypes.c_uint64(), _capi.VariantStats(), _capi.DepthContigs()
    assert host.ahost_variant_sites_of(handle, header, len(header), record_bytes, len(record_bytes), *_thresholds(case), ctypes.byref(rows), ctypes.byref(n_rows), ctypes.byref(stats)) == 0, host.ahost_last_error()
    assert host.ahost_depth_contigs_of(header, len(header), ctypes.byref(contigs)) == 0, host.ahost_last_error()
    text, size = ctypes.c_void_p(), ctypes.c_uint64()
    assert host.ahost_variant_sites_text(ctypes.byref(contigs), rows, n_rows.value, ctypes.byref(text), ctypes.byref(size)) == 0, host.ahost_last_error()
    assert n_rows.value == stats.reported
    return ctypes.string_at(text, size.value), variant_stats_of(stats)


@pytest.fixture(scope="module")
def host_side(cases, committed_session):
    """name -> what the host stepping gives: computed once, compared against by every test"""
    cache = {}

    def get(name):
        if name not in cache:
            header, record_bytes, _, case = cases(name)
            cache[name] = _host_sites(committed_session, header, record_bytes, case)
        return cache[name]
    return get


# ---- CPU tier -----------------------------------------------------------------------------------------------------------------------------------------------------

def test_restatement_equals_the_committed_file(assembly):
    """the restatement of the rule against the case that is checked by eye"""
    text, stats = lib.restate(assembly, lib.committed_case())
    assert text == _golden("hand_made.tsv")
    assert stats == HAND_MADE_STATS
    assert len(_golden("hand_made.sam")) < 10000 and len(lib.committed_case()["records"]) == 22
    lines = text.decode().split("\n")
    assert lines[0] + "\n" == lib.HEADER_LINE and "a1\t33\tG\tA,T\t2\t0\t0\t2\t0\t1\t0\t0" in lines and not [line for line in lines if line.startswith(("chr2", "orphan", "a1\t43"))]


def test_the_made_cases_hold_what_they_are_for(cases):
    """the shapes the kernels can go wrong at are in the cases, by what the restatement finds in them"""
    text = {name: cases(name)[2][0].decode() for name in lib.MADE}
    stats = {name: cases(name)[2][1] for name in lib.MADE}
    assert {1, 7, 63, 64, 65, 128, 129} <= set(len(record[6]) for record in cases("lanes")[3]["records"])
    for line in ("a1\t1\t", "a1\t64\t", "a1\t65\t", "a1\t100\t", "a1\t12\t", "a1\t21\t", "a1\t31\t", "a1\t80\t", "a1\t44\t", "a1\t45\t", "chr2\t13\t", "chr2\t27\t"):
        assert "\n" + line in text["lanes"], line
    assert "\na1\t98\t" in text["edges"] and "\na1\t100\t" in text["edges"] and "\nchr2\t50\t" in text["edges"] and "\na1\t1\t" in text["edges"] and "orphan" not in text["edges"] and "\na1\t55\t" not in text["edges"]
    assert "\na1\t22\tC\t" in text["edges"] and "\na1\t67\tG\tA,T\t" in text["edges"] and "\na1\t63\t" not in text["edges"]
    assert "\na1\t100\t" in text["long_header"] and "\na1\t101\t" not in text["long_header"] and stats["long_header"]["events"] == 12
    assert stats["filters"]["contributing"] == 9 and "\nchr2\t5\tC\t" in text["filters"] and text["filters"].count("\n") == 6
    assert [line for line in text["filters"].split("\n") if line.startswith("chr2\t5\t")][0].split("\t")[-1] == "2"  # (LOWQ: quality 12 and quality 0; quality 13 and 0xFF are the two events)
    counting = {tuple(line.split("\t")[:2]): line.split("\t") for line in text["counting"].split("\n")[1:-1]}
    assert counting[("a1", "50")][3:] == ["G", "0", "0", "200", "0", "0", "2", "1", "0"]
    assert counting[("a1", "10")][2:8] == ["C", "A,T", "3", "2", "0", "3"] and counting[("a1", "12")][2:8] == ["T", "A", "4", "2", "1", "1"] and ("a1", "14") not in counting
    assert ("a1", "20") not in counting and ("a1", "21") in counting and {("a1", "70"), ("a1", "71"), ("a1", "72"), ("chr2", "20"), ("chr2", "21")} <= set(counting)
    assert [line.split("\t")[:2] for line in text["percent"].split("\n")[1:-1]] == [["a1", "10"], ["chr2", "5"]] and stats["percent"]["candidates"] == 3
    assert stats["seeded"]["records"] == 2000 and stats["seeded"]["events"] > 500 and stats["seeded"]["reported"] >= 4 and stats["seeded"]["candidates"] > stats["seeded"]["reported"]
    for name in ("no_records", "no_mismatch", "no_references"):
        assert text[name] == lib.HEADER_LINE
    assert stats["no_mismatch"]["contributing"] == 40


def test_host_gives_the_committed_bytes(built, cases, host_side, committed_session, tmp_path):
    from arriba_amd import _capi
    text, stats = host_side("hand_made")
    assert text == _golden("hand_made.tsv")
    assert {key: stats[key] for key in COUNTED} == HAND_MADE_STATS and stats["inconsistent"] == 0
    # ... and through the project's own readers of SAM text and of BAM, which leave no temporary file
    host = committed_session._lib
    sample = str(tmp_path / "hand_made.bam")
    lib.write_bgzf(sample, cases("hand_made")[0] + cases("hand_made")[1], 6)
    for source in (SAM, sample):
        path, found = str(tmp_path / "variants.tsv"), _capi.VariantStats()
        assert host.ahost_variant_sites_file(committed_session._session, source.encode(), path.encode(), 20, 13, 2, 50, ctypes.byref(found)) == 0, host.ahost_last_error()
        assert open(path, "rb").read() == text and found.events == 13 and sorted(os.listdir(str(tmp_path))) == ["hand_made.bam", "variants.tsv"]
        os.remove(path)
    assert host.ahost_variant_sites_file(committed_session._session, sample.encode(), str(tmp_path / "missing" / "variants.tsv").encode(), 20, 13, 2, 50, None) != 0
    assert sorted(os.listdir(str(tmp_path))) == ["hand_made.bam"]
    # the thresholds are part of the result: with min_alt 1 and no percent test s1 opens a1 43 and chr2 5 is reported; with MAPQ 19 admitted m1 counts as well
    assert host.ahost_variant_sites_file(committed_session._session, sample.encode(), str(tmp_path / "open.tsv").encode(), 19, 0, 1, 0, None) == 0
    lines = open(str(tmp_path / "open.tsv")).read().split("\n")
    assert "a1\t43\tT\tG\t0\t0\t2\t0\t0\t0\t0\t0" in lines and "chr2\t5\tC\tT\t0\t3\t0\t2\t0\t0\t0\t0" in lines and "a1\t48\tA\tC\t0\t3\t0\t0\t0\t0\t0\t0" in lines
    # thresholds the rule does not admit
    rows, n_rows = ctypes.POINTER(_capi.VariantRow)(), ctypes.c_uint64()
    for thresholds, message in (((256, 13, 3, 5), "a threshold above 255"), ((20, 256, 3, 5), "a threshold above 255"), ((20, 13, 0, 5), "min_alt is 1 to 2^31-1"), ((20, 13, 2 ** 31, 5), "min_alt is 1 to 2^31-1"), ((20, 13, 3, 101), "min_percent is 0 to 100")):
        assert host.ahost_variant_sites_of(committed_session._session, cases("hand_made")[0], len(cases("hand_made")[0]), None, 0, *thresholds, ctypes.byref(rows), ctypes.byref(n_rows), None) != 0
        assert message in host.ahost_last_error().decode()


@pytest.mark.parametrize("name", list(lib.MADE))
def test_host_equals_the_restatement(name, built, cases, host_side):
    text, stats = host_side(name)
    expected_text, expected = cases(name)[2]
    assert text == expected_text
    assert {key: stats[key] for key in COUNTED} == expected and stats["inconsistent"] == 0


def _harness(target):
    directory = os.path.join(conftest.ROOT, "tests", "emu")
    subprocess.run(["make", "-s", "-C", directory, target], check=True)
    return os.path.join(directory, target)


def _arguments(sample, outputs, extra):
    return ["-x", sample, "-g", GTF, "-a", FASTA, "-i", lib.COMMITTED_CONTIGS, "-o", outputs[0], "-O", outputs[1], "-f", "blacklist"] + extra


def test_host_ingest_through_the_command_line(built, emu_api, tmp_path):
    """--host-ingest --variant-sites: the C++ driver (over the host stepping harness, where there is no GPU) writes the committed table, and fusions.tsv and discarded.tsv are
    those of a run without the option"""
    files = {}
    for option in ([], ["--variant-sites", str(tmp_path / "variants.tsv")] + HAND_MADE_OPTIONS):
        outputs = [str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv")]
        result = subprocess.run([_harness("workflow_on_harness")] + _arguments(SAM, outputs, ["--host-ingest"] + option), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
        assert result.returncode == 0, result.stderr[-2000:]
        assert (HAND_MADE_LINE in result.stdout) == bool(option) and ("Finding variant sites" in result.stdout) == bool(option)
        files[bool(option)] = [open(path, "rb").read() for path in outputs]
    assert open(str(tmp_path / "variants.tsv"), "rb").read() == _golden("hand_made.tsv")
    assert files[True] == files[False] and sorted(os.listdir(str(tmp_path))) == ["discarded.tsv", "fusions.tsv", "variants.tsv"]


def _refused(command, tmp_path, message):
    result = subprocess.run(command, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert result.returncode != 0 and message in result.stderr, (message, result.stderr[-2000:])
    assert not [name for name in os.listdir(str(tmp_path)) if name.startswith(("variants", "fusions", "discarded"))], os.listdir(str(tmp_path))


def _workflow_options(driver):
    from arriba_amd import _capi
    options = _capi.WorkflowOptions()
    driver.arriba_workflow_default_options(ctypes.byref(options))
    options.assembly_file, options.gene_annotation_file, options.interesting_contigs = FASTA.encode(), GTF.encode(), lib.COMMITTED_CONTIGS.encode()
    return options


def test_refusals_before_the_input_is_read(built, emu_api, tmp_path):
    """a threshold without the file, thresholds out of their range, a path in a missing directory, -c: refused with --host-ingest as without it, before the feed, and nothing is
    written.  The test-only build of the C++ driver against the host stepping harness has no twin of the kernels of agpu_variants.hip: without --host-ingest it says so, also
    before the feed.  The defaults and the usage text"""
    outputs, table = [str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv")], str(tmp_path / "variants.tsv")
    for ingest in (["--host-ingest"], []):
        command = [_harness("workflow_on_harness")] + _arguments(SAM, outputs, ingest)
        for threshold in ("--variant-min-alt", "--variant-min-percent", "--variant-min-mapq", "--variant-min-baseq"):
            _refused(command + [threshold, "7"], tmp_path, "need --variant-sites")
        _refused(command + ["--variant-sites", table, "--variant-min-alt", "0"], tmp_path, "ERROR: --variant-min-alt is 1 to 2147483647")
        _refused(command + ["--variant-sites", table, "--variant-min-alt", "2147483648"], tmp_path, "ERROR: --variant-min-alt is 1 to 2147483647")
        _refused(command + ["--variant-sites", table, "--variant-min-percent", "101"], tmp_path, "ERROR: --variant-min-percent is 0 to 100")
        _refused(command + ["--variant-sites", table, "--variant-min-mapq", "256"], tmp_path, "ERROR: --variant-min-mapq is at most 255")
        _refused(command + ["--variant-sites", table, "--variant-min-baseq", "256"], tmp_path, "ERROR: --variant-min-baseq is at most 255")
        _refused(command + ["--variant-sites", table, "--variant-min-baseq", "-1"], tmp_path, "invalid argument to --variant-min-baseq")
        _refused(command + ["--variant-sites", str(tmp_path / "missing" / "variants.tsv")], tmp_path, "parent directory of output file")
        _refused(command + ["--variant-sites", table, "-c", SAM], tmp_path, "-c (separate chimeric alignments) and --variant-sites exclude each other")
        if not ingest:
            _refused(command + ["--variant-sites", table], tmp_path, "--variant-sites needs the device library (agpu_variant_sites)")
    # the driver itself refuses a missing directory before the feed, whoever calls it (the command line checks it once more while it reads its arguments)
    driver = ctypes.CDLL(_harness("libworkflow_on_harness.so"))
    driver.arriba_workflow_last_error.restype = ctypes.c_char_p
    options = _workflow_options(driver)
    assert options.variant_sites_file is None and (options.variant_min_alt, options.variant_min_percent, options.variant_min_mapq, options.variant_min_baseq) == (3, 5, 20, 13)
    options.chimeric_bam_file, options.output_file, options.host_ingest, options.variant_sites_file = SAM.encode(), outputs[0].encode(), 1, str(tmp_path / "missing" / "variants.tsv").encode()
    assert driver.arriba_workflow_run(ctypes.byref(options), None) != 0 and "parent directory of output file" in driver.arriba_workflow_last_error().decode()
    options.variant_sites_file, options.variant_min_percent = None, 6
    assert driver.arriba_workflow_run(ctypes.byref(options), None) != 0 and "need --variant-sites" in driver.arriba_workflow_last_error().decode()
    assert os.listdir(str(tmp_path)) == []
    usage = subprocess.run([WORKFLOW, "-h"], stdout=subprocess.PIPE, universal_newlines=True, timeout=60).stdout
    assert "--variant-sites FILE" in usage and "--variant-min-alt N" in usage and "--variant-min-percent P" in usage and "--variant-min-mapq N" in usage and "--variant-min-baseq N" in usage


def test_a_sample_over_ranks_is_refused_before_the_feed(built, emu_api, tmp_path):
    """one sample over several ranks: refused before a byte of the file is fed (the driver over the harness, a communicator of one rank that does nothing)"""
    from arriba_amd import _capi
    driver = ctypes.CDLL(_harness("libworkflow_on_harness.so"))
    driver.arriba_workflow_open.restype = ctypes.c_void_p
    driver.arriba_workflow_last_error.restype = ctypes.c_char_p
    options = _workflow_options(driver)
    session = ctypes.c_void_p(driver.arriba_workflow_open(ctypes.byref(options)))
    assert session, driver.arriba_workflow_last_error()
    nothing = lambda *arguments: 0  # noqa: E731
    communicator = _capi.WorkflowCommunicator(0, 1, None, _capi.ALL_GATHER(nothing), _capi.ALL_REDUCE_INT64(nothing), _capi.ALL_REDUCE_MAX_BYTES(nothing), None)
    assert driver.arriba_workflow_set_communicator(session, ctypes.byref(communicator)) == 0
    driver.arriba_workflow_variant_sites.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    assert driver.arriba_workflow_variant_sites(session, str(tmp_path / "variants.tsv").encode(), 20, 13, 3, 5) == 0
    status = driver.arriba_workflow_sample(session, SAM.encode(), str(tmp_path / "fusions.tsv").encode(), None, None, None)
    message = driver.arriba_workflow_last_error().decode()
    driver.arriba_workflow_close(session)
    assert status != 0 and "ERROR: " + SEVERAL_GPUS in message
    assert os.listdir(str(tmp_path)) == []


# ---- GPU tier -----------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pipeline(committed_session, cases, tmp_path_factory):
    """one device pipeline on the committed assembly for every case that is ingested here"""
    sample = str(tmp_path_factory.mktemp("committed") / "hand_made.bam")
    lib.write_bgzf(sample, cases("hand_made")[0] + cases("hand_made")[1], 0)
    made = lib.stream_pipeline(committed_session, sample)
    yield made
    made.close()


KNOBS = ("ARRIBA_INGEST_WINDOWS", "ARRIBA_ALLELE_PLAIN_ATOMICS", "ARRIBA_ALLELE_NO_BITMAP", "ARRIBA_VARIANT_LAUNCH_RECORDS", "ARRIBA_VARIANT_MAX_EVENTS")


def _set(knobs, monkeypatch):
    for knob in KNOBS:
        if knob in knobs:
            monkeypatch.setenv(knob, knobs[knob])
        else:
            monkeypatch.delenv(knob, raising=False)


def _ingest(pipeline, cases, name, tmp_path):
    header, record_bytes, _, case = cases(name)
    sample = str(tmp_path / (name + ".bam"))
    lib.write_bgzf(sample, header + record_bytes, 0)
    pipeline.read_chimeric_alignments(sample)
    os.remove(sample)
    return case


def _device_sites(pipeline, cases, name, tmp_path):
    """the case through an ingest and agpu_variant_sites -> (the bytes of the file, the statistics)"""
    case = _ingest(pipeline, cases, name, tmp_path)
    path = str(tmp_path / (name + ".tsv"))
    stats = pipeline.write_variant_sites(path, *_thresholds(case))
    text = open(path, "rb").read()
    assert not os.path.exists(path + ".tmp") and pipeline.variant_sites_allocated_bytes() == 0 and stats["inconsistent"] == 0, name
    os.remove(path)
    return text, stats


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_device_file_is_the_host_file(name, built, pipeline, cases, host_side, tmp_path, monkeypatch):
    """the file of agpu_variant_sites equals the host stepping and the restatement byte for byte and the statistics are equal, on every case of variant_sites_lib"""
    _set({}, monkeypatch)
    text, stats = _device_sites(pipeline, cases, name, tmp_path)
    expected_text, expected = host_side(name)
    print(name, stats)
    assert text == expected_text == cases(name)[2][0]
    assert {key: stats[key] for key in COUNTED} == {key: expected[key] for key in COUNTED} == cases(name)[2][1]
    assert (stats["peak_bytes"] > 0) == (stats["records"] > 0)
    if name == "hand_made":
        assert text == _golden("hand_made.tsv")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", [{"ARRIBA_INGEST_WINDOWS": "1048576,65536"}, {"ARRIBA_ALLELE_PLAIN_ATOMICS": "1"}, {"ARRIBA_ALLELE_NO_BITMAP": "1"}, {"ARRIBA_VARIANT_LAUNCH_RECORDS": "300"}, {"ARRIBA_VARIANT_LAUNCH_RECORDS": "1"}],
                         ids=["ingest_windows", "plain_atomics", "no_bitmap", "launches_of_300", "launches_of_1"])
def test_every_schedule_gives_the_same_file(knobs, built, pipeline, cases, host_side, tmp_path, monkeypatch):
    """the ingest cut into windows, the two knobs of the counters, the event kernel launched in pieces of 300 records (seven launches of the seeded case) and, on the smaller
    cases, of one"""
    _set(knobs, monkeypatch)
    for name in (["counting", "lanes"] if knobs.get("ARRIBA_VARIANT_LAUNCH_RECORDS") == "1" else ["seeded", "counting", "hand_made"]):
        text, stats = _device_sites(pipeline, cases, name, tmp_path)
        assert text == host_side(name)[0], name
        assert {key: stats[key] for key in COUNTED} == cases(name)[2][1], name


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["seeded", "counting", "hand_made", "edges"])
def test_the_rows_are_those_of_allele_counts(name, built, pipeline, cases, host_side, tmp_path, monkeypatch):
    """the reported sites as a sites file through agpu_allele_counts on the same ingest with the same thresholds: its counters and REF equal the row's, column by column"""
    _set({}, monkeypatch)
    case = _ingest(pipeline, cases, name, tmp_path)
    table, sites_path, counts_path = str(tmp_path / "variants.tsv"), str(tmp_path / "reported.sites"), str(tmp_path / "alleles.tsv")
    pipeline.write_variant_sites(table, *_thresholds(case))
    sites, expected = lib.sites_of(open(table, "rb").read())
    assert sites.count(b"\n") == cases(name)[2][1]["reported"] > 0
    open(sites_path, "wb").write(sites)
    pipeline.write_allele_counts(sites_path, counts_path, case["min_mapq"], case["min_baseq"])
    assert open(counts_path, "rb").read() == expected
    assert pipeline.variant_sites_allocated_bytes() == 0 and pipeline.allele_counts_allocated_bytes() == 0


@pytest.mark.gpu
def test_the_event_cap_refuses_and_leaves_the_stream_usable(built, pipeline, cases, host_side, tmp_path, monkeypatch):
    from arriba_amd.pipeline import ArribaError
    _set({"ARRIBA_VARIANT_MAX_EVENTS": "1"}, monkeypatch)
    case = _ingest(pipeline, cases, "seeded", tmp_path)
    path = str(tmp_path / "variants.tsv")
    events = cases("seeded")[2][1]["events"]
    with pytest.raises(ArribaError, match=r"agpu_variant_sites: %d bases differ from the assembly, more than 1 \(ARRIBA_VARIANT_MAX_EVENTS\): the assembly of -a hardly matches the sample" % events):
        pipeline.write_variant_sites(path, *_thresholds(case))
    assert os.listdir(str(tmp_path)) == [] and pipeline.variant_sites_allocated_bytes() == 0
    _set({}, monkeypatch)
    stats = pipeline.write_variant_sites(path, *_thresholds(case))
    assert open(path, "rb").read() == host_side("seeded")[0] and stats["events"] == events > 1


def _command_line(sample, outputs, extra):
    return subprocess.run(["timeout", "-k", "10", "120", WORKFLOW] + _arguments(sample, outputs, extra), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)


@pytest.fixture(scope="module")
def without_the_option(tmp_path_factory):
    """fusions.tsv and discarded.tsv of the committed case from a run of the command line without the option"""
    directory = tmp_path_factory.mktemp("plain")
    outputs = [str(directory / "fusions.tsv"), str(directory / "discarded.tsv")]
    result = _command_line(SAM, outputs, [])
    assert result.returncode == 0, result.stderr[-2000:]
    assert "Finding variant sites" not in result.stdout
    return [open(path, "rb").read() for path in outputs]


@pytest.mark.gpu
@pytest.mark.parametrize("container", ["stored_bgzf", "deflated_bgzf", "sam_text"])
def test_command_line_writes_the_table_next_to_the_fusions(container, built, cases, without_the_option, tmp_path):
    """the committed case as BAM and as SAM text: the committed table, and the other outputs as without the option"""
    os.mkdir(str(tmp_path / "in")); os.mkdir(str(tmp_path / "out"))
    sample = str(tmp_path / "in" / "sample.bam")
    if container == "sam_text":
        sample = SAM
    else:
        lib.write_bgzf(sample, cases("hand_made")[0] + cases("hand_made")[1], 0 if container == "stored_bgzf" else 6)
    outputs = [str(tmp_path / "out" / "fusions.tsv"), str(tmp_path / "out" / "discarded.tsv")]
    result = _command_line(sample, outputs, ["--variant-sites", str(tmp_path / "out" / "variants.tsv")] + HAND_MADE_OPTIONS)
    assert result.returncode == 0, result.stderr[-2000:]
    assert open(str(tmp_path / "out" / "variants.tsv"), "rb").read() == _golden("hand_made.tsv")
    assert HAND_MADE_LINE in result.stdout
    assert [open(path, "rb").read() for path in outputs] == without_the_option
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["discarded.tsv", "fusions.tsv", "variants.tsv"]


@pytest.mark.gpu
def test_session_writes_the_table_of_the_sample_that_asked_for_it(built, without_the_option, tmp_path):
    """three samples in a queue: none, the committed thresholds, then none again: nothing is written for the sample behind the one that asked; no buffer of the option is left on
    either lane"""
    from arriba_amd.pipeline import WorkflowSession
    session = WorkflowSession(FASTA, GTF, interesting_contigs=lib.COMMITTED_CONTIGS, params={"disable_filters": ["blacklist"]})
    for directory in ("first", "second", "third"):
        os.mkdir(str(tmp_path / directory))
    session.submit(SAM)
    session.submit(SAM, variant_sites_file=str(tmp_path / "second" / "variants.tsv"), variant_min_mapq=20, variant_min_baseq=13, variant_min_alt=2, variant_min_percent=50)
    session.sample(SAM, str(tmp_path / "first" / "fusions.tsv"))
    assert session.timing["variant_sites"] == 0
    session.submit(SAM)
    session.sample(SAM, str(tmp_path / "second" / "fusions.tsv"))
    assert session.timing["variant_sites"] > 0
    session.sample(SAM, str(tmp_path / "third" / "fusions.tsv"))
    assert session.timing["variant_sites"] == 0
    from arriba_amd.pipeline import ArribaError
    with pytest.raises(ArribaError, match="need --variant-sites"):  # a threshold without the file, through `sample` as through `submit`
        session.sample(SAM, str(tmp_path / "third" / "refused.tsv"), variant_min_alt=2)
    session.submit(SAM, variant_min_percent=6)
    with pytest.raises(ArribaError, match="need --variant-sites"):
        session.sample(SAM, str(tmp_path / "third" / "refused.tsv"))
    for context in session._lane_contexts():
        count = ctypes.c_uint64(1)
        assert session.api.variant_sites_allocated_bytes(context, ctypes.byref(count)) == 0 and count.value == 0
    session.close()
    assert os.listdir(str(tmp_path / "first")) == ["fusions.tsv"] and sorted(os.listdir(str(tmp_path / "second"))) == ["fusions.tsv", "variants.tsv"] and os.listdir(str(tmp_path / "third")) == ["fusions.tsv"]
    assert open(str(tmp_path / "second" / "variants.tsv"), "rb").read() == _golden("hand_made.tsv")
    for directory in ("first", "second", "third"):
        assert open(str(tmp_path / directory / "fusions.tsv"), "rb").read() == without_the_option[0]


@pytest.mark.gpu
def test_refusals_on_the_device_path(built, cases, tmp_path, monkeypatch):
    """the command line linked with the device library refuses before the feed; agpu_variant_sites is refused with a message before an ingest, with thresholds out of their range, with other references than the ingest had, for a part of a sample, with the stream given back and behind the begin of the next ingest; with
    the option off no kernel of it is in the kernel profile"""
    from arriba_amd import _capi
    from arriba_amd.pipeline import ArribaError, DevicePipeline, HostSession
    outputs, table = [str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv")], str(tmp_path / "variants.tsv")
    command = ["timeout", "-k", "10", "120", WORKFLOW] + _arguments(SAM, outputs, [])
    _refused(command + ["--variant-min-alt", "2"], tmp_path, "need --variant-sites")
    _refused(command + ["--variant-sites", table, "--variant-min-percent", "101"], tmp_path, "ERROR: --variant-min-percent is 0 to 100")
    _refused(command + ["--variant-sites", table, "--variant-min-alt", "0"], tmp_path, "ERROR: --variant-min-alt is 1 to 2147483647")
    _refused(command + ["--variant-sites", table, "-c", SAM], tmp_path, "-c (separate chimeric alignments) and --variant-sites exclude each other")
    _refused(command + ["--variant-sites", str(tmp_path / "missing" / "variants.tsv")], tmp_path, "parent directory of output file")
    api, params = _capi.bind_device_api(_capi.device_library(), "agpu_"), _capi.Params()
    api.default_params(ctypes.byref(params))
    fresh = api.create(0, ctypes.byref(params))
    assert fresh, api.last_error()
    rows, n_rows = ctypes.POINTER(_capi.VariantRow)(), ctypes.c_uint64()
    refused = api.variant_sites(fresh, None, 0, 20, 13, 3, 5, ctypes.byref(rows), ctypes.byref(n_rows), None)  # before an ingest
    message = api.last_error()
    api.destroy(fresh)
    assert refused != 0 and b"agpu_variant_sites: the record stream of the last ingest is not on the device any more" in message
    made = DevicePipeline(HostSession(FASTA, GTF, interesting_contigs=lib.COMMITTED_CONTIGS), bam=SAM)
    made.set_profiling(True)
    host, handle, config = made.session._lib, made.session._session, _capi.IngestConfig()
    # a context without the assembly gets no record stream: the ingest itself is refused there, so the call finds no stream ("agpu_upload_genome must run first" of the guard
    # all consumers share stands behind that and cannot be reached through the entry points)
    bare = api.create(0, ctypes.byref(params))
    assert bare, api.last_error()
    assert host.ahost_bam_open(handle, SAM.encode(), 0, 100, ctypes.byref(config)) == 0
    begun = api.ingest_begin(bare, ctypes.byref(config))
    message = api.last_error()
    host.ahost_bam_close(handle)
    refused = api.variant_sites(bare, None, 0, 20, 13, 3, 5, ctypes.byref(rows), ctypes.byref(n_rows), None)
    after = api.last_error()
    api.destroy(bare)
    assert begun != 0 and b"annotation and genome must be uploaded before the ingest" in message and refused != 0 and b"agpu_variant_sites: the record stream of the last ingest is not on the device any more" in after
    made.read_chimeric_alignments(SAM)
    made.run_workflow(str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv"))
    assert made.kernel_profile() and not [launch for launch in made.kernel_profile() if launch[0].startswith(("variant", "allele"))] and made.variant_sites_allocated_bytes() == 0
    made.read_chimeric_alignments(SAM)
    with pytest.raises(ArribaError, match="need --variant-sites"):
        made.run_workflow(str(tmp_path / "again.tsv"), None, variant_min_baseq=14)
    made.read_chimeric_alignments(SAM)
    made.run_workflow(str(tmp_path / "again.tsv"), None, variant_sites_file=table, variant_min_alt=2, variant_min_percent=50)
    names = set(launch[0] for launch in made.kernel_profile())
    assert {"variant_event_kernel<count>", "variant_event_kernel<fill>", "variant_candidate_kernel", "variant_rows_kernel", "allele_bitmap_kernel", "allele_count_kernel"} <= names
    assert open(table, "rb").read() == _golden("hand_made.tsv") and open(str(tmp_path / "again.tsv")).read() == open(str(tmp_path / "fusions.tsv")).read()
    assert made.variant_sites_allocated_bytes() == 0
    # thresholds and references the call does not admit
    made.read_chimeric_alignments(SAM)
    for thresholds, message in (((256, 13, 3, 5), "a threshold above 255"), ((20, 256, 3, 5), "a threshold above 255"), ((20, 13, 0, 5), "min_alt is 1 to 2\\^31-1"), ((20, 13, 3, 101), "min_percent is 0 to 100")):
        with pytest.raises(ArribaError, match="agpu_variant_sites: " + message):
            made.variant_sites(*thresholds)
    contigs = _capi.DepthContigs()
    assert host.ahost_depth_contigs_of_session(handle, ctypes.byref(contigs)) == 0
    assert made.api.variant_sites(made.ctx, contigs.length, contigs.n_ref + 1, 20, 13, 3, 5, ctypes.byref(rows), ctypes.byref(n_rows), None) != 0 and b"the lengths are not those of the references of the last ingest" in made.api.last_error()
    # a part of a sample (which only a BAM file has)
    os.mkdir(str(tmp_path / "in"))
    lib.write_bgzf(str(tmp_path / "in" / "hand_made.bam"), cases("hand_made")[0] + cases("hand_made")[1], 0)
    made._ingest_records(str(tmp_path / "in" / "hand_made.bam"), False, 100, 64 << 20, part=0, parts=2)
    with pytest.raises(ArribaError, match=SEVERAL_GPUS):
        made.write_variant_sites(str(tmp_path / "part.tsv"))
    # the stream was given back behind the ingest: no ingest kept
    monkeypatch.setenv("ARRIBA_RELEASE_INGEST_BUFFERS", "1")
    made.read_chimeric_alignments(SAM)
    monkeypatch.delenv("ARRIBA_RELEASE_INGEST_BUFFERS")
    with pytest.raises(ArribaError, match="agpu_variant_sites: the record stream of the last ingest is not on the device any more"):
        made.write_variant_sites(str(tmp_path / "gone.tsv"))
    assert made.variant_sites_allocated_bytes() == 0
    # the next read_chimeric_alignments has begun
    made.read_chimeric_alignments(SAM)
    assert host.ahost_bam_open(handle, SAM.encode(), 0, 100, ctypes.byref(config)) == 0
    made._check(made.api.ingest_begin(made.ctx, ctypes.byref(config)))
    with pytest.raises(ArribaError, match="an ingest is under way|not on the device any more"):
        made.write_variant_sites(str(tmp_path / "second.tsv"))
    host.ahost_bam_close(handle)
    made.close()
    assert sorted(os.listdir(str(tmp_path))) == ["again.tsv", "discarded.tsv", "fusions.tsv", "in", "variants.tsv"]
