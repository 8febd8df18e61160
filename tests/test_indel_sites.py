"""--indel-sites: the insertions and deletions the records of -x carry in their CIGARs, left-normalised against -a, with their support and the depth at their anchor (the rule:
DESIGN.md 4.22).

No program of the reference writes this file; the rule is the project's.  tests/golden/indel_sites/hand_made.{sam,tsv} (on hand_made.{fa,gtf} of the same folder) are a case a
reader can check by eye; tests/indel_sites_lib.py restates the rule in plain Python with dicts and strings, test_restatement_equals_the_committed_file holds it to that case, and
only therefore it is the independent side for inputs made at test time.  The CPU tier runs indel_core.hpp and allele_core.hpp stepped on the host (ahost_indel_sites_*); the GPU
tier the kernels of agpu_indels.hip, whose file must equal the host's and the restatement's byte for byte."""
import ctypes
import os
import subprocess

import pytest

import conftest
import indel_sites_lib as lib

GOLDEN = lib.GOLDEN
FASTA, GTF = os.path.join(GOLDEN, "hand_made.fa"), os.path.join(GOLDEN, "hand_made.gtf")
SAM = os.path.join(GOLDEN, "hand_made.sam")
WORKFLOW = os.path.join(conftest.ROOT, "arriba_amd", "lib", "arriba_gpu_workflow")
COUNTED = lib.COUNTED
CASES = ["hand_made"] + list(lib.MADE)
HAND_MADE_STATS = {"records": 42, "contributing": 41, "operations": 28, "events": 25, "unkeyed_insertions": 3, "shift_capped": 0, "runs": 12, "candidates": 11, "sites": 9, "reported": 10}
HAND_MADE_LINE = "Finding indel sites (records=42, contributing=41, operations=28, events=25, unkeyed_insertions=3, shift_capped=0, runs=12, candidates=11, reported=10)"
HAND_MADE_OPTIONS = ["--indel-min-mapq", "20", "--indel-min-alt", "2", "--indel-min-percent", "20"]
SEVERAL_GPUS = "indel sites of one sample over several GPUs are not supported"
KNOBS = ("ARRIBA_INGEST_WINDOWS", "ARRIBA_ALLELE_PLAIN_ATOMICS", "ARRIBA_ALLELE_NO_BITMAP", "ARRIBA_INDEL_LAUNCH_RECORDS", "ARRIBA_INDEL_MAX_EVENTS", "ARRIBA_INDEL_MAX_SHIFT")


def _golden(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


def _thresholds(case):
    return case["min_mapq"], case["min_alt"], case["min_percent"]


def _set(knobs, monkeypatch, case=None):
    """the knobs of the environment, and the cap of the case where it is not the default: the host stepping and the device read it at every call"""
    knobs = dict(knobs)
    if case is not None and case["max_shift"] != 4096:
        knobs["ARRIBA_INDEL_MAX_SHIFT"] = str(case["max_shift"])
    for knob in KNOBS:
        if knob in knobs:
            monkeypatch.setenv(knob, knobs[knob])
        else:
            monkeypatch.delenv(knob, raising=False)


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
    """-> (text, statistics) of ahost_indel_sites_of + ahost_indel_sites_text"""
    from arriba_amd import _capi
    from arriba_amd.pipeline import indel_stats_of
    host, handle = session._lib, session._session
    rows, n_rows, stats, contigs = ctypes.POINTER(_capi.IndelRow)(), ctypes.c_uint64(), _capi.IndelStats(), _capi.DepthContigs()
    assert host.ahost_indel_sites_of(handle, header, len(header), record_bytes, len(record_bytes), *_thresholds(case), ctypes.byref(rows), ctypes.byref(n_rows), ctypes.byref(stats)) == 0, host.ahost_last_error()
    assert host.ahost_depth_contigs_of(header, len(header), ctypes.byref(contigs)) == 0, host.ahost_last_error()
    text, size = ctypes.c_void_p(), ctypes.c_uint64()
    assert host.ahost_indel_sites_text(handle, ctypes.byref(contigs), rows, n_rows.value, ctypes.byref(text), ctypes.byref(size)) == 0, host.ahost_last_error()
    assert n_rows.value == stats.reported
    return ctypes.string_at(text, size.value), indel_stats_of(stats)


@pytest.fixture(scope="module")
def host_side(cases, committed_session):
    """name -> what the host stepping gives: computed once (under the cap of the case), compared against by every test"""
    cache = {}

    def get(name):
        if name not in cache:
            header, record_bytes, _, case = cases(name)
            with pytest.MonkeyPatch.context() as patch:
                _set({}, patch, case)
                cache[name] = _host_sites(committed_session, header, record_bytes, case)
        return cache[name]
    return get


# ---- CPU tier -----------------------------------------------------------------------------------------------------------------------------------------------------

def test_restatement_equals_the_committed_file(assembly):
    """the restatement of the rule against the case that is checked by eye"""
    text, stats = lib.restate(assembly, lib.committed_case())
    assert text == _golden("hand_made.tsv")
    assert stats == HAND_MADE_STATS
    assert len(_golden("hand_made.sam")) < 10000 and len(lib.committed_case()["records"]) == 42
    lines = text.decode().split("\n")
    assert lines[0] + "\n" == lib.HEADER_LINE and "i1\t11\tC\tDEL\t1\tT\t2\t4" in lines and "i1\t30\tG\tINS\t2\tCA\t2\t4" in lines and "chr2\t1\tA\tDEL\t1\tA\t4\t2" in lines and "orphan\t14\tN\tDEL\t1\tN\t2\t2" in lines
    assert not [line for line in lines if line.startswith(("i1\t75\t", "i1\t86\t", "i1\t87\t"))]
    # the assembly of the folder holds what the rule is about
    assert assembly["i1"][10:20] == "CTTTTTTTTG" and assembly["i1"][29:43] == "GCACACACACACAG" and assembly["i1"][45:55] == "CAAAAaaaac" and assembly["i1"][64] == "N" and assembly["2"][:9] == "AAAAAAAAC" and "orphan" not in assembly


def test_the_made_cases_hold_what_they_are_for(cases):
    """the shapes the kernels can go wrong at are in the cases, by what the restatement finds in them"""
    text = {name: cases(name)[2][0].decode() for name in lib.MADE}
    stats = {name: cases(name)[2][1] for name in lib.MADE}
    assert [stats["wave_%d" % n]["records"] for n in (1, 63, 64, 65, 129)] == [1, 63, 64, 65, 129]
    assert stats["wave_1"]["events"] == 4 and cases("wave_1")[3]["records"][0][5] == lib.FOUR_EVENTS
    for n, carriers in ((63, [0, 62]), (64, [0, 63]), (65, [0, 63, 64]), (129, [0, 63, 128])):
        assert [k for k, record in enumerate(cases("wave_%d" % n)[3]["records"]) if "I" in record[5] or "D" in record[5]] == carriers
    assert "\ni1\t85\tT\tINS\t1\tG\t1\t" in text["insertions"] and "\tINS\t27\t" in text["insertions"] and text["insertions"].count("\tINS\t28\t") == 2 and "\tINS\t29\t" not in text["insertions"]
    assert stats["insertions"]["unkeyed_insertions"] == 3 and "\ni1\t104\tA\tINS\t2\tTG\t2\t" in text["insertions"]  # (29 bases, an N, an R; the even and the odd read index give one event)
    normal = text["normalisation"]
    for line in ("i1\t11\tC\tDEL\t1\tT\t2\t", "i1\t11\tC\tINS\t1\tT\t1\t", "chr2\t1\tA\tDEL\t1\tA\t1\t", "i1\t65\tN\tDEL\t1\tG\t1\t", "i1\t46\tC\tDEL\t1\tA\t1\t", "i1\t30\tG\tINS\t2\tCA\t2\t", "i1\t30\tG\tDEL\t2\tCA\t1\t", "i1\t42\tA\tINS\t3\tCAG\t1\t"):
        assert "\n" + line in normal, line
    assert stats["normalisation"]["shift_capped"] == 0 and stats["capped"]["shift_capped"] == 13 and stats["capped"]["runs"] == 16 and "\ni1\t16\tT\tDEL\t1\tT\t1\t" in text["capped"]
    edges = text["edges"]
    assert "\ni1\t117\tC\tDEL\t3\tTGA\t1\t" in edges and "\tDEL\t4\t" not in edges and "\ni1\t120\tA\tINS\t2\tGG\t" in edges and "\ni1\t1\tG\tDEL\t2\tAT\t" in edges and "\ni1\t0\t" not in edges
    assert "\ni1\t25\tC\tDEL\t70\t.\t1\t" in edges and "\norphan\t14\tN\tDEL\t1\tN\t2\t3" in edges and "\norphan\t14\tN\tINS\t2\tAC\t1\t3" in edges and stats["edges"]["operations"] == 15
    assert stats["filters"]["contributing"] == 5 and text["filters"].count("\n") == 4
    assert "\nchr2\t1\tA\tDEL\t1\tA\t4\t2\n" in text["support"] and "\ni1\t105\tT\tINS\t1\tA\t2\t10\n" in text["support"] and "\ni1\t75\t" not in text["support"] and stats["support"]["candidates"] == 5 and stats["support"]["runs"] == 7
    assert stats["seeded"]["records"] == 2000 and stats["seeded"]["events"] > 400 and stats["seeded"]["reported"] >= 4 and stats["seeded"]["candidates"] > stats["seeded"]["reported"] and stats["seeded"]["unkeyed_insertions"] > 0
    for name in ("no_records", "no_events", "no_references"):
        assert text[name] == lib.HEADER_LINE
    assert stats["no_events"]["contributing"] == 40


def test_host_gives_the_committed_bytes(built, cases, host_side, committed_session, tmp_path):
    from arriba_amd import _capi
    text, stats = host_side("hand_made")
    assert text == _golden("hand_made.tsv")
    assert {key: stats[key] for key in COUNTED} == HAND_MADE_STATS
    # ... and through the project's own readers of SAM text and of BAM, which leave no temporary file
    host = committed_session._lib
    sample = str(tmp_path / "hand_made.bam")
    lib.write_bgzf(sample, cases("hand_made")[0] + cases("hand_made")[1], 6)
    for source in (SAM, sample):
        path, found = str(tmp_path / "indels.tsv"), _capi.IndelStats()
        assert host.ahost_indel_sites_file(committed_session._session, source.encode(), path.encode(), 20, 2, 20, ctypes.byref(found)) == 0, host.ahost_last_error()
        assert open(path, "rb").read() == text and found.events == 25 and sorted(os.listdir(str(tmp_path))) == ["hand_made.bam", "indels.tsv"]
        os.remove(path)
    assert host.ahost_indel_sites_file(committed_session._session, sample.encode(), str(tmp_path / "missing" / "indels.tsv").encode(), 20, 2, 20, None) != 0
    assert sorted(os.listdir(str(tmp_path))) == ["hand_made.bam"]
    # the thresholds are part of the result: with min_alt 1 b1 opens i1 86 and the percent test off lets p1 p2 through; with MAPQ 19 admitted m1 counts as well
    assert host.ahost_indel_sites_file(committed_session._session, sample.encode(), str(tmp_path / "open.tsv").encode(), 19, 1, 0, None) == 0
    lines = open(str(tmp_path / "open.tsv")).read().split("\n")
    assert "i1\t86\tG\tDEL\t2\tCA\t2\t5" in lines and "i1\t75\tC\tINS\t1\tA\t2\t11" in lines
    # thresholds the rule does not admit
    rows, n_rows = ctypes.POINTER(_capi.IndelRow)(), ctypes.c_uint64()
    for thresholds, message in (((256, 3, 5), "a threshold above 255"), ((20, 0, 5), "min_alt is 1 to 2^31-1"), ((20, 2 ** 31, 5), "min_alt is 1 to 2^31-1"), ((20, 3, 101), "min_percent is 0 to 100")):
        assert host.ahost_indel_sites_of(committed_session._session, cases("hand_made")[0], len(cases("hand_made")[0]), None, 0, *thresholds, ctypes.byref(rows), ctypes.byref(n_rows), None) != 0
        assert message in host.ahost_last_error().decode()


@pytest.mark.parametrize("name", list(lib.MADE))
def test_host_equals_the_restatement(name, built, cases, host_side):
    text, stats = host_side(name)
    expected_text, expected = cases(name)[2]
    assert text == expected_text
    assert {key: stats[key] for key in COUNTED} == expected


def _harness(target):
    directory = os.path.join(conftest.ROOT, "tests", "emu")
    subprocess.run(["make", "-s", "-C", directory, target], check=True)
    return os.path.join(directory, target)


def _arguments(sample, outputs, extra):
    return ["-x", sample, "-g", GTF, "-a", FASTA, "-i", lib.COMMITTED_CONTIGS, "-o", outputs[0], "-O", outputs[1], "-f", "blacklist"] + extra


def test_host_ingest_through_the_command_line(built, emu_api, tmp_path):
    """--host-ingest --indel-sites: the C++ driver (over the host stepping harness, where there is no GPU) writes the committed table, and fusions.tsv and discarded.tsv are those
    of a run without the option"""
    files = {}
    for option in ([], ["--indel-sites", str(tmp_path / "indels.tsv")] + HAND_MADE_OPTIONS):
        outputs = [str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv")]
        result = subprocess.run([_harness("workflow_on_harness")] + _arguments(SAM, outputs, ["--host-ingest"] + option), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
        assert result.returncode == 0, result.stderr[-2000:]
        assert (HAND_MADE_LINE in result.stdout) == bool(option) and ("Finding indel sites" in result.stdout) == bool(option)
        files[bool(option)] = [open(path, "rb").read() for path in outputs]
    assert open(str(tmp_path / "indels.tsv"), "rb").read() == _golden("hand_made.tsv")
    assert files[True] == files[False] and sorted(os.listdir(str(tmp_path))) == ["discarded.tsv", "fusions.tsv", "indels.tsv"]


def _refused(command, tmp_path, message):
    result = subprocess.run(command, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert result.returncode != 0 and message in result.stderr, (message, result.stderr[-2000:])
    assert not [name for name in os.listdir(str(tmp_path)) if name.startswith(("indels", "fusions", "discarded"))], os.listdir(str(tmp_path))


def _workflow_options(driver):
    from arriba_amd import _capi
    options = _capi.WorkflowOptions()
    driver.arriba_workflow_default_options(ctypes.byref(options))
    options.assembly_file, options.gene_annotation_file, options.interesting_contigs = FASTA.encode(), GTF.encode(), lib.COMMITTED_CONTIGS.encode()
    return options


def test_refusals_before_the_input_is_read(built, emu_api, tmp_path):
    """a threshold without the file, thresholds out of their range, a path in a missing directory, -c: refused with --host-ingest as without it, before the feed, and nothing is
    written.  The test-only build of the C++ driver against the host stepping harness has no twin of the kernels of agpu_indels.hip: without --host-ingest it says so, also before
    the feed.  The defaults and the usage text"""
    outputs, table = [str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv")], str(tmp_path / "indels.tsv")
    for ingest in (["--host-ingest"], []):
        command = [_harness("workflow_on_harness")] + _arguments(SAM, outputs, ingest)
        for threshold in ("--indel-min-alt", "--indel-min-percent", "--indel-min-mapq"):
            _refused(command + [threshold, "7"], tmp_path, "need --indel-sites")
        _refused(command + ["--indel-sites", table, "--indel-min-alt", "0"], tmp_path, "ERROR: --indel-min-alt is 1 to 2147483647")
        _refused(command + ["--indel-sites", table, "--indel-min-alt", "2147483648"], tmp_path, "ERROR: --indel-min-alt is 1 to 2147483647")
        _refused(command + ["--indel-sites", table, "--indel-min-percent", "101"], tmp_path, "ERROR: --indel-min-percent is 0 to 100")
        _refused(command + ["--indel-sites", table, "--indel-min-mapq", "256"], tmp_path, "ERROR: --indel-min-mapq is at most 255")
        _refused(command + ["--indel-sites", table, "--indel-min-mapq", "-1"], tmp_path, "invalid argument to --indel-min-mapq")
        _refused(command + ["--indel-sites", str(tmp_path / "missing" / "indels.tsv")], tmp_path, "parent directory of output file")
        _refused(command + ["--indel-sites", table, "-c", SAM], tmp_path, "-c (separate chimeric alignments) and --indel-sites exclude each other")
        if not ingest:
            _refused(command + ["--indel-sites", table], tmp_path, "--indel-sites needs the device library (agpu_indel_sites)")
    # the driver itself refuses a missing directory before the feed, whoever calls it (the command line checks it once more while it reads its arguments)
    driver = ctypes.CDLL(_harness("libworkflow_on_harness.so"))
    driver.arriba_workflow_last_error.restype = ctypes.c_char_p
    options = _workflow_options(driver)
    assert options.indel_sites_file is None and (options.indel_min_alt, options.indel_min_percent, options.indel_min_mapq) == (3, 5, 20)
    options.chimeric_bam_file, options.output_file, options.host_ingest, options.indel_sites_file = SAM.encode(), outputs[0].encode(), 1, str(tmp_path / "missing" / "indels.tsv").encode()
    assert driver.arriba_workflow_run(ctypes.byref(options), None) != 0 and "parent directory of output file" in driver.arriba_workflow_last_error().decode()
    options.indel_sites_file, options.indel_min_percent = None, 6
    assert driver.arriba_workflow_run(ctypes.byref(options), None) != 0 and "need --indel-sites" in driver.arriba_workflow_last_error().decode()
    assert os.listdir(str(tmp_path)) == []
    usage = subprocess.run([WORKFLOW, "-h"], stdout=subprocess.PIPE, universal_newlines=True, timeout=60).stdout
    assert "--indel-sites FILE" in usage and "--indel-min-alt N" in usage and "--indel-min-percent P" in usage and "--indel-min-mapq N" in usage


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
    driver.arriba_workflow_indel_sites.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    assert driver.arriba_workflow_indel_sites(session, str(tmp_path / "indels.tsv").encode(), 20, 3, 5) == 0
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


def _ingest(pipeline, cases, name, tmp_path):
    header, record_bytes, _, case = cases(name)
    sample = str(tmp_path / (name + ".bam"))
    lib.write_bgzf(sample, header + record_bytes, 0)
    pipeline.read_chimeric_alignments(sample)
    os.remove(sample)
    return case


def _device_sites(pipeline, cases, name, tmp_path):
    """the case through an ingest and agpu_indel_sites -> (the bytes of the file, the statistics)"""
    case = _ingest(pipeline, cases, name, tmp_path)
    path = str(tmp_path / (name + ".tsv"))
    stats = pipeline.write_indel_sites(path, *_thresholds(case))
    text = open(path, "rb").read()
    assert not os.path.exists(path + ".tmp") and pipeline.indel_sites_allocated_bytes() == 0, name
    os.remove(path)
    return text, stats


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_device_file_is_the_host_file(name, built, pipeline, cases, host_side, tmp_path, monkeypatch):
    """the file of agpu_indel_sites equals the host stepping and the restatement byte for byte and the statistics are equal, on every case of indel_sites_lib: the wavefront edges,
    the insertions, the normalisation (also under a cap of two steps), the edges, the filter, support > depth, the seeded case"""
    expected_text, expected = host_side(name)
    _set({}, monkeypatch, cases(name)[3])
    text, stats = _device_sites(pipeline, cases, name, tmp_path)
    print(name, stats)
    assert text == expected_text == cases(name)[2][0]
    assert {key: stats[key] for key in COUNTED} == {key: expected[key] for key in COUNTED} == cases(name)[2][1]
    assert (stats["peak_bytes"] > 0) == (stats["records"] > 0)
    if name == "hand_made":
        assert text == _golden("hand_made.tsv")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", [{"ARRIBA_INGEST_WINDOWS": "1048576,65536"}, {"ARRIBA_ALLELE_PLAIN_ATOMICS": "1"}, {"ARRIBA_ALLELE_NO_BITMAP": "1"}, {"ARRIBA_INDEL_LAUNCH_RECORDS": "300"}, {"ARRIBA_INDEL_LAUNCH_RECORDS": "64"},
                                   {"ARRIBA_INDEL_LAUNCH_RECORDS": "1"}], ids=["ingest_windows", "plain_atomics", "no_bitmap", "launches_of_300", "launches_of_64", "launches_of_1"])
def test_every_schedule_gives_the_same_file(knobs, built, pipeline, cases, host_side, tmp_path, monkeypatch):
    """the ingest cut into windows, the two knobs of the counters, the event kernel launched in pieces of 300 records (seven launches of the seeded case), of 64 (a wavefront a
    launch) and, on the smaller cases, of one"""
    expected = {name: host_side(name)[0] for name in ("seeded", "support", "hand_made", "wave_129")}
    _set(knobs, monkeypatch)
    for name in (["support", "wave_129"] if knobs.get("ARRIBA_INDEL_LAUNCH_RECORDS") == "1" else ["seeded", "support", "hand_made", "wave_129"]):
        text, stats = _device_sites(pipeline, cases, name, tmp_path)
        assert text == expected[name], name
        assert {key: stats[key] for key in COUNTED} == cases(name)[2][1], name


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["seeded", "support", "hand_made", "edges"])
def test_depth_is_the_sum_of_allele_counts(name, built, pipeline, cases, tmp_path, monkeypatch):
    """the anchors of the reported events as a sites file through agpu_allele_counts on the same ingest with the same MAPQ and min_baseq 0: DEPTH equals A + C + G + T + N + DEL
    there, and REF its REF"""
    _set({}, monkeypatch)
    case = _ingest(pipeline, cases, name, tmp_path)
    table, sites_path, counts_path = str(tmp_path / "indels.tsv"), str(tmp_path / "anchors.sites"), str(tmp_path / "alleles.tsv")
    pipeline.write_indel_sites(table, *_thresholds(case))
    rows = [line.split("\t") for line in open(table).read().split("\n")[1:-1]]
    assert len(rows) == cases(name)[2][1]["reported"] > 0
    open(sites_path, "w").write("".join("%s\t%s\n" % (row[0], row[1]) for row in rows))
    pipeline.write_allele_counts(sites_path, counts_path, case["min_mapq"], 0)
    counted = [line.split("\t") for line in open(counts_path).read().split("\n")[1:-1]]
    assert len(counted) == len(rows)
    for row, other in zip(rows, counted):
        assert other[:3] == row[:3] and sum(int(number) for number in other[3:9]) == int(row[7]), (row, other)
    assert pipeline.indel_sites_allocated_bytes() == 0 and pipeline.allele_counts_allocated_bytes() == 0


@pytest.mark.gpu
def test_the_event_cap_refuses_and_leaves_the_stream_usable(built, pipeline, cases, host_side, tmp_path, monkeypatch):
    from arriba_amd.pipeline import ArribaError
    expected = host_side("seeded")[0]
    _set({"ARRIBA_INDEL_MAX_EVENTS": "1"}, monkeypatch)
    case = _ingest(pipeline, cases, "seeded", tmp_path)
    path = str(tmp_path / "indels.tsv")
    events = cases("seeded")[2][1]["events"]
    with pytest.raises(ArribaError, match=r"agpu_indel_sites: %d insertions and deletions, more than 1 \(ARRIBA_INDEL_MAX_EVENTS\)" % events):
        pipeline.write_indel_sites(path, *_thresholds(case))
    assert os.listdir(str(tmp_path)) == [] and pipeline.indel_sites_allocated_bytes() == 0
    _set({}, monkeypatch)
    stats = pipeline.write_indel_sites(path, *_thresholds(case))
    assert open(path, "rb").read() == expected and stats["events"] == events > 1


def _command_line(sample, outputs, extra):
    return subprocess.run(["timeout", "-k", "10", "120", WORKFLOW] + _arguments(sample, outputs, extra), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)


@pytest.fixture(scope="module")
def without_the_option(tmp_path_factory):
    """fusions.tsv and discarded.tsv of the committed case from a run of the command line without the option"""
    directory = tmp_path_factory.mktemp("plain")
    outputs = [str(directory / "fusions.tsv"), str(directory / "discarded.tsv")]
    result = _command_line(SAM, outputs, [])
    assert result.returncode == 0, result.stderr[-2000:]
    assert "Finding indel sites" not in result.stdout
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
    result = _command_line(sample, outputs, ["--indel-sites", str(tmp_path / "out" / "indels.tsv")] + HAND_MADE_OPTIONS)
    assert result.returncode == 0, result.stderr[-2000:]
    assert open(str(tmp_path / "out" / "indels.tsv"), "rb").read() == _golden("hand_made.tsv")
    assert HAND_MADE_LINE in result.stdout
    assert [open(path, "rb").read() for path in outputs] == without_the_option
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["discarded.tsv", "fusions.tsv", "indels.tsv"]


@pytest.mark.gpu
def test_session_writes_the_table_of_the_sample_that_asked_for_it(built, without_the_option, tmp_path):
    """three samples in a queue: none, the committed thresholds, then none again: nothing is written for the sample behind the one that asked; no buffer of the option is left on
    either lane"""
    from arriba_amd.pipeline import ArribaError, WorkflowSession
    session = WorkflowSession(FASTA, GTF, interesting_contigs=lib.COMMITTED_CONTIGS, params={"disable_filters": ["blacklist"]})
    for directory in ("first", "second", "third"):
        os.mkdir(str(tmp_path / directory))
    session.submit(SAM)
    session.submit(SAM, indel_sites_file=str(tmp_path / "second" / "indels.tsv"), indel_min_mapq=20, indel_min_alt=2, indel_min_percent=20)
    session.sample(SAM, str(tmp_path / "first" / "fusions.tsv"))
    assert session.timing["indel_sites"] == 0
    session.submit(SAM)
    session.sample(SAM, str(tmp_path / "second" / "fusions.tsv"))
    assert session.timing["indel_sites"] > 0
    session.sample(SAM, str(tmp_path / "third" / "fusions.tsv"))
    assert session.timing["indel_sites"] == 0
    with pytest.raises(ArribaError, match="need --indel-sites"):  # a threshold without the file, through `sample` as through `submit`
        session.sample(SAM, str(tmp_path / "third" / "refused.tsv"), indel_min_alt=2)
    session.submit(SAM, indel_min_percent=6)
    with pytest.raises(ArribaError, match="need --indel-sites"):
        session.sample(SAM, str(tmp_path / "third" / "refused.tsv"))
    for context in session._lane_contexts():
        count = ctypes.c_uint64(1)
        assert session.api.indel_sites_allocated_bytes(context, ctypes.byref(count)) == 0 and count.value == 0
    session.close()
    assert os.listdir(str(tmp_path / "first")) == ["fusions.tsv"] and sorted(os.listdir(str(tmp_path / "second"))) == ["fusions.tsv", "indels.tsv"] and os.listdir(str(tmp_path / "third")) == ["fusions.tsv"]
    assert open(str(tmp_path / "second" / "indels.tsv"), "rb").read() == _golden("hand_made.tsv")
    for directory in ("first", "second", "third"):
        assert open(str(tmp_path / directory / "fusions.tsv"), "rb").read() == without_the_option[0]


@pytest.mark.gpu
def test_refusals_on_the_device_path(built, cases, tmp_path, monkeypatch):
    """the command line linked with the device library refuses before the feed; agpu_indel_sites is refused with a message before an ingest (no resident stream), with a null
    argument, with thresholds out of their range, with other references than the ingest had, for a part of a sample (a read-sharded context) and with the stream given back; with
    the option off no kernel of it is in the kernel profile"""
    from arriba_amd import _capi
    from arriba_amd.pipeline import ArribaError, DevicePipeline, HostSession
    _set({}, monkeypatch)
    outputs, table = [str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv")], str(tmp_path / "indels.tsv")
    command = ["timeout", "-k", "10", "120", WORKFLOW] + _arguments(SAM, outputs, [])
    _refused(command + ["--indel-min-alt", "2"], tmp_path, "need --indel-sites")
    _refused(command + ["--indel-sites", table, "--indel-min-percent", "101"], tmp_path, "ERROR: --indel-min-percent is 0 to 100")
    _refused(command + ["--indel-sites", table, "--indel-min-alt", "0"], tmp_path, "ERROR: --indel-min-alt is 1 to 2147483647")
    _refused(command + ["--indel-sites", table, "-c", SAM], tmp_path, "-c (separate chimeric alignments) and --indel-sites exclude each other")
    _refused(command + ["--indel-sites", str(tmp_path / "missing" / "indels.tsv")], tmp_path, "parent directory of output file")
    api, params = _capi.bind_device_api(_capi.device_library(), "agpu_"), _capi.Params()
    api.default_params(ctypes.byref(params))
    fresh = api.create(0, ctypes.byref(params))
    assert fresh, api.last_error()
    rows, n_rows = ctypes.POINTER(_capi.IndelRow)(), ctypes.c_uint64()
    refused = api.indel_sites(fresh, None, 0, 20, 3, 5, ctypes.byref(rows), ctypes.byref(n_rows), None)  # before an ingest
    message = api.last_error()
    null_rows = api.indel_sites(fresh, None, 0, 20, 3, 5, None, ctypes.byref(n_rows), None)
    null_message = api.last_error()
    null_count = api.indel_sites(fresh, None, 0, 20, 3, 5, ctypes.byref(rows), None, None)
    null_lengths = api.indel_sites(fresh, None, 3, 20, 3, 5, ctypes.byref(rows), ctypes.byref(n_rows), None)
    api.destroy(fresh)
    assert refused != 0 and b"agpu_indel_sites: the record stream of the last ingest is not on the device any more" in message
    assert null_rows != 0 and null_count != 0 and null_lengths != 0 and b"null argument" in null_message
    made = DevicePipeline(HostSession(FASTA, GTF, interesting_contigs=lib.COMMITTED_CONTIGS), bam=SAM)
    made.set_profiling(True)
    host, handle = made.session._lib, made.session._session
    made.run_workflow(str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv"))
    assert made.kernel_profile() and not [launch for launch in made.kernel_profile() if launch[0].startswith(("indel", "allele"))] and made.indel_sites_allocated_bytes() == 0
    made.read_chimeric_alignments(SAM)
    with pytest.raises(ArribaError, match="need --indel-sites"):
        made.run_workflow(str(tmp_path / "again.tsv"), None, indel_min_mapq=21)
    made.read_chimeric_alignments(SAM)
    made.run_workflow(str(tmp_path / "again.tsv"), None, indel_sites_file=table, indel_min_alt=2, indel_min_percent=20)
    names = set(launch[0] for launch in made.kernel_profile())
    assert {"indel_event_kernel<count>", "indel_event_kernel<fill>", "indel_candidate_kernel", "indel_rows_kernel", "allele_bitmap_kernel", "allele_count_kernel"} <= names
    assert open(table, "rb").read() == _golden("hand_made.tsv") and open(str(tmp_path / "again.tsv")).read() == open(str(tmp_path / "fusions.tsv")).read()
    assert made.indel_sites_allocated_bytes() == 0
    # thresholds and references the call does not admit
    made.read_chimeric_alignments(SAM)
    for thresholds, message in (((256, 3, 5), "a threshold above 255"), ((20, 0, 5), "min_alt is 1 to 2\\^31-1"), ((20, 2 ** 31, 5), "min_alt is 1 to 2\\^31-1"), ((20, 3, 101), "min_percent is 0 to 100")):
        with pytest.raises(ArribaError, match="agpu_indel_sites: " + message):
            made.indel_sites(*thresholds)
    contigs = _capi.DepthContigs()
    assert host.ahost_depth_contigs_of_session(handle, ctypes.byref(contigs)) == 0
    assert made.api.indel_sites(made.ctx, contigs.length, contigs.n_ref + 1, 20, 3, 5, ctypes.byref(rows), ctypes.byref(n_rows), None) != 0 and b"the lengths are not those of the references of the last ingest" in made.api.last_error()
    # a part of a sample (which only a BAM file has)
    os.mkdir(str(tmp_path / "in"))
    lib.write_bgzf(str(tmp_path / "in" / "hand_made.bam"), cases("hand_made")[0] + cases("hand_made")[1], 0)
    made._ingest_records(str(tmp_path / "in" / "hand_made.bam"), False, 100, 64 << 20, part=0, parts=2)
    with pytest.raises(ArribaError, match=SEVERAL_GPUS):
        made.write_indel_sites(str(tmp_path / "part.tsv"))
    # the stream was given back behind the ingest: no ingest kept
    monkeypatch.setenv("ARRIBA_RELEASE_INGEST_BUFFERS", "1")
    made.read_chimeric_alignments(SAM)
    monkeypatch.delenv("ARRIBA_RELEASE_INGEST_BUFFERS")
    with pytest.raises(ArribaError, match="agpu_indel_sites: the record stream of the last ingest is not on the device any more"):
        made.write_indel_sites(str(tmp_path / "gone.tsv"))
    assert made.indel_sites_allocated_bytes() == 0
    made.close()
    assert sorted(os.listdir(str(tmp_path))) == ["again.tsv", "discarded.tsv", "fusions.tsv", "in", "indels.tsv"]
