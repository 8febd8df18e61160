"""--allele-counts: the bases the records of -x show at a list of known positions (the rule: DESIGN.md 4.17).

No program of the reference writes this file; the rule is the project's.  tests/golden/allele_counts/hand_made.{fa,gtf,sam,sites,tsv} are a case a reader can check by eye, one
record per clause of the rule; tests/allele_counts_lib.py restates the rule in plain Python with dicts, test_restatement_equals_the_committed_file holds it to that case, and only
therefore it is the independent side for inputs made at test time.  The CPU tier runs arriba_amd/csrc/device/allele_core.hpp stepped on the host (ahost_allele_*); the GPU tier the
kernels of agpu_alleles.hip, whose file must equal the host's byte for byte and whose statistics must equal the host's."""
import ctypes
import os
import subprocess

import pytest

import conftest
import allele_counts_lib as lib

GOLDEN = lib.GOLDEN
WORKFLOW = os.path.join(conftest.ROOT, "arriba_amd", "lib", "arriba_gpu_workflow")
SEEDED = ["seed%d" % (1700 + k) for k in range(50)]
COUNTED = lib.COUNTED  # what the device, the host and the restatement must agree on
MADE = {"hot": lib.hot_case, "wavefront": lib.wavefront_case, "dense": lib.dense_case, "long_cigar": lib.long_cigar_case, "sparse": lib.sparse_case, "no_records": lib.no_records_case,
        "no_sites": lib.no_sites_case, "header_only": lib.header_only_case}
HAND_MADE_STATS = {"records": 20, "contributing": 13, "hits": 29, "sites": 27, "placed": 25, "covered": 23}
HAND_MADE_LINE = "Counting alleles at known sites (records=20, contributing=13, hits=29, sites=27, placed=25, covered=23)"
HAND_MADE_OPTIONS = ["--allele-min-mapq", str(lib.COMMITTED_THRESHOLDS[0]), "--allele-min-baseq", str(lib.COMMITTED_THRESHOLDS[1])]
SITES = os.path.join(GOLDEN, "hand_made.sites")


def _golden(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


def _invariant(text, stats, case):
    """`hits` is the sum of the eight columns, the file has a header line and `sites` lines of eleven fields in the order of the sites file, `covered` counts the lines with a
    non-zero column, an unplaced line has REF '.' and no count"""
    assert text.startswith(lib.HEADER_LINE.encode()) and text.endswith(b"\n")
    rows = [line.split(b"\t") for line in text.split(b"\n")[1:-1]]
    assert len(rows) == stats["sites"] and all(len(row) == 11 for row in rows)
    assert sum(int(field) for row in rows for field in row[3:]) == stats["hits"]
    assert sum(1 for row in rows if any(int(field) for field in row[3:])) == stats["covered"] <= stats["placed"] <= stats["sites"]
    assert sum(1 for row in rows if row[2] != b".") == stats["placed"] and all(not any(int(field) for field in row[3:]) for row in rows if row[2] == b".")
    assert [(row[0].decode("latin-1"), int(row[1])) for row in rows] == lib.parse_sites(case["sites"])
    assert stats["contributing"] <= stats["records"] == len(case["records"])
    return rows


@pytest.fixture(scope="module")
def assembly():
    return lib.load_assembly()


@pytest.fixture(scope="module")
def cases(assembly, tmp_path_factory):
    """name -> (BAM header, record bytes, (text, stats) of the restatement, the case, the path of its sites file): made once"""
    cache, directory = {}, tmp_path_factory.mktemp("sites")

    def get(name):
        if name not in cache:
            case = lib.committed_case() if name == "hand_made" else lib.random_case(int(name[4:])) if name.startswith("seed") else MADE[name]()
            path = str(directory / (name + ".sites"))
            open(path, "wb").write(case["sites"])
            cache[name] = (lib.bam_header(case["references"]), lib.bam_records(case), lib.restate(assembly, case), case, path)
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
    return _capi.AlleleStats()


def _host_counts(session, header, record_bytes, case, sites_path):
    """-> (text, statistics) of ahost_allele_sites_load + ahost_allele_counts_of + ahost_allele_counts_text"""
    from arriba_amd import _capi
    from arriba_amd.pipeline import allele_stats_of
    host, handle = session._lib, session._session
    sites, rows, stats = _capi.AlleleSites(), ctypes.POINTER(_capi.AlleleRow)(), _stats()
    assert host.ahost_allele_sites_load(sites_path.encode(), header, len(header), ctypes.byref(sites)) == 0, host.ahost_last_error()
    try:
        assert host.ahost_allele_counts_of(handle, header, len(header), record_bytes, len(record_bytes), ctypes.byref(sites), case["min_mapq"], case["min_baseq"], ctypes.byref(rows), ctypes.byref(stats)) == 0, host.ahost_last_error()
        text, size = ctypes.c_void_p(), ctypes.c_uint64()
        assert host.ahost_allele_counts_text(ctypes.byref(sites), rows, sites.n_sites, ctypes.byref(text), ctypes.byref(size)) == 0, host.ahost_last_error()
        assert sites.placed == stats.placed and sites.n_sites == stats.sites
        return ctypes.string_at(text, size.value), allele_stats_of(stats)
    finally:
        host.ahost_allele_sites_free(ctypes.byref(sites))


@pytest.fixture(scope="module")
def host_side(cases, committed_session):
    """name -> what the host stepping gives: computed once, compared against by every test"""
    cache = {}

    def get(name):
        if name not in cache:
            header, record_bytes, _, case, path = cases(name)
            cache[name] = _host_counts(committed_session, header, record_bytes, case, path)
        return cache[name]
    return get


# ---- CPU tier -----------------------------------------------------------------------------------------------------------------------------------------------------

def test_restatement_equals_the_committed_file(assembly):
    """the restatement of the rule against the case that is checked by eye"""
    case = lib.committed_case()
    text, stats = lib.restate(assembly, case)
    assert text == _golden("hand_made.tsv")
    assert stats == HAND_MADE_STATS
    assert case["references"] == lib.HEADER and set(assembly) == {"a1", "2"} and len(assembly["a1"]) == 100 and assembly["a1"][20:30].islower() and assembly["a1"][54] == "N"
    assert all(len(_golden("hand_made." + kind)) < 100000 for kind in ("fa", "gtf", "sam", "sites", "tsv"))
    rows = _invariant(text, stats, case)
    assert all(any(int(row[3 + column]) for row in rows) for column in range(8)), "every column is used"
    assert set(row[2] for row in rows) == {b"A", b"C", b"G", b"T", b"N", b"."}


def test_host_gives_the_committed_bytes(built, cases, host_side, committed_session, tmp_path):
    text, stats = host_side("hand_made")
    assert text == _golden("hand_made.tsv")
    assert {key: stats[key] for key in COUNTED} == HAND_MADE_STATS == cases("hand_made")[2][1]
    # ... and through the project's own readers of SAM text and of BAM, which leave no temporary file
    host = committed_session._lib
    sample = str(tmp_path / "hand_made.bam")
    lib.write_bgzf(sample, cases("hand_made")[0] + cases("hand_made")[1], 6)
    for source in (os.path.join(GOLDEN, "hand_made.sam"), sample):
        path, counted = str(tmp_path / "alleles.tsv"), _stats()
        assert host.ahost_allele_counts_file(committed_session._session, source.encode(), SITES.encode(), path.encode(), 20, 13, ctypes.byref(counted)) == 0, host.ahost_last_error()
        assert open(path, "rb").read() == text and counted.hits == 29 and sorted(os.listdir(str(tmp_path))) == ["alleles.tsv", "hand_made.bam"]
        os.remove(path)
    assert host.ahost_allele_counts_file(committed_session._session, sample.encode(), SITES.encode(), str(tmp_path / "missing" / "alleles.tsv").encode(), 20, 13, None) != 0
    assert sorted(os.listdir(str(tmp_path))) == ["hand_made.bam"]
    # the thresholds are part of the result: without them m2 counts (G at a1 51) and nothing is LOWQ
    assert host.ahost_allele_counts_file(committed_session._session, sample.encode(), SITES.encode(), str(tmp_path / "open.tsv").encode(), 0, 0, None) == 0
    lines = open(str(tmp_path / "open.tsv"), "rb").read().split(b"\n")
    assert b"a1\t51\tA\t0\t1\t1\t1\t0\t0\t0\t0" in lines and b"a1\t42\tT\t0\t1\t0\t1\t0\t0\t0\t0" in lines


@pytest.mark.parametrize("name", ["seeded", "hot", "wavefront", "dense", "long_cigar", "sparse", "no_records", "no_sites", "header_only"])
def test_host_equals_the_restatement(name, built, cases, host_side):
    """file and statistics, and the invariants: `hits` is the sum of the columns, the lines are those of the sites file in its order"""
    used, seen = [0] * 8, {"ref": set(), "unplaced": 0, "duplicates": 0}
    for case_name in (SEEDED if name == "seeded" else [name]):
        text, stats = host_side(case_name)
        expected_text, expected = cases(case_name)[2]
        assert expected["records"] <= (300 if name == "seeded" else 1 << 17)
        assert text == expected_text, case_name
        assert {key: stats[key] for key in COUNTED} == expected, case_name
        rows = _invariant(text, stats, cases(case_name)[3])
        for row in rows:
            used = [total + int(field) for total, field in zip(used, row[3:])]
            seen["ref"].add(row[2]); seen["unplaced"] += row[2] == b"."
        seen["duplicates"] += len(rows) - len(set((row[0], row[1]) for row in rows))
    if name == "seeded":  # the seeded set as a whole exercises the rule
        assert all(total > 100 for total in used), used
        assert seen["ref"] >= {b"A", b"C", b"G", b"T", b"N", b"."} and seen["unplaced"] > 100 and seen["duplicates"] > 100
        assert set(cases(case_name)[3]["min_mapq"] for case_name in SEEDED) == {0, 20, 255} and set(cases(case_name)[3]["min_baseq"] for case_name in SEEDED) == {0, 13, 30, 255}
    if name == "hot":
        assert stats["records"] == 70129 and stats["contributing"] == 70129
        first = text.split(b"\n")[1].split(b"\t")
        assert text.split(b"\n")[5].split(b"\t")[1:] == first[1:] and first[:3] == [b"a1", b"50", b"A"]
        assert sum(int(field) for field in first[3:]) == 70001 and int(first[8]) == 5385 and sum(int(field) for field in first[3:7]) > 1 << 15
        assert text.split(b"\n")[2] == b"a1\t60\tA\t0\t0\t64\t0\t0\t0\t0\t0"
    if name == "wavefront":
        assert text.split(b"\n")[1].split(b"\t")[3:] == [b"22", b"22", b"21", b"0", b"0", b"0", b"0", b"0"]
    if name == "dense":
        assert stats["sites"] == 151 and stats["covered"] == 151 and stats["hits"] == 151 + 20 and used[7] > 10 and used[4] > 10
    if name == "long_cigar":
        assert [line.split(b"\t", 3)[3] for line in text.split(b"\n")[1:-1]] == [b"1\t0\t0\t0\t0\t0\t0\t0", b"0\t0\t0\t0\t0\t0\t1\t0", b"0\t0\t1\t0\t0\t0\t0\t0", b"0\t0\t0\t0\t0\t1\t0\t0",
                                                                                 b"1\t0\t0\t0\t0\t0\t0\t0", b"0\t0\t0\t0\t0\t1\t0\t0", b"0\t0\t0\t0\t0\t0\t0\t0"]
    if name == "sparse":
        assert stats["contributing"] == 400 and stats["sites"] == 1000 and stats["placed"] == 900 and stats["hits"] == 0 and stats["covered"] == 0
    if name == "no_records":
        assert text == (lib.HEADER_LINE + "a1\t5\tA\t0\t0\t0\t0\t0\t0\t0\t0\nchr2\t5\tC\t0\t0\t0\t0\t0\t0\t0\t0\nnowhere\t5\t.\t0\t0\t0\t0\t0\t0\t0\t0\n").encode()
    if name == "no_sites":
        assert text == lib.HEADER_LINE.encode() and stats["contributing"] == 5 and stats["sites"] == 0
    if name == "header_only":
        assert text == (lib.HEADER_LINE + "a1\t5\t.\t0\t0\t0\t0\t0\t0\t0\t0\nchr2\t7\t.\t0\t0\t0\t0\t0\t0\t0\t0\n").encode() and stats["placed"] == 0


REFUSED = [(b"a1\t5\nchr2\n", 2, "fewer than two fields"), (b"#c\n\na1\t\n", 3, "the position is empty"), (b"a1\t5\na1\t\tx\n", 2, "the position is empty"), (b"a1\t12x\n", 1, "not a digit"),
           (b"a1\t5\n\n\na1\t-3\n", 4, "not a digit"), (b"a1\t 7\n", 1, "not a digit"), (b"a1\t0\n", 1, "0 or above 2^31-1"), (b"a1\t1\na1\t2147483648\n", 2, "0 or above 2^31-1"),
           (b"a1\t99999999999999999999999\n", 1, "0 or above 2^31-1"), (b"a1\t7\nno tab at the end", 2, "fewer than two fields")]


def test_every_refusal_of_the_sites_file_names_its_line(built, committed_session, tmp_path):
    from arriba_amd import _capi
    host = committed_session._lib
    path = str(tmp_path / "refused.sites")
    for text, line, reason in REFUSED:
        open(path, "wb").write(text)
        with pytest.raises(ValueError, match="line %d$" % line):
            lib.parse_sites(text)
        sites = _capi.AlleleSites()
        assert host.ahost_allele_sites_load(path.encode(), None, 0, ctypes.byref(sites)) != 0, text
        message = host.ahost_last_error().decode()
        assert "--allele-sites" in message and "refused.sites" in message and "line %d: " % line in message and reason in message, (text, message)
        assert not sites.owner
    sites = _capi.AlleleSites()
    assert host.ahost_allele_sites_load(str(tmp_path / "missing.sites").encode(), None, 0, ctypes.byref(sites)) != 0 and "cannot read" in host.ahost_last_error().decode()
    assert host.ahost_allele_sites_load(str(tmp_path).encode(), None, 0, ctypes.byref(sites)) != 0 and "cannot read" in host.ahost_last_error().decode()
    # 2^31-1 is a position, the last line needs no end, an empty file is valid; without a header every line is unplaced
    open(path, "wb").write(b"a1\t2147483647\tx\nchr2\t007")
    assert host.ahost_allele_sites_load(path.encode(), None, 0, ctypes.byref(sites)) == 0, host.ahost_last_error()
    assert sites.n_sites == 2 and sites.placed == 0 and sites.sites[0].pos == 2 ** 31 - 2 and sites.sites[1].pos == 6 and sites.sites[1].ref == 0xFFFFFFFF
    host.ahost_allele_sites_free(ctypes.byref(sites))
    open(path, "wb").write(b"")
    assert host.ahost_allele_sites_load(path.encode(), None, 0, ctypes.byref(sites)) == 0 and sites.n_sites == 0
    host.ahost_allele_sites_free(ctypes.byref(sites))
    # thresholds above 255
    header = lib.bam_header(lib.HEADER)
    assert host.ahost_allele_sites_load(SITES.encode(), header, len(header), ctypes.byref(sites)) == 0 and sites.placed == 25
    rows = ctypes.POINTER(_capi.AlleleRow)()
    for thresholds in ((256, 0), (0, 256)):
        assert host.ahost_allele_counts_of(committed_session._session, header, len(header), None, 0, ctypes.byref(sites), thresholds[0], thresholds[1], ctypes.byref(rows), None) != 0
        assert "a threshold above 255" in host.ahost_last_error().decode()
    host.ahost_allele_sites_free(ctypes.byref(sites))


def _harness(target):
    directory = os.path.join(conftest.ROOT, "tests", "emu")
    subprocess.run(["make", "-s", "-C", directory, target], check=True)
    return os.path.join(directory, target)


def _arguments(sample, outputs, extra):
    return ["-x", sample, "-g", os.path.join(GOLDEN, "hand_made.gtf"), "-a", os.path.join(GOLDEN, "hand_made.fa"), "-i", lib.COMMITTED_CONTIGS, "-o", outputs[0], "-O", outputs[1], "-f", "blacklist"] + extra


def test_host_ingest_through_the_command_line(built, emu_api, tmp_path):
    """--host-ingest --allele-sites --allele-counts: the C++ driver (over the host stepping harness, where there is no GPU) writes the committed table, and fusions.tsv is the one
    of a run without the options"""
    sample = os.path.join(GOLDEN, "hand_made.sam")
    files = {}
    for option in ([], ["--allele-sites", SITES, "--allele-counts", str(tmp_path / "alleles.tsv")] + HAND_MADE_OPTIONS):
        outputs = [str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv")]
        result = subprocess.run([_harness("workflow_on_harness")] + _arguments(sample, outputs, ["--host-ingest"] + option), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
        assert result.returncode == 0, result.stderr[-2000:]
        assert (HAND_MADE_LINE in result.stdout) == bool(option) and ("Counting alleles" in result.stdout) == bool(option)
        files[bool(option)] = [open(path, "rb").read() for path in outputs]
    assert open(str(tmp_path / "alleles.tsv"), "rb").read() == _golden("hand_made.tsv")
    assert files[True] == files[False] and sorted(os.listdir(str(tmp_path))) == ["alleles.tsv", "discarded.tsv", "fusions.tsv"]


def _refused(command, tmp_path, message):
    result = subprocess.run(command, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert result.returncode != 0 and message in result.stderr, (message, result.stderr[-2000:])
    assert not [name for name in os.listdir(str(tmp_path)) if name.startswith(("alleles", "fusions", "discarded"))], os.listdir(str(tmp_path))


def test_refusals_before_the_input_is_read(built, emu_api, tmp_path):
    """one path without the other, a threshold above 255, a sites file that does not parse, a path in a missing directory: refused with --host-ingest as without it, before the
    feed, and nothing is written.  The test-only build of the C++ driver against the host stepping harness has no twin of the kernels of agpu_alleles.hip: without --host-ingest it
    says so, also before the feed"""
    sample, outputs, table = os.path.join(GOLDEN, "hand_made.sam"), [str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv")], str(tmp_path / "alleles.tsv")
    bad = str(tmp_path / "bad.sites")
    open(bad, "w").write("a1\t5\na1\tfive\n")
    for ingest in (["--host-ingest"], []):
        command = [_harness("workflow_on_harness")] + _arguments(sample, outputs, ingest)
        _refused(command + ["--allele-sites", SITES], tmp_path, "ERROR: --allele-sites and --allele-counts need each other")
        _refused(command + ["--allele-counts", table], tmp_path, "ERROR: --allele-sites and --allele-counts need each other")
        _refused(command + ["--allele-sites", SITES, "--allele-counts", table, "--allele-min-mapq", "256"], tmp_path, "ERROR: --allele-min-mapq is at most 255")
        _refused(command + ["--allele-sites", SITES, "--allele-counts", table, "--allele-min-baseq", "256"], tmp_path, "ERROR: --allele-min-baseq is at most 255")
        _refused(command + ["--allele-sites", SITES, "--allele-counts", table, "--allele-min-baseq", "-1"], tmp_path, "invalid argument to --allele-min-baseq")
        if ingest:
            _refused(command + ["--allele-sites", bad, "--allele-counts", table], tmp_path, "bad.sites' line 2: the position holds something that is not a digit")
            _refused(command + ["--allele-sites", str(tmp_path / "none.sites"), "--allele-counts", table], tmp_path, "--allele-sites: cannot read")
        else:
            _refused(command + ["--allele-sites", SITES, "--allele-counts", table], tmp_path, "--allele-counts needs the device library (agpu_allele_counts)")
    _refused([WORKFLOW] + _arguments(sample, outputs, ["--allele-sites", SITES, "--allele-counts", str(tmp_path / "missing" / "alleles.tsv")]), tmp_path, "parent directory of output file")
    usage = subprocess.run([WORKFLOW, "-h"], stdout=subprocess.PIPE, universal_newlines=True, timeout=60).stdout
    assert "--allele-sites FILE --allele-counts FILE" in usage and "--allele-min-mapq N" in usage and "--allele-min-baseq N" in usage


def test_a_sample_over_ranks_is_refused_before_the_feed(built, emu_api, tmp_path):
    """one sample over several ranks: refused before a byte of the file is fed (the driver over the harness, a communicator of one rank that does nothing)"""
    from arriba_amd import _capi
    driver = ctypes.CDLL(_harness("libworkflow_on_harness.so"))
    driver.arriba_workflow_open.restype = ctypes.c_void_p
    driver.arriba_workflow_last_error.restype = ctypes.c_char_p
    options = _capi.WorkflowOptions()
    driver.arriba_workflow_default_options(ctypes.byref(options))
    assert options.allele_sites_file is None and options.allele_counts_file is None and options.allele_min_mapq == 0 and options.allele_min_baseq == 13
    options.assembly_file, options.gene_annotation_file, options.interesting_contigs = os.path.join(GOLDEN, "hand_made.fa").encode(), os.path.join(GOLDEN, "hand_made.gtf").encode(), lib.COMMITTED_CONTIGS.encode()
    session = ctypes.c_void_p(driver.arriba_workflow_open(ctypes.byref(options)))
    assert session, driver.arriba_workflow_last_error()
    nothing = lambda *arguments: 0  # noqa: E731
    communicator = _capi.WorkflowCommunicator(0, 1, None, _capi.ALL_GATHER(nothing), _capi.ALL_REDUCE_INT64(nothing), _capi.ALL_REDUCE_MAX_BYTES(nothing), None)
    assert driver.arriba_workflow_set_communicator(session, ctypes.byref(communicator)) == 0
    driver.arriba_workflow_allele_counts.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32]
    assert driver.arriba_workflow_allele_counts(session, SITES.encode(), str(tmp_path / "alleles.tsv").encode(), 0, 13) == 0
    status = driver.arriba_workflow_sample(session, os.path.join(GOLDEN, "hand_made.sam").encode(), str(tmp_path / "fusions.tsv").encode(), None, None, None)
    message = driver.arriba_workflow_last_error().decode()
    driver.arriba_workflow_close(session)
    assert status != 0 and "ERROR: allele counts of one sample over several GPUs are not supported" in message
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


KNOBS = [{}, {"ARRIBA_ALLELE_PLAIN_ATOMICS": "1"}, {"ARRIBA_ALLELE_NO_BITMAP": "1"}, {"ARRIBA_INGEST_WINDOWS": "1048576,65536"}]


def _set(knobs, monkeypatch):
    for knob in ("ARRIBA_INGEST_WINDOWS", "ARRIBA_ALLELE_PLAIN_ATOMICS", "ARRIBA_ALLELE_NO_BITMAP"):
        if knob in knobs:
            monkeypatch.setenv(knob, knobs[knob])
        else:
            monkeypatch.delenv(knob, raising=False)


def _device_counts(pipeline, cases, name, tmp_path):
    """the case through an ingest and agpu_allele_counts -> (the bytes of the file, the statistics)"""
    header, record_bytes, _, case, sites_path = cases(name)
    sample = str(tmp_path / (name + ".bam"))
    lib.write_bgzf(sample, header + record_bytes, 0)
    pipeline.read_chimeric_alignments(sample)
    os.remove(sample)
    path = str(tmp_path / (name + ".tsv"))
    stats = pipeline.write_allele_counts(sites_path, path, case["min_mapq"], case["min_baseq"])
    text = open(path, "rb").read()
    assert not os.path.exists(path + ".tmp") and pipeline.allele_counts_allocated_bytes() == 0, name
    os.remove(path)
    return text, stats


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["committed_and_made", "seeded"])
@pytest.mark.parametrize("knobs", KNOBS, ids=["no_knobs", "plain_atomics", "no_bitmap", "ingest_windows"])
def test_device_file_is_the_host_file(knobs, group, built, pipeline, cases, host_side, tmp_path, monkeypatch):
    """the file of agpu_allele_counts equals the host stepping byte for byte and the statistics are equal: the committed case, the hot site (70 001 records over one site, then a
    wavefront that shows one base, then one over two neighbours), 65 records, 150 sites under one read, one record of 601 operations, 1 000 sites that no read covers, no records,
    no sites, no references; 50 seeded inputs in one session; with one atomic per lane instead of the leader loop, without the window bitmap, with the ingest cut into windows"""
    _set(knobs, monkeypatch)
    for name in (["hand_made", "hot", "wavefront", "dense", "long_cigar", "sparse", "no_records", "no_sites", "header_only"] if group == "committed_and_made" else SEEDED):
        text, stats = _device_counts(pipeline, cases, name, tmp_path)
        expected_text, expected = host_side(name)
        print(name, stats)
        assert text == expected_text, name
        assert {key: stats[key] for key in COUNTED} == {key: expected[key] for key in COUNTED}, name
        assert (stats["peak_bytes"] > 0) == (stats["records"] > 0 or stats["sites"] > 0), name
        _invariant(text, stats, cases(name)[3])
        if name == "hand_made":
            assert text == _golden("hand_made.tsv")


def _command_line(sample, outputs, extra):
    return subprocess.run(["timeout", "-k", "10", "120", WORKFLOW] + _arguments(sample, outputs, extra), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)


@pytest.fixture(scope="module")
def without_the_option(tmp_path_factory):
    """fusions.tsv and discarded.tsv of the committed case from a run of the command line without the options"""
    directory = tmp_path_factory.mktemp("plain")
    outputs = [str(directory / "fusions.tsv"), str(directory / "discarded.tsv")]
    result = _command_line(os.path.join(GOLDEN, "hand_made.sam"), outputs, [])
    assert result.returncode == 0, result.stderr[-2000:]
    assert "Counting alleles" not in result.stdout
    return [open(path, "rb").read() for path in outputs]


@pytest.mark.gpu
@pytest.mark.parametrize("container", ["stored_bgzf", "deflated_bgzf", "sam_text", "host_ingest"])
def test_command_line_writes_the_table_next_to_the_fusions(container, built, cases, without_the_option, tmp_path):
    """the committed case as BAM and as SAM text, and with --host-ingest: the committed table, and the other outputs as without the options"""
    os.mkdir(str(tmp_path / "in")); os.mkdir(str(tmp_path / "out"))
    sample = str(tmp_path / "in" / "sample.bam")
    if container in ("sam_text", "host_ingest"):
        sample = os.path.join(GOLDEN, "hand_made.sam")
    else:
        lib.write_bgzf(sample, cases("hand_made")[0] + cases("hand_made")[1], 0 if container == "stored_bgzf" else 6)
    outputs = [str(tmp_path / "out" / "fusions.tsv"), str(tmp_path / "out" / "discarded.tsv")]
    result = _command_line(sample, outputs, ["--allele-sites", SITES, "--allele-counts", str(tmp_path / "out" / "alleles.tsv")] + HAND_MADE_OPTIONS + (["--host-ingest"] if container == "host_ingest" else []))
    assert result.returncode == 0, result.stderr[-2000:]
    assert open(str(tmp_path / "out" / "alleles.tsv"), "rb").read() == _golden("hand_made.tsv")
    assert HAND_MADE_LINE in result.stdout
    assert [open(path, "rb").read() for path in outputs] == without_the_option
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["alleles.tsv", "discarded.tsv", "fusions.tsv"]


@pytest.mark.gpu
def test_command_line_refusals_on_the_device_path(built, tmp_path):
    """the refusals of the driver that is linked with the device library: before the feed, nothing written"""
    sample, outputs, table = os.path.join(GOLDEN, "hand_made.sam"), [str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv")], str(tmp_path / "alleles.tsv")
    bad = str(tmp_path / "bad.sites")
    open(bad, "w").write("a1\t5\n\na1\n")
    command = ["timeout", "-k", "10", "120", WORKFLOW] + _arguments(sample, outputs, [])
    _refused(command + ["--allele-sites", SITES], tmp_path, "ERROR: --allele-sites and --allele-counts need each other")
    _refused(command + ["--allele-counts", table], tmp_path, "ERROR: --allele-sites and --allele-counts need each other")
    _refused(command + ["--allele-sites", SITES, "--allele-counts", table, "--allele-min-mapq", "256"], tmp_path, "ERROR: --allele-min-mapq is at most 255")
    _refused(command + ["--allele-sites", SITES, "--allele-counts", table, "--allele-min-baseq", "1000"], tmp_path, "ERROR: --allele-min-baseq is at most 255")
    _refused(command + ["--allele-sites", bad, "--allele-counts", table], tmp_path, "bad.sites' line 3: fewer than two fields")
    _refused(command + ["--allele-sites", str(tmp_path / "none.sites"), "--allele-counts", table], tmp_path, "--allele-sites: cannot read")


@pytest.mark.gpu
def test_session_writes_the_table_of_the_sample_that_asked_for_it(built, cases, without_the_option, tmp_path):
    """three samples in a queue: none, the committed sites and thresholds, then other sites, another path and other thresholds behind it; no buffer of the option is left on
    either lane"""
    from arriba_amd.pipeline import WorkflowSession
    sample = os.path.join(GOLDEN, "hand_made.sam")
    other = str(tmp_path / "other.sites")
    open(other, "w").write("a1\t51\n2\t5\n")
    session = WorkflowSession(os.path.join(GOLDEN, "hand_made.fa"), os.path.join(GOLDEN, "hand_made.gtf"), interesting_contigs=lib.COMMITTED_CONTIGS, params={"disable_filters": ["blacklist"]})
    for directory in ("first", "second", "third"):
        os.mkdir(str(tmp_path / directory))
    session.submit(sample)
    session.submit(sample, allele_sites_file=SITES, allele_counts_file=str(tmp_path / "second" / "alleles.tsv"), allele_min_mapq=20, allele_min_baseq=13)
    session.sample(sample, str(tmp_path / "first" / "fusions.tsv"))
    assert session.timing["allele_counts"] == 0
    session.submit(sample, allele_sites_file=other, allele_counts_file=str(tmp_path / "third" / "counts.tsv"), allele_min_mapq=0, allele_min_baseq=0)
    session.sample(sample, str(tmp_path / "second" / "fusions.tsv"))
    assert session.timing["allele_counts"] > 0
    session.sample(sample, str(tmp_path / "third" / "fusions.tsv"))
    assert session.timing["allele_counts"] > 0
    for context in session._lane_contexts():
        count = ctypes.c_uint64(1)
        assert session.api.allele_counts_allocated_bytes(context, ctypes.byref(count)) == 0 and count.value == 0
    session.close()
    assert os.listdir(str(tmp_path / "first")) == ["fusions.tsv"] and sorted(os.listdir(str(tmp_path / "second"))) == ["alleles.tsv", "fusions.tsv"] and sorted(os.listdir(str(tmp_path / "third"))) == ["counts.tsv", "fusions.tsv"]
    assert open(str(tmp_path / "second" / "alleles.tsv"), "rb").read() == _golden("hand_made.tsv")
    assert open(str(tmp_path / "third" / "counts.tsv")).read() == lib.HEADER_LINE + "a1\t51\tA\t0\t1\t1\t1\t0\t0\t0\t0\n2\t5\tC\t0\t1\t0\t0\t0\t0\t0\t0\n"
    for directory in ("first", "second", "third"):
        assert open(str(tmp_path / directory / "fusions.tsv"), "rb").read() == without_the_option[0]


@pytest.mark.gpu
def test_refusals_and_the_off_switch(built, cases, tmp_path, monkeypatch):
    """with the option off no kernel whose name begins with allele is in the kernel profile and no buffer of it exists; before an ingest, for a part of a sample, with the stream
    given back, behind the begin of the next ingest, with a threshold above 255 and with a site beyond its reference agpu_allele_counts is refused with a message"""
    from arriba_amd import _capi
    from arriba_amd.pipeline import ArribaError, DevicePipeline, HostSession
    api, params = _capi.bind_device_api(_capi.device_library(), "agpu_"), _capi.Params()
    api.default_params(ctypes.byref(params))
    fresh = api.create(0, ctypes.byref(params))
    assert fresh, api.last_error()
    rows = ctypes.POINTER(_capi.AlleleRow)()
    refused = api.allele_counts(fresh, None, 0, None, 0, 0, 13, ctypes.byref(rows), None)  # before an ingest
    message = api.last_error()
    api.destroy(fresh)
    assert refused != 0 and b"agpu_allele_counts: the record stream of the last ingest is not on the device any more" in message
    sample = os.path.join(GOLDEN, "hand_made.sam")
    made = DevicePipeline(HostSession(os.path.join(GOLDEN, "hand_made.fa"), os.path.join(GOLDEN, "hand_made.gtf"), interesting_contigs=lib.COMMITTED_CONTIGS), bam=sample)
    made.set_profiling(True)
    made.read_chimeric_alignments(sample)
    made.run_workflow(str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv"))
    assert made.kernel_profile() and not [launch for launch in made.kernel_profile() if launch[0].startswith("allele")] and made.allele_counts_allocated_bytes() == 0
    # ... and on, through the stages of the pipeline
    made.read_chimeric_alignments(sample)
    with pytest.raises(ArribaError, match="--allele-sites and --allele-counts need each other"):
        made.run_workflow(str(tmp_path / "again.tsv"), None, allele_sites_file=SITES)
    made.read_chimeric_alignments(sample)
    made.run_workflow(str(tmp_path / "again.tsv"), None, allele_sites_file=SITES, allele_counts_file=str(tmp_path / "alleles.tsv"), allele_min_mapq=20, allele_min_baseq=13)
    names = set(launch[0] for launch in made.kernel_profile())
    assert {"allele_bitmap_kernel", "allele_count_kernel", "allele_rows_kernel", "allele_ref_kernel"} <= names
    assert made.allele_counts_allocated_bytes() == 0
    assert open(str(tmp_path / "alleles.tsv"), "rb").read() == _golden("hand_made.tsv") and open(str(tmp_path / "again.tsv")).read() == open(str(tmp_path / "fusions.tsv")).read()
    # thresholds and sites the call does not admit
    made.read_chimeric_alignments(sample)
    for thresholds in ((256, 13), (0, 256)):
        with pytest.raises(ArribaError, match="agpu_allele_counts: a threshold above 255"):
            made.allele_counts(SITES, *thresholds)
    contigs = _capi.DepthContigs()
    assert made.session._lib.ahost_depth_contigs_of_session(made.session._session, ctypes.byref(contigs)) == 0
    beyond = (_capi.AlleleSite * 2)(_capi.AlleleSite(0, 99), _capi.AlleleSite(0, 100))
    assert made.api.allele_counts(made.ctx, beyond, 2, contigs.length, contigs.n_ref, 0, 13, ctypes.byref(rows), None) != 0 and b"site 1 lies on no reference of the header or beyond its length" in made.api.last_error()
    assert made.api.allele_counts(made.ctx, beyond, 2, contigs.length, contigs.n_ref + 1, 0, 13, ctypes.byref(rows), None) != 0 and b"the lengths are not those of the references of the last ingest" in made.api.last_error()
    # a part of a sample (which only a BAM file has)
    os.mkdir(str(tmp_path / "in"))
    lib.write_bgzf(str(tmp_path / "in" / "hand_made.bam"), cases("hand_made")[0] + cases("hand_made")[1], 0)
    made._ingest_records(str(tmp_path / "in" / "hand_made.bam"), False, 100, 64 << 20, part=0, parts=2)
    with pytest.raises(ArribaError, match="allele counts of one sample over several GPUs are not supported"):
        made.write_allele_counts(SITES, str(tmp_path / "part.tsv"))
    # the stream was given back behind the ingest: no ingest kept
    monkeypatch.setenv("ARRIBA_RELEASE_INGEST_BUFFERS", "1")
    made.read_chimeric_alignments(sample)
    monkeypatch.delenv("ARRIBA_RELEASE_INGEST_BUFFERS")
    with pytest.raises(ArribaError, match="agpu_allele_counts: the record stream of the last ingest is not on the device any more"):
        made.write_allele_counts(SITES, str(tmp_path / "gone.tsv"))
    assert made.allele_counts_allocated_bytes() == 0
    # the next read_chimeric_alignments has begun
    made.read_chimeric_alignments(sample)
    host, handle, config = made.session._lib, made.session._session, _capi.IngestConfig()
    assert host.ahost_bam_open(handle, sample.encode(), 0, 100, ctypes.byref(config)) == 0
    made._check(made.api.ingest_begin(made.ctx, ctypes.byref(config)))
    with pytest.raises(ArribaError, match="an ingest is under way|not on the device any more"):
        made.write_allele_counts(SITES, str(tmp_path / "second.tsv"))
    host.ahost_bam_close(handle)
    made.close()
    assert sorted(os.listdir(str(tmp_path))) == ["again.tsv", "alleles.tsv", "discarded.tsv", "fusions.tsv", "in"]
