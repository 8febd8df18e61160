"""--realign-reads [--realign-kept]: the records of -x split into the templates that must be aligned again and the templates that are passed on, as SAM text (the rule: DESIGN.md
4.18).

tests/golden/realign_split/hand_made.sam (paired-end) and hand_made_se.sam (single-end) are cases a reader can check by eye, one template per clause of the rule, with the two
files each must give next to them; tests/realign_split_lib.py restates the rule in plain Python with dicts, string formatting and the regular expressions of the rule on the CIGAR
text, test_restatement_equals_the_committed_files holds it to those cases, and only therefore it is the independent side for inputs made at test time.  The CPU tier runs
arriba_amd/csrc/device/realign_core.hpp stepped on the host (ahost_realign_*); the GPU tier the kernels of agpu_realign.hip, whose files must equal the host's byte for byte and
whose statistics must equal the host's."""
import ctypes
import os
import subprocess
import sys

import pytest

import conftest
import realign_split_lib as lib

GOLDEN = lib.GOLDEN
WORKFLOW = os.path.join(conftest.ROOT, "arriba_amd", "lib", "arriba_gpu_workflow")
SEEDED = ["seed%d" % (1800 + k) for k in range(50)]
COUNTED = lib.COUNTED
MADE = {"templates65": lambda: lib.templates_case(65), "templates129": lambda: lib.templates_case(129), "templates65_se": lambda: lib.templates_case(65, False), "templates129_se": lambda: lib.templates_case(129, False),
        "long_cigar": lib.long_cigar_case, "long_name": lib.long_name_case, "no_records": lib.no_records_case, "header_only": lib.header_only_case, "all_kept": lib.all_kept_case, "all_realign": lib.all_realign_case,
        "single_end": lib.single_end_case}
COMMITTED = ["hand_made", "hand_made_se"]
HAND_MADE_STATS = {"records": 35, "templates": 17, "realign_templates": 7, "kept_templates": 8, "dropped_secondary": 2, "extra": 1, "orphans": 2, "placeholder_cigar": 1, "realign_bytes": 992, "kept_bytes": 1049, "layout": "PE"}
HAND_MADE_SE_STATS = {"records": 22, "templates": 20, "realign_templates": 9, "kept_templates": 11, "dropped_secondary": 2, "extra": 0, "orphans": 0, "placeholder_cigar": 1, "realign_bytes": 574, "kept_bytes": 650, "layout": "SE"}
HAND_MADE_LINE = "Splitting reads for realignment (layout=PE, templates=17, realign=7, kept=8, dropped_secondary=2, extra=1, orphans=2)"
KEPT_HEADER = b"@HD\tVN:1.4\tSO:unsorted\n@SQ\tSN:a1\tLN:100\n@SQ\tSN:chr2\tLN:50\n"
KNOBS = ("ARRIBA_REALIGN_TEXT_WINDOW", "ARRIBA_REALIGN_TEXT_FORM", "ARRIBA_REALIGN_LAUNCH_ITEMS", "ARRIBA_REALIGN_HASH_BITS")


def _golden(name):
    return open(os.path.join(GOLDEN, name), "rb").read()


def _invariant(realign, kept, stats, header=KEPT_HEADER):
    """realign_templates + kept_templates + orphans = templates, the sums of the line lengths are the bytes, every line has eleven fields, the kept file begins with its header"""
    assert stats["realign_templates"] + stats["kept_templates"] + stats["orphans"] == stats["templates"]
    assert kept.startswith(header)
    lines = {"realign": realign.split(b"\n"), "kept": kept[len(header):].split(b"\n")}
    per_template = 2 if stats["layout"] == "PE" else 1
    for name, text in (("realign", realign), ("kept", kept[len(header):])):
        assert lines[name][-1] == b"" and all(len(line.split(b"\t")) == 11 for line in lines[name][:-1]), name
        assert len(lines[name]) - 1 == per_template * stats[name + "_templates"], name
        assert sum(len(line) + 1 for line in lines[name][:-1]) == stats[name + "_bytes"] == len(text), name
    assert stats["dropped_secondary"] + stats["extra"] <= stats["records"]


@pytest.fixture(scope="module")
def assembly():
    return lib.load_assembly()


@pytest.fixture(scope="module")
def cases(assembly):
    """name -> (BAM header, record bytes, (realign, kept, stats) of the restatement, the case): made once"""
    cache = {}

    def get(name):
        if name not in cache:
            case = lib.committed_case(name) if name in COMMITTED else lib.random_case(int(name[4:])) if name.startswith("seed") else MADE[name]()
            cache[name] = (lib.bam_header(case["references"]), lib.bam_records(case), lib.restate(assembly, case), case)
        return cache[name]
    return get


# ---- the host side ------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def committed_session(built):
    from arriba_amd.pipeline import HostSession
    session = HostSession(os.path.join(GOLDEN, "hand_made.fa"), os.path.join(GOLDEN, "hand_made.gtf"), interesting_contigs=lib.COMMITTED_CONTIGS)
    yield session
    session.close()


def _host_split(session, header, record_bytes, want_kept=1):
    """-> (realign, kept or None, statistics) of ahost_realign_split_of"""
    from arriba_amd import _capi
    from arriba_amd.pipeline import realign_stats_of
    host, stats = session._lib, _capi.RealignStats()
    realign, realign_bytes, kept, kept_bytes = ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_void_p(), ctypes.c_uint64()
    status = host.ahost_realign_split_of(session._session, header, len(header), record_bytes, len(record_bytes), want_kept, ctypes.byref(realign), ctypes.byref(realign_bytes), ctypes.byref(kept) if want_kept else None,
                                         ctypes.byref(kept_bytes) if want_kept else None, ctypes.byref(stats))
    assert status == 0, host.ahost_last_error()
    return ctypes.string_at(realign, realign_bytes.value), ctypes.string_at(kept, kept_bytes.value) if want_kept else None, realign_stats_of(stats)


@pytest.fixture(scope="module")
def host_side(cases, committed_session):
    """name -> what the host stepping gives: computed once, compared against by every test"""
    cache = {}

    def get(name):
        if name not in cache:
            header, record_bytes, _, _ = cases(name)
            cache[name] = _host_split(committed_session, header, record_bytes)
        return cache[name]
    return get


# ---- CPU tier -----------------------------------------------------------------------------------------------------------------------------------------------------

def test_restatement_equals_the_committed_files(assembly):
    """the restatement of the rule against the cases that are checked by eye, and its line formatter against tools/bam_to_sam.py on them"""
    sys.path.insert(0, os.path.join(conftest.ROOT, "tools"))
    import bam_to_sam
    assert assembly == [("a1", 100), ("2", 50)]
    for name, expected in (("hand_made", HAND_MADE_STATS), ("hand_made_se", HAND_MADE_SE_STATS)):
        case = lib.committed_case(name)
        realign, kept, stats = lib.restate(assembly, case)
        assert realign == _golden(name + ".realign.sam") and kept == _golden(name + ".kept.sam")
        assert stats == expected
        assert case["references"] == lib.HEADER
        _invariant(realign, kept, stats)
        text, _ = bam_to_sam.bam_to_sam(lib.bam_header(case["references"]) + lib.bam_records(case), with_header=False)
        assert text == "".join(lib.line_of(record) for record in case["records"]).encode()
        assert all(len(_golden(name + kind)) < 100000 for kind in (".sam", ".realign.sam", ".kept.sam"))
    # every clause of the rule has its template in the paired-end case
    names = lambda text: [line.split(b"\t")[0] for line in text.split(b"\n") if line and not line.startswith(b"@")][::2]  # noqa: E731
    assert names(_golden("hand_made.realign.sam")) == [b"u1", b"c1", b"c2", b"d1", b"o1", b"n1", b"g1"]
    assert names(_golden("hand_made.kept.sam")) == [b"k1", b"c3", b"c4", b"c5", b"x1", b"e1", b"e2", b"f1"]


def test_host_gives_the_committed_bytes(built, cases, host_side, committed_session, tmp_path):
    from arriba_amd import _capi
    host = committed_session._lib
    for name, expected in (("hand_made", HAND_MADE_STATS), ("hand_made_se", HAND_MADE_SE_STATS)):
        realign, kept, stats = host_side(name)
        assert realign == _golden(name + ".realign.sam") and kept == _golden(name + ".kept.sam")
        assert {key: stats[key] for key in COUNTED} == expected == cases(name)[2][2]
        # without the kept file the statistics are the same
        only, nothing, fewer = _host_split(committed_session, cases(name)[0], cases(name)[1], want_kept=0)
        assert only == realign and nothing is None and fewer == stats
        # ... and through the project's own readers of SAM text and of BAM, which leave no temporary file
        sample = str(tmp_path / (name + ".bam"))
        lib.write_bgzf(sample, cases(name)[0] + cases(name)[1], 6)
        for source in (os.path.join(GOLDEN, name + ".sam"), sample):
            paths, counted = [str(tmp_path / "realign.sam"), str(tmp_path / "kept.sam")], _capi.RealignStats()
            assert host.ahost_realign_split_file(committed_session._session, source.encode(), paths[0].encode(), paths[1].encode(), ctypes.byref(counted)) == 0, host.ahost_last_error()
            assert [open(path, "rb").read() for path in paths] == [realign, kept] and counted.templates == expected["templates"]
            assert sorted(os.listdir(str(tmp_path))) == sorted(["realign.sam", "kept.sam", name + ".bam"])
            os.remove(paths[1])
            assert host.ahost_realign_split_file(committed_session._session, source.encode(), paths[0].encode(), None, None) == 0
            assert sorted(os.listdir(str(tmp_path))) == sorted(["realign.sam", name + ".bam"])
            os.remove(paths[0])
        assert host.ahost_realign_split_file(committed_session._session, sample.encode(), str(tmp_path / "missing" / "realign.sam").encode(), None, None) != 0
        assert host.ahost_realign_split_file(committed_session._session, sample.encode(), str(tmp_path / "realign.sam").encode(), str(tmp_path / "missing" / "kept.sam").encode(), None) != 0
        assert os.listdir(str(tmp_path)) == [name + ".bam"]
        os.remove(sample)


@pytest.mark.parametrize("name", ["seeded"] + sorted(MADE))
def test_host_equals_the_restatement(name, built, cases, host_side):
    """both files and the statistics, and the invariants"""
    seen = dict.fromkeys(COUNTED[1:-1], 0)
    layouts = set()
    for case_name in (SEEDED if name == "seeded" else [name]):
        realign, kept, stats = host_side(case_name)
        expected_realign, expected_kept, expected = cases(case_name)[2]
        assert expected["records"] <= 700
        assert realign == expected_realign, case_name
        assert kept == expected_kept, case_name
        assert {key: stats[key] for key in COUNTED} == expected, case_name
        _invariant(realign, kept, stats, b"@HD\tVN:1.4\tSO:unsorted\n@SQ\tSN:a1\tLN:100\n@SQ\tSN:2\tLN:50\n" if name == "header_only" else KEPT_HEADER)
        for key in seen:
            seen[key] += stats[key]
        layouts.add(stats["layout"])
    if name == "seeded":  # the seeded set as a whole exercises the rule
        assert layouts == {"PE", "SE"} and all(total > 50 for key, total in seen.items() if key != "placeholder_cigar"), seen
    if name.startswith("templates"):
        count = int(name[9:].split("_")[0])
        assert stats["templates"] == count and stats["realign_templates"] == (count + 2) // 3 and stats["layout"] == ("SE" if name.endswith("_se") else "PE")
    if name == "long_cigar":
        assert stats["realign_templates"] == 1 and realign.count(b"1N1M") == 300 and realign.split(b"\n")[1].split(b"\t")[5].endswith(b"1D1M12S") and b"9S1M1N1M" in kept
    if name == "long_name":
        assert realign.startswith(b"m" * 254 + b"\t99\t") and kept[len(KEPT_HEADER):].startswith(b"n" * 254 + b"\t99\t")
    if name in ("no_records", "header_only"):
        assert realign == b"" and stats["layout"] == "SE" and stats["templates"] == 0
        assert kept == (KEPT_HEADER if name == "no_records" else b"@HD\tVN:1.4\tSO:unsorted\n@SQ\tSN:a1\tLN:100\n@SQ\tSN:2\tLN:50\n")
    if name == "all_kept":
        assert realign == b"" and stats["kept_templates"] == 70
    if name == "all_realign":
        assert kept == KEPT_HEADER and stats["realign_templates"] == 70


@pytest.mark.parametrize("bits", ["0", "3"])
def test_host_with_colliding_names(bits, built, cases, committed_session, monkeypatch):
    """the name hash cut to a few bits: every probe run is long, and the files do not change"""
    monkeypatch.setenv("ARRIBA_REALIGN_HASH_BITS", bits)
    for name in ["hand_made", "seed1801", "seed1803", "templates129"]:
        realign, kept, stats = _host_split(committed_session, cases(name)[0], cases(name)[1])
        assert (realign, kept, {key: stats[key] for key in COUNTED}) == cases(name)[2], name


def test_a_record_cut_short_fails_the_stream(built, cases, committed_session):
    host = committed_session._lib
    header, record_bytes, _, _ = cases("hand_made")
    pointers = [ctypes.c_void_p(), ctypes.c_uint64(), ctypes.c_void_p(), ctypes.c_uint64()]
    for cut in (1, 20, 45):
        assert host.ahost_realign_split_of(committed_session._session, header, len(header), record_bytes, len(record_bytes) - cut, 1, *[ctypes.byref(p) for p in pointers], None) != 0
        assert b"failed to load alignments" in host.ahost_last_error()
    # a record whose name is missing (l_read_name 0) and one that names a reference the header does not have
    for at, value in ((12, b"\0"), (4, b"\x07\0\0\0")):
        broken = record_bytes[:at] + value + record_bytes[at + len(value):]
        assert host.ahost_realign_split_of(committed_session._session, header, len(header), broken, len(broken), 1, *[ctypes.byref(p) for p in pointers], None) != 0
        assert b"failed to load alignments" in host.ahost_last_error()


def _harness(target):
    directory = os.path.join(conftest.ROOT, "tests", "emu")
    subprocess.run(["make", "-s", "-C", directory, target], check=True)
    return os.path.join(directory, target)


def _arguments(sample, outputs, extra):
    return ["-x", sample, "-g", os.path.join(GOLDEN, "hand_made.gtf"), "-a", os.path.join(GOLDEN, "hand_made.fa"), "-i", lib.COMMITTED_CONTIGS, "-o", outputs[0], "-O", outputs[1], "-f", "blacklist"] + extra


def test_host_ingest_through_the_command_line(built, emu_api, tmp_path):
    """--host-ingest --realign-reads --realign-kept: the C++ driver (over the host stepping harness, where there is no GPU) writes the committed files, and fusions.tsv is the one
    of a run without the options"""
    sample = os.path.join(GOLDEN, "hand_made.sam")
    files = {}
    for option in ([], ["--realign-reads", str(tmp_path / "realign.sam"), "--realign-kept", str(tmp_path / "kept.sam")]):
        outputs = [str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv")]
        result = subprocess.run([_harness("workflow_on_harness")] + _arguments(sample, outputs, ["--host-ingest"] + option), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
        assert result.returncode == 0, result.stderr[-2000:]
        assert (HAND_MADE_LINE in result.stdout) == bool(option) and ("Splitting reads" in result.stdout) == bool(option)
        files[bool(option)] = [open(path, "rb").read() for path in outputs]
    assert open(str(tmp_path / "realign.sam"), "rb").read() == _golden("hand_made.realign.sam") and open(str(tmp_path / "kept.sam"), "rb").read() == _golden("hand_made.kept.sam")
    assert files[True] == files[False] and sorted(os.listdir(str(tmp_path))) == ["discarded.tsv", "fusions.tsv", "kept.sam", "realign.sam"]
    # the single-end case, and the file to realign alone
    outputs = [str(tmp_path / "se.tsv"), str(tmp_path / "se_discarded.tsv")]
    result = subprocess.run([_harness("workflow_on_harness")] + _arguments(os.path.join(GOLDEN, "hand_made_se.sam"), outputs, ["--host-ingest", "--realign-reads", str(tmp_path / "se.sam")]), stdin=subprocess.DEVNULL,
                            stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert "Splitting reads for realignment (layout=SE, templates=20, realign=9, kept=11, dropped_secondary=2, extra=0, orphans=0)" in result.stdout, result.stderr[-2000:]
    assert open(str(tmp_path / "se.sam"), "rb").read() == _golden("hand_made_se.realign.sam") and not os.path.exists(str(tmp_path / "se.sam.tmp"))


def _refused(command, tmp_path, message):
    result = subprocess.run(command, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert result.returncode != 0 and message in result.stderr, (message, result.stderr[-2000:])
    assert not [name for name in os.listdir(str(tmp_path)) if name.startswith(("realign", "kept", "fusions", "discarded"))], os.listdir(str(tmp_path))


def test_refusals_before_the_input_is_read(built, emu_api, tmp_path):
    """the kept file without the other, equal paths, a path another output has, a directory that does not exist or does not take a file: refused with --host-ingest as without it,
    before the feed, and nothing is written.  The test-only build of the C++ driver against the host stepping harness has no twin of the kernels of agpu_realign.hip: without
    --host-ingest it says so, also before the feed"""
    sample, outputs = os.path.join(GOLDEN, "hand_made.sam"), [str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv")]
    realign, kept = str(tmp_path / "realign.sam"), str(tmp_path / "kept.sam")
    os.mkdir(str(tmp_path / "closed"))
    os.chmod(str(tmp_path / "closed"), 0o500)
    for ingest in (["--host-ingest"], []):
        command = [_harness("workflow_on_harness")] + _arguments(sample, outputs, ingest)
        _refused(command + ["--realign-kept", kept], tmp_path, "ERROR: --realign-kept needs --realign-reads")
        _refused(command + ["--realign-reads", realign, "--realign-kept", realign], tmp_path, "ERROR: --realign-reads and --realign-kept name the same file")
        _refused(command + ["--realign-reads", outputs[0]], tmp_path, "ERROR: --realign-reads names a file that another option of the run names")
        _refused(command + ["--realign-reads", realign, "--realign-kept", outputs[1]], tmp_path, "ERROR: --realign-kept names a file that another option of the run names")
        _refused(command + ["--realign-reads", realign, "--realign-kept", str(tmp_path / "missing" / "kept.sam")], tmp_path, "parent directory of output file")
        if os.geteuid() != 0:  # (a directory without the write bit stops nobody who runs as root)
            _refused(command + ["--realign-reads", str(tmp_path / "closed" / "realign.sam")], tmp_path, "ERROR: failed to open '" + str(tmp_path / "closed" / "realign.sam") + ".tmp' for writing")
        if not ingest:
            _refused(command + ["--realign-reads", realign, "--realign-kept", kept], tmp_path, "--realign-reads needs the device library (agpu_realign_begin)")
    os.chmod(str(tmp_path / "closed"), 0o700)
    usage = subprocess.run([WORKFLOW, "-h"], stdout=subprocess.PIPE, universal_newlines=True, timeout=60).stdout
    assert "--realign-reads FILE [--realign-kept FILE]" in usage


def _driver():
    from arriba_amd import _capi
    driver = ctypes.CDLL(_harness("libworkflow_on_harness.so"))
    driver.arriba_workflow_open.restype = ctypes.c_void_p
    driver.arriba_workflow_last_error.restype = ctypes.c_char_p
    driver.arriba_workflow_realign.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p]
    driver.arriba_workflow_sample.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p]
    driver.arriba_workflow_close.argtypes = [ctypes.c_void_p]
    options = _capi.WorkflowOptions()
    driver.arriba_workflow_default_options(ctypes.byref(options))
    assert options.realign_reads_file is None and options.realign_kept_file is None
    options.assembly_file, options.gene_annotation_file, options.interesting_contigs = os.path.join(GOLDEN, "hand_made.fa").encode(), os.path.join(GOLDEN, "hand_made.gtf").encode(), lib.COMMITTED_CONTIGS.encode()
    return driver, options


def test_a_sample_over_ranks_is_refused_before_the_feed(built, emu_api, tmp_path):
    """one sample over several ranks: refused before a byte of the file is fed (the driver over the harness, a communicator of one rank that does nothing)"""
    from arriba_amd import _capi
    driver, options = _driver()
    session = ctypes.c_void_p(driver.arriba_workflow_open(ctypes.byref(options)))
    assert session, driver.arriba_workflow_last_error()
    nothing = lambda *arguments: 0  # noqa: E731
    communicator = _capi.WorkflowCommunicator(0, 1, None, _capi.ALL_GATHER(nothing), _capi.ALL_REDUCE_INT64(nothing), _capi.ALL_REDUCE_MAX_BYTES(nothing), None)
    assert driver.arriba_workflow_set_communicator(session, ctypes.byref(communicator)) == 0
    assert driver.arriba_workflow_realign(session, str(tmp_path / "realign.sam").encode(), None) == 0
    status = driver.arriba_workflow_sample(session, os.path.join(GOLDEN, "hand_made.sam").encode(), str(tmp_path / "fusions.tsv").encode(), None, None, None)
    message = driver.arriba_workflow_last_error().decode()
    driver.arriba_workflow_close(session)
    assert status != 0 and "ERROR: a split for realignment of one sample over several GPUs is not supported" in message
    assert os.listdir(str(tmp_path)) == []


def test_session_call_with_host_ingest(built, emu_api, tmp_path):
    """arriba_workflow_realign is of the next sample only: the first sample writes both files, the second none, and fusions.tsv is the same"""
    from arriba_amd import _capi
    driver, options = _driver()
    options.host_ingest = 1
    session = ctypes.c_void_p(driver.arriba_workflow_open(ctypes.byref(options)))
    assert session, driver.arriba_workflow_last_error()
    sample, timing = os.path.join(GOLDEN, "hand_made.sam").encode(), _capi.WorkflowTiming()
    assert driver.arriba_workflow_realign(session, str(tmp_path / "realign.sam").encode(), str(tmp_path / "kept.sam").encode()) == 0
    first = driver.arriba_workflow_sample(session, sample, str(tmp_path / "first.tsv").encode(), None, None, ctypes.byref(timing))
    message = driver.arriba_workflow_last_error().decode()
    written = sorted(os.listdir(str(tmp_path)))
    seconds = timing.realign
    timing = _capi.WorkflowTiming()
    second = driver.arriba_workflow_sample(session, sample, str(tmp_path / "second.tsv").encode(), None, None, ctypes.byref(timing))
    driver.arriba_workflow_close(session)
    assert first == second, message
    assert written[-2:] == ["kept.sam", "realign.sam"] and seconds > 0 and timing.realign == 0
    assert sorted(os.listdir(str(tmp_path))) == sorted(written + (["second.tsv"] if second == 0 else []))
    assert open(str(tmp_path / "realign.sam"), "rb").read() == _golden("hand_made.realign.sam") and open(str(tmp_path / "kept.sam"), "rb").read() == _golden("hand_made.kept.sam")
    if first == 0:
        assert open(str(tmp_path / "first.tsv"), "rb").read() == open(str(tmp_path / "second.tsv"), "rb").read()


# ---- GPU tier -----------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pipeline(committed_session, cases, tmp_path_factory):
    """one device pipeline on the committed assembly for every case that is ingested here"""
    sample = str(tmp_path_factory.mktemp("committed") / "hand_made.bam")
    lib.write_bgzf(sample, cases("hand_made")[0] + cases("hand_made")[1], 0)
    made = lib.stream_pipeline(committed_session, sample)
    yield made
    made.close()


def _set(knobs, monkeypatch):
    for knob in KNOBS:
        if knob in knobs:
            monkeypatch.setenv(knob, knobs[knob])
        else:
            monkeypatch.delenv(knob, raising=False)


def _device_split(pipeline, cases, name, tmp_path, want_kept=True):
    """the case through an ingest and agpu_realign_* -> (the bytes of the two files, the statistics)"""
    header, record_bytes, _, _ = cases(name)
    sample = str(tmp_path / (name + ".bam"))
    lib.write_bgzf(sample, header + record_bytes, 0)
    pipeline.read_chimeric_alignments(sample)
    os.remove(sample)
    paths = [str(tmp_path / (name + ".realign.sam")), str(tmp_path / (name + ".kept.sam"))]
    stats = pipeline.realign_split(paths[0], paths[1] if want_kept else None)
    texts = [open(path, "rb").read() if os.path.exists(path) else None for path in paths]
    assert not os.path.exists(paths[0] + ".tmp") and not os.path.exists(paths[1] + ".tmp") and pipeline.realign_allocated_bytes() == 0, name
    for path in paths:
        if os.path.exists(path):
            os.remove(path)
    return texts[0], texts[1], stats


DEVICE_KNOBS = {"no_knobs": {}, "lane_form": {"ARRIBA_REALIGN_TEXT_FORM": "lane"}, "window_64": {"ARRIBA_REALIGN_TEXT_WINDOW": "64"}, "window_64_lane_form": {"ARRIBA_REALIGN_TEXT_WINDOW": "64", "ARRIBA_REALIGN_TEXT_FORM": "lane"},
                "window_4096": {"ARRIBA_REALIGN_TEXT_WINDOW": "4096"}, "launch_256": {"ARRIBA_REALIGN_LAUNCH_ITEMS": "256", "ARRIBA_REALIGN_TEXT_WINDOW": "4096"}, "hash_bits_3": {"ARRIBA_REALIGN_HASH_BITS": "3"}}


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", sorted(DEVICE_KNOBS))
def test_device_files_are_the_host_files(knobs, built, pipeline, cases, host_side, tmp_path, monkeypatch):
    """the files of agpu_realign_* equal the host stepping byte for byte and the statistics are equal: the committed cases, ten seeded inputs, every made case; with either form of
    the text kernel, with windows of 64 bytes (smaller than a line) and 4096 bytes (lines straddle windows), with launches of 256 work-items and with a name hash of 3 bits"""
    _set(DEVICE_KNOBS[knobs], monkeypatch)
    names = COMMITTED + SEEDED[:10] + sorted(MADE)
    if knobs.startswith("window_64"):  # (a window per 64 bytes: the large cases would take thousands of launches)
        names = COMMITTED + SEEDED[:2] + ["templates65", "templates65_se", "long_name", "no_records", "header_only"]
    for name in names:
        realign, kept, stats = _device_split(pipeline, cases, name, tmp_path)
        expected_realign, expected_kept, expected = host_side(name)
        assert realign == expected_realign, name
        assert kept == expected_kept, name
        assert {key: stats[key] for key in COUNTED} == {key: expected[key] for key in COUNTED}, name
        assert stats["peak_bytes"] > 0, name
        if name in COMMITTED:
            assert realign == _golden(name + ".realign.sam") and kept == _golden(name + ".kept.sam")


@pytest.mark.gpu
def test_device_without_the_kept_file_and_the_order_of_the_calls(built, pipeline, cases, host_side, tmp_path, monkeypatch):
    """want_kept 0: the same file to realign and the same statistics, and no window of the other file; _end without _begin does nothing; _begin twice is refused; the buffers are
    gone after _end"""
    from arriba_amd import _capi
    _set({}, monkeypatch)
    for name in ("hand_made", "hand_made_se", "seed1801"):
        realign, kept, stats = _device_split(pipeline, cases, name, tmp_path, want_kept=False)
        assert realign == host_side(name)[0] and kept is None
        assert {key: stats[key] for key in COUNTED} == {key: host_side(name)[2][key] for key in COUNTED}
    api, ctx, host, handle = pipeline.api, pipeline.ctx, pipeline.session._lib, pipeline.session._session
    assert api.realign_end(ctx, None) == 0  # (without a begin)
    contigs, plan, info, got = _capi.DepthContigs(), _capi.RealignPlan(), _capi.RealignInfo(), ctypes.c_uint64()
    assert host.ahost_depth_contigs_of_session(handle, ctypes.byref(contigs)) == 0 and host.ahost_realign_plan_of_session(handle, ctypes.byref(plan)) == 0
    buffer = api.host_alloc(16 << 20)
    assert api.realign_next(ctx, 0, buffer, 16 << 20, ctypes.byref(got)) != 0 and b"agpu_realign_begin must run first" in api.last_error()
    assert api.realign_begin(ctx, plan.in_assembly, contigs.names, contigs.name_offset, contigs.n_ref + 1, 0, ctypes.byref(info)) != 0 and b"the references are not those of the header" in api.last_error()
    assert pipeline.realign_allocated_bytes() == 0
    assert api.realign_begin(ctx, plan.in_assembly, contigs.names, contigs.name_offset, contigs.n_ref, 0, ctypes.byref(info)) == 0, api.last_error()
    assert info.layout == 1 and info.realign_bytes == host_side("seed1801")[2]["realign_bytes"] and info.window_bytes == 16 << 20 and pipeline.realign_allocated_bytes() > 0
    assert api.realign_begin(ctx, plan.in_assembly, contigs.names, contigs.name_offset, contigs.n_ref, 0, ctypes.byref(info)) != 0 and b"agpu_realign_end must run first" in api.last_error()
    assert api.realign_next(ctx, 1, buffer, 16 << 20, ctypes.byref(got)) != 0 and b"the kept templates were not asked for" in api.last_error()
    assert api.realign_next(ctx, 0, buffer, 1024, ctypes.byref(got)) != 0 and b"smaller than a window" in api.last_error()
    assert api.realign_next(ctx, 0, buffer, 16 << 20, ctypes.byref(got)) == 0 and ctypes.string_at(buffer, got.value) == host_side("seed1801")[0]
    assert api.realign_next(ctx, 0, buffer, 16 << 20, ctypes.byref(got)) == 0 and got.value == 0
    stats = _capi.RealignStats()
    assert api.realign_end(ctx, ctypes.byref(stats)) == 0 and stats.templates == host_side("seed1801")[2]["templates"] and pipeline.realign_allocated_bytes() == 0
    api.host_free(buffer)


def _command_line(sample, outputs, extra):
    return subprocess.run(["timeout", "-k", "10", "120", WORKFLOW] + _arguments(sample, outputs, extra), stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)


@pytest.fixture(scope="module")
def without_the_option(tmp_path_factory):
    """fusions.tsv and discarded.tsv of the committed case from a run of the command line without the options"""
    directory = tmp_path_factory.mktemp("plain")
    outputs = [str(directory / "fusions.tsv"), str(directory / "discarded.tsv")]
    result = _command_line(os.path.join(GOLDEN, "hand_made.sam"), outputs, [])
    assert result.returncode == 0, result.stderr[-2000:]
    assert "Splitting reads" not in result.stdout
    return [open(path, "rb").read() for path in outputs]


@pytest.mark.gpu
@pytest.mark.parametrize("container", ["stored_bgzf", "sam_text", "host_ingest"])
def test_command_line_writes_the_files_next_to_the_fusions(container, built, cases, without_the_option, tmp_path):
    """the committed case as BAM and as SAM text, and with --host-ingest: the committed files, and the other outputs as without the options"""
    os.mkdir(str(tmp_path / "in")); os.mkdir(str(tmp_path / "out"))
    sample = str(tmp_path / "in" / "sample.bam")
    if container in ("sam_text", "host_ingest"):
        sample = os.path.join(GOLDEN, "hand_made.sam")
    else:
        lib.write_bgzf(sample, cases("hand_made")[0] + cases("hand_made")[1], 0)
    outputs = [str(tmp_path / "out" / "fusions.tsv"), str(tmp_path / "out" / "discarded.tsv")]
    result = _command_line(sample, outputs, ["--realign-reads", str(tmp_path / "out" / "realign.sam"), "--realign-kept", str(tmp_path / "out" / "kept.sam")] + (["--host-ingest"] if container == "host_ingest" else []))
    assert result.returncode == 0, result.stderr[-2000:]
    assert open(str(tmp_path / "out" / "realign.sam"), "rb").read() == _golden("hand_made.realign.sam") and open(str(tmp_path / "out" / "kept.sam"), "rb").read() == _golden("hand_made.kept.sam")
    assert HAND_MADE_LINE in result.stdout
    assert [open(path, "rb").read() for path in outputs] == without_the_option
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["discarded.tsv", "fusions.tsv", "kept.sam", "realign.sam"]


@pytest.mark.gpu
def test_session_and_the_off_switch(built, cases, without_the_option, tmp_path):
    """two samples in a queue, the second with the options: its files are the committed ones, the first writes none; with the options off no kernel whose name begins with realign
    is in the kernel profile and no buffer of it exists; the refusals of the driver that is linked with the device library come before the feed"""
    from arriba_amd.pipeline import ArribaError, DevicePipeline, HostSession, WorkflowSession
    sample = os.path.join(GOLDEN, "hand_made.sam")
    session = WorkflowSession(os.path.join(GOLDEN, "hand_made.fa"), os.path.join(GOLDEN, "hand_made.gtf"), interesting_contigs=lib.COMMITTED_CONTIGS, params={"disable_filters": ["blacklist"]})
    for directory in ("first", "second"):
        os.mkdir(str(tmp_path / directory))
    session.submit(sample)
    session.submit(sample, realign_reads_file=str(tmp_path / "second" / "realign.sam"), realign_kept_file=str(tmp_path / "second" / "kept.sam"))
    session.sample(sample, str(tmp_path / "first" / "fusions.tsv"))
    assert session.timing["realign"] == 0
    session.sample(sample, str(tmp_path / "second" / "fusions.tsv"))
    assert session.timing["realign"] > 0
    for context in session._lane_contexts():
        count = ctypes.c_uint64(1)
        assert session.api.realign_allocated_bytes(context, ctypes.byref(count)) == 0 and count.value == 0
    session.close()
    assert os.listdir(str(tmp_path / "first")) == ["fusions.tsv"] and sorted(os.listdir(str(tmp_path / "second"))) == ["fusions.tsv", "kept.sam", "realign.sam"]
    assert open(str(tmp_path / "second" / "realign.sam"), "rb").read() == _golden("hand_made.realign.sam") and open(str(tmp_path / "second" / "kept.sam"), "rb").read() == _golden("hand_made.kept.sam")
    for directory in ("first", "second"):
        assert open(str(tmp_path / directory / "fusions.tsv"), "rb").read() == without_the_option[0]
    # the off switch, and on through the stages of the pipeline
    made = DevicePipeline(HostSession(os.path.join(GOLDEN, "hand_made.fa"), os.path.join(GOLDEN, "hand_made.gtf"), interesting_contigs=lib.COMMITTED_CONTIGS), bam=sample)
    made.set_profiling(True)
    made.read_chimeric_alignments(sample)
    made.run_workflow(str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv"))
    assert made.kernel_profile() and not [launch for launch in made.kernel_profile() if launch[0].startswith("realign")] and made.realign_allocated_bytes() == 0
    made.read_chimeric_alignments(sample)
    with pytest.raises(ArribaError, match="--realign-kept needs --realign-reads"):
        made.run_workflow(str(tmp_path / "again.tsv"), None, realign_kept_file=str(tmp_path / "kept.sam"))
    made.read_chimeric_alignments(sample)
    made.run_workflow(str(tmp_path / "again.tsv"), None, realign_reads_file=str(tmp_path / "realign.sam"), realign_kept_file=str(tmp_path / "kept.sam"))
    assert {"realign_name_kernel", "realign_verdict_kernel", "realign_bound_kernel", "realign_text_kernel<wave>"} <= set(launch[0] for launch in made.kernel_profile())
    assert open(str(tmp_path / "realign.sam"), "rb").read() == _golden("hand_made.realign.sam") and open(str(tmp_path / "again.tsv")).read() == open(str(tmp_path / "fusions.tsv")).read()
    made.close()
    # the refusals of the command line on the device path
    outputs = [str(tmp_path / "refused" / "fusions.tsv"), str(tmp_path / "refused" / "discarded.tsv")]
    os.mkdir(str(tmp_path / "refused"))
    command = ["timeout", "-k", "10", "120", WORKFLOW] + _arguments(sample, outputs, [])
    _refused(command + ["--realign-kept", str(tmp_path / "refused" / "kept.sam")], tmp_path / "refused", "ERROR: --realign-kept needs --realign-reads")
    _refused(command + ["--realign-reads", outputs[1]], tmp_path / "refused", "ERROR: --realign-reads names a file that another option of the run names")
