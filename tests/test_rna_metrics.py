"""--rna-metrics: the alignment QC table of the records of -x -- records by flag, MAPQ, aligned bases per class of the annotation, strandedness, insert sizes, coverage of gene
bodies (the rule: DESIGN.md 4.19).

No program of the reference writes this file; the rule is the project's.  tests/golden/rna_metrics/hand_made.{fa,gtf,bed,sam,tsv} are a case with one or two records per line of
the rule, whose numbers test_restatement_equals_the_committed_file also writes out one by one; tests/rna_metrics_lib.py restates the rule in plain Python base by base, is held to
that case, and only therefore is the independent side for inputs made at test time.  The CPU tier runs arriba_amd/csrc/device/rnametrics_core.hpp stepped on the host against the
region track of arriba_amd/csrc/host/region_track.cpp (ahost_rna_metrics_*, ahost_region_track); the GPU tier the kernel of agpu_rnametrics.hip, whose file must equal the host's
byte for byte and whose statistics must equal the host's."""
import ctypes
import gzip
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import conftest
import rna_metrics_lib as lib

sys.path.insert(0, os.path.join(conftest.ROOT, "tools"))

GOLDEN = lib.GOLDEN
WORKFLOW = os.path.join(conftest.ROOT, "arriba_amd", "lib", "arriba_gpu_workflow")
ANNOTATION_SEEDS = (1900, 1901, 1902, 1903, 1904)
SEEDED = ["seed%d" % (1900 + k) for k in range(50)]  # input 1900 + k lies on the annotation of seed 1900 + k % 5
MADE = ["wavefront", "workgroup", "hot", "long_cigar", "empty", "no_records"]  # on the annotation of seed 1900
COUNTED = ("records", "base_records", "blocks")  # what the device, the host and the restatement must agree on
COUNTED_BY_BOTH = COUNTED + ("segments", "track_runs")  # ... and the device and the host


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


def _annotation_of(name):
    return "hand_made" if name == "hand_made" else 1900 + int(name[4:]) % 5 if name.startswith("seed") else 1900


@pytest.fixture(scope="module")
def annotations(tmp_path_factory):
    """key ("hand_made" or a seed) -> (prefix of .fa / .gtf / .bed, the annotation as the restatement reads it, its bases one by one): made once"""
    cache, directory = {}, str(tmp_path_factory.mktemp("annotations"))

    def get(key):
        if key not in cache:
            prefix = os.path.join(GOLDEN, "hand_made") if key == "hand_made" else lib.write_seeded_annotation(key, directory)
            annotation = lib.load_annotation(prefix + ".gtf", prefix + ".fa", prefix + ".bed")
            cache[key] = (prefix, annotation, lib.per_position(annotation))
        return cache[key]
    return get


@pytest.fixture(scope="module")
def cases(annotations):
    """name -> (BAM header, record bytes, (text, stats, counters) of the restatement, the case): made once and left unchanged"""
    cache = {}

    def get(name):
        if name not in cache:
            _, annotation, bases = annotations(_annotation_of(name))
            if name == "hand_made":
                case = lib.parse_sam(_golden("hand_made.sam"))
            elif name.startswith("seed"):
                case = lib.random_case(int(name[4:]), annotation)
            else:
                case = {"wavefront": lambda a: lib.spread_case(a, 65), "workgroup": lambda a: lib.spread_case(a, 257), "hot": lib.hot_case, "long_cigar": lib.long_cigar_case, "empty": lib.empty_case,
                        "no_records": lib.no_records_case}[name](annotation)
            cache[name] = (lib.bam_header(case[0]), lib.bam_records(case), lib.restate(annotation, case, bases), case)
        return cache[name]
    return get


# ---- the host side ------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sessions(built, annotations):
    """key of an annotation -> a host session on it"""
    from arriba_amd.pipeline import HostSession
    cache = {}

    def get(key):
        if key not in cache:
            prefix, annotation, _ = annotations(key)
            cache[key] = HostSession(prefix + ".fa", prefix + ".gtf", interesting_contigs=" ".join(sorted(annotation["lengths"])))
        return cache[key]
    yield get
    for session in cache.values():
        session.close()


def _stats():
    from arriba_amd import _capi
    return _capi.RnaMetricsStats()


def _text_of(host, counters):
    text, size = ctypes.c_void_p(), ctypes.c_uint64()
    assert host.ahost_rna_metrics_text(counters.ctypes.data, counters.size, ctypes.byref(text), ctypes.byref(size)) == 0, host.ahost_last_error()
    return ctypes.string_at(text, size.value)


def _host_metrics(session, bed, header, record_bytes):
    """-> (text, statistics, counters) of ahost_rna_metrics_of + ahost_rna_metrics_text"""
    from arriba_amd import _capi
    from arriba_amd.pipeline import rna_metrics_stats_of
    host, handle = session._lib, session._session
    counters, stats = np.zeros(_capi.RNA_METRICS_WORDS, dtype=np.uint64), _stats()
    assert host.ahost_rna_metrics_of(handle, bed.encode() if bed else None, header, len(header), record_bytes, len(record_bytes), counters.ctypes.data, counters.size, ctypes.byref(stats)) == 0, host.ahost_last_error()
    return _text_of(host, counters), rna_metrics_stats_of(stats), counters


@pytest.fixture(scope="module")
def host_side(cases, sessions, annotations):
    """name -> what the host stepping gives: computed once, compared against by every test"""
    cache = {}

    def get(name):
        if name not in cache:
            key = _annotation_of(name)
            cache[name] = _host_metrics(sessions(key), annotations(key)[0] + ".bed", *cases(name)[:2])
        return cache[name]
    return get


@pytest.fixture(scope="module")
def toy3k(dataset_files, tmp_path_factory):
    """(prefix, uncompressed BAM stream, SAM text, an interval file) of the dataset"""
    from bam_to_sam import bam_to_sam
    prefix = dataset_files("toy3k")
    bed = str(tmp_path_factory.mktemp("toy3k_bed") / "rrna.bed")
    open(bed, "w").write("# made for the test\n1\t1000\t60000\tone\nchr2\t0\t25000\nMT\t0\t16000\n")
    return prefix, gzip.open(prefix + ".bam", "rb").read(), bam_to_sam(open(prefix + ".bam", "rb").read())[0], bed


@pytest.fixture(scope="module")
def toy3k_host(toy3k):
    """(text, statistics) of the host stepping on toy3k, against toy3k's own annotation"""
    from arriba_amd.pipeline import HostSession
    prefix = toy3k[0]
    session = HostSession(prefix + ".fa", prefix + ".gtf", interesting_contigs="1 2 3 4")
    result = _host_metrics(session, toy3k[3], *_split(toy3k[1]))
    session.close()
    return result[:2]


# ---- CPU tier -----------------------------------------------------------------------------------------------------------------------------------------------------

def test_restatement_equals_the_committed_file(annotations):
    """the base-by-base restatement of the rule against the committed case; the numbers a reader works out from the comments of hand_made.sam are written out here"""
    _, annotation, bases = annotations("hand_made")
    case = lib.parse_sam(_golden("hand_made.sam"))
    text, stats, counters = lib.restate(annotation, case, bases)
    assert text == _golden("hand_made.tsv")
    assert stats == {"records": 33, "base_records": 27, "blocks": 29}
    assert [name for name, _ in case[0]] == ["r1", "r2", "orphan"] and set(annotation["lengths"]) == {"r1", "r2"} and annotation["unknown_intervals"] == 1 and annotation["intervals"] == 3
    assert all(len(_golden("hand_made." + kind)) < 100000 for kind in ("fa", "gtf", "bed", "sam", "tsv"))
    n = lib.check_invariants(text)
    # kinds and flags
    assert (n["SECONDARY"], n["SUPPLEMENTARY"], n["PRIMARY"], n["UNMAPPED"], n["MAPPED"]) == (2, 1, 30, 2, 28)  # s1 and s3; s2; u1 and the mate of p5
    assert (n["QC_FAIL"], n["DUPLICATE"], n["MULTIMAPPING"], n["READ2"], n["MATE_UNMAPPED"], n["MATE_OTHER_CONTIG"]) == (1, 1, 1, 1, 1, 1)
    # twelve base records lie on 100-149 (UTR of GA: 600); a1, a2, a9 10 each; a3 and a12 20 each
    assert n["UTR_BASES"] == 600 + 30 + 40
    # rRNA: a1 160-179, a2 160-169, a13 1100-1129, and the last base of p3 (1051-1100)
    assert n["RIBOSOMAL_BASES"] == 20 + 10 + 30 + 1
    # coding: a1 10 + 20 + 40, a2 10 + 40, a4 20, a5 50, a6 30, a10 40
    assert n["CODING_BASES"] == 70 + 50 + 20 + 50 + 30 + 40
    assert n["INTRONIC_BASES"] == 100 + 30 and n["UNKNOWN_CONTIG_BASES"] == 25  # a1 and a11; a8
    # intergenic: a3 650-669, a7 390-399 (clipped at LN 400), p1's second mate 1050-1099, p3 1051-1099
    assert n["INTERGENIC_BASES"] == 20 + 10 + 50 + 49
    assert (n["INSERTED_BASES"], n["DELETED_BASES"], n["SOFT_CLIPPED_BASES"], n["SKIPPED_BASES"], n["SPLICED_RECORDS"]) == (2, 10, 10, 130, 1)
    assert (n["ANTISENSE_STRAND_RECORDS"], n["AMBIGUOUS_STRAND_RECORDS"], n["NO_GENE_RECORDS"]) == (1, 1, 5)  # a12; a4; a7, a8, a13, p1's second mate, p3
    assert counters["INSERT_SIZE"] == {150: 2, 1000: 2, 1001: 3} and b"\nMEDIAN_INSERT_SIZE\t1000\n" in text  # 1001, -1001 and INT32_MIN share the last bin
    assert counters["MAPQ"] == {0: 1, 3: 1, 60: 25, 255: 1}
    body = counters["GENE_BODY"]
    # a6 alone reaches bins 25-29 of GD (t 25-29) ... together with the reverse gene GB (a3: t 19-0) and the twelve reads on GA's first 50 exonic bases (t 0-49 of L 200: bins 0-24, 2 each)
    assert body[75:] == [0] * 25 and body[25:30] == [1 + 4] * 5  # a6: 1; a1 (t 40-139 of 200: bins 20-69, 2 each) and a2 (t 40-69: bins 20-34): 2 + 2
    assert body[70:75] == [2] * 5 and body[65:70] == [2 + 2 + 2] * 5  # a10's first block alone: t 149-130 of L 200; bins 65-69 also hold a1 and a2's second block (t 100-139: bins 50-69)
    assert body[0:5] == [24 + 1 + 1] * 5  # the twelve reads on GA (2 each), a3 on GB (bins 0-19) and a6 on GD


def test_host_gives_the_committed_bytes(built, cases, host_side, sessions, tmp_path):
    text, stats, _ = host_side("hand_made")
    assert text == _golden("hand_made.tsv")
    assert {key: stats[key] for key in COUNTED} == cases("hand_made")[2][1]
    # ... and through the project's own reader of SAM text
    session = sessions("hand_made")
    path, counted = str(tmp_path / "metrics.tsv"), _stats()
    host = session._lib
    assert host.ahost_rna_metrics_file(session._session, os.path.join(GOLDEN, "hand_made.sam").encode(), os.path.join(GOLDEN, "hand_made.bed").encode(), path.encode(), ctypes.byref(counted)) == 0, host.ahost_last_error()
    assert open(path, "rb").read() == text and counted.blocks == 29 and os.listdir(str(tmp_path)) == ["metrics.tsv"]
    # without the interval file the ribosomal bases fall to what lies under them
    plain, _, counters = _host_metrics(session, None, *cases("hand_made")[:2])
    n = lib.check_invariants(plain)
    assert n["RIBOSOMAL_BASES"] == 0 and n["CODING_BASES"] == 260 + 30 and n["INTERGENIC_BASES"] == 129 + 31


@pytest.mark.parametrize("name", ["seeded"] + MADE)
def test_host_equals_the_restatement(name, built, cases, host_side):
    totals = None
    for case in (SEEDED if name == "seeded" else [name]):
        text, stats, counters = host_side(case)
        expected_text, expected, _, records = cases(case)[2] + (cases(case)[3][1],)
        assert text == expected_text, case
        assert {key: stats[key] for key in COUNTED} == expected, case
        n = lib.check_invariants(text)
        assert n["RECORDS"] == len(records) <= 20000
        totals = counters.copy() if totals is None else totals + counters
    n = dict(zip(lib.SCALARS, (int(x) for x in totals)))
    if name == "seeded":  # the seeded set as a whole exercises the rule
        assert all(n[key] > 0 for key in lib.SCALARS), n
        assert (totals[36:36 + 256] > 0).sum() > 50 and (totals[36 + 256:36 + 256 + 1002] > 0).sum() > 100 and totals[36 + 256 + 1001] > 0 and (totals[-100:] > 0).all()
    if name == "wavefront":
        assert n["RECORDS"] == 65
    if name == "workgroup":
        assert n["RECORDS"] == 257
    if name == "hot":
        assert n["RECORDS"] == n["INSERT_SIZE_PAIRS"] == n["SPLICED_RECORDS"] == 20000 and n["ALIGNED_BASES"] == 20000 * 50 and totals[36 + 37] == 20000 and totals[36 + 256 + 321] == 20000 and totals[-100:].sum() >= 20000 * 25
    if name == "long_cigar":
        assert stats["blocks"] >= 250 and stats["segments"] >= stats["blocks"] + 300 and n["SKIPPED_BASES"] > 0 and n["DELETED_BASES"] > 0  # (touching blocks are one block)
    if name == "empty":
        assert n["PRIMARY"] == 0 and n["SECONDARY"] == n["SUPPLEMENTARY"] == 1 and totals[3:].sum() == 0
    if name == "no_records":
        assert totals.sum() == 0 and len(text.split(b"\n")) == 1 + 34 + 10 + 3 + 100 + 1 and b"\nMEDIAN_INSERT_SIZE\tNA\nPCT_RIBOSOMAL_BASES\tNA\n" in text


@pytest.mark.parametrize("key", ("hand_made",) + ANNOTATION_SEEDS)
def test_region_track_equals_the_bases_one_by_one(key, built, sessions, annotations):
    """the runs of the track decoded back to bits, body gene and offset per base, against the restatement's sets; and what the reader of the interval file counts"""
    from arriba_amd import _capi
    prefix, annotation, bases = annotations(key)
    session = sessions(key)
    host, handle = session._lib, session._session
    track, info = _capi.RegionTrack(), _capi.RegionTrackInfo()
    assert host.ahost_region_track(handle, (prefix + ".bed").encode(), ctypes.byref(track), ctypes.byref(info)) == 0, host.ahost_last_error()
    assert track.id != 0 and info.runs == track.n_runs and info.intervals == annotation["intervals"] and info.intervals_unknown_contig == annotation["unknown_intervals"] > 0

    def array(pointer, count, kind):
        return np.ctypeslib.as_array(ctypes.cast(pointer, ctypes.POINTER(kind)), shape=(max(int(count), 1),))[:int(count)].copy()
    arrays = (array(track.contig_offset, track.n_contigs + 1, ctypes.c_uint32), array(track.run_start, track.n_runs, ctypes.c_int32), array(track.run_bits, track.n_runs, ctypes.c_uint8),
              array(track.run_gene, track.n_runs, ctypes.c_uint32), array(track.run_rank, track.n_runs, ctypes.c_uint32), array(track.gene_body, track.n_genes, ctypes.c_uint32))
    host.ahost_contig_name.restype = ctypes.c_char_p
    contig_index = {host.ahost_contig_name(handle, c).decode(): c for c in range(track.n_contigs)}
    assert set(contig_index) == set(annotation["lengths"]) and track.n_genes == len(annotation["genes"])
    decoded = lib.decode_track(arrays, annotation, contig_index)
    for name in annotation["lengths"]:
        assert decoded[name]["bits"] == bases[name]["bits"], name
        theirs = {p: (annotation["genes"][gene], t, length) for p, (gene, t, length) in decoded[name]["body"].items()}
        assert theirs == bases[name]["body"], name
    if key != "hand_made":
        assert track.n_runs > 600 and sum(len(bases[name]["body"]) for name in bases) > 1000
    # the same track again: built once per session and interval file
    again = _capi.RegionTrack()
    assert host.ahost_region_track(handle, (prefix + ".bed").encode(), ctypes.byref(again), None) == 0 and again.id == track.id and again.run_start == track.run_start
    assert host.ahost_region_track(handle, None, ctypes.byref(again), None) == 0 and again.id != track.id


def test_the_file_interface(built, toy3k, toy3k_host, tmp_path):
    """ahost_rna_metrics_file reads BAM and SAM text itself and leaves no temporary file"""
    from arriba_amd.pipeline import HostSession
    prefix, stream, text, bed = toy3k
    session = HostSession(prefix + ".fa", prefix + ".gtf", interesting_contigs="1 2 3 4")
    host, handle = session._lib, session._session
    open(str(tmp_path / "sample.sam"), "wb").write(text)
    expected, expected_stats = toy3k_host
    n = lib.check_invariants(expected)
    assert n["RIBOSOMAL_BASES"] > 0 and n["CODING_BASES"] + n["UTR_BASES"] > 0 and expected_stats["blocks"] > 1000  # (the generator writes TLEN 0: no insert sizes here)
    for source in (prefix + ".bam", str(tmp_path / "sample.sam")):
        path, stats = str(tmp_path / "metrics.tsv"), _stats()
        assert host.ahost_rna_metrics_file(handle, source.encode(), bed.encode(), path.encode(), ctypes.byref(stats)) == 0, host.ahost_last_error()
        assert open(path, "rb").read() == expected and stats.blocks == expected_stats["blocks"]
        os.remove(path)
    assert host.ahost_rna_metrics_file(handle, (prefix + ".bam").encode(), bed.encode(), str(tmp_path / "missing" / "metrics.tsv").encode(), None) != 0
    session.close()
    assert sorted(os.listdir(str(tmp_path))) == ["sample.sam"]


MALFORMED = {"two_fields": "1\t100\n", "no_digit": "1\t1x\t20\n", "negative": "1\t-5\t20\n", "start_behind_end": "1\t10\t20\n2\t30\t29\n", "empty_end": "1\t5\t\n", "too_large": "1\t5\t4294967296\n", "empty_contig": "\t5\t6\n"}


@pytest.mark.parametrize("kind", sorted(MALFORMED))
def test_a_malformed_interval_file_is_refused_with_its_line(kind, built, tmp_path):
    from arriba_amd import _capi
    host = _capi.host_library()
    path = str(tmp_path / "rrna.bed")
    open(path, "w").write("# a comment\n" + MALFORMED[kind])
    assert host.ahost_rrna_intervals_load(path.encode(), None) != 0
    message = host.ahost_last_error().decode()
    assert "--rrna-intervals: '%s' line %d: " % (path, 3 if kind == "start_behind_end" else 2) in message
    count = ctypes.c_uint64()
    open(path, "w").write("track name=x\nbrowser hide all\n\n# c\n1\t5\t5\n1\t0\t7\tname\t0\t-\r\n")
    assert host.ahost_rrna_intervals_load(path.encode(), ctypes.byref(count)) == 0 and count.value == 2
    assert host.ahost_rrna_intervals_load(str(tmp_path).encode(), None) != 0 and "cannot read" in host.ahost_last_error().decode()


def _harness(target):
    directory = os.path.join(conftest.ROOT, "tests", "emu")
    subprocess.run(["make", "-s", "-C", directory, target], check=True)
    return os.path.join(directory, target)


def _run(command, timeout=300):
    return subprocess.run(command, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=timeout)


def test_host_ingest_through_the_command_line(built, emu_api, toy3k, toy3k_host, tmp_path):
    """--host-ingest --rna-metrics: the C++ driver (over the host stepping harness, where there is no GPU) writes the table of the host stepping, and fusions.tsv is the golden one"""
    prefix, bed = toy3k[0], toy3k[3]
    command = [_harness("workflow_on_harness"), "-x", prefix + ".bam", "-g", prefix + ".gtf", "-a", prefix + ".fa", "-o", str(tmp_path / "fusions.tsv"), "-f", "blacklist", "--host-ingest",
               "--rna-metrics", str(tmp_path / "metrics.tsv"), "--rrna-intervals", bed]
    result = _run(command)
    assert result.returncode == 0, result.stderr[-2000:]
    assert open(str(tmp_path / "metrics.tsv"), "rb").read() == toy3k_host[0]
    assert not os.path.exists(str(tmp_path / "metrics.tsv.tmp"))
    assert "Collecting RNA-seq metrics (records=%d, " % toy3k_host[1]["records"] in result.stdout
    assert open(str(tmp_path / "fusions.tsv")).read() == gzip.open(os.path.join(conftest.golden_dir("toy3k"), "fusions.tsv.gz"), "rt").read()
    # a malformed interval file is refused before the input is read
    open(str(tmp_path / "bad.bed"), "w").write("1\t9\t3\n")
    os.remove(str(tmp_path / "metrics.tsv")); os.remove(str(tmp_path / "fusions.tsv"))
    result = _run(command[:-1] + [str(tmp_path / "bad.bed")])
    assert result.returncode != 0 and "line 1: the start lies behind the end" in result.stderr and "Reading chimeric alignments" not in result.stdout
    assert sorted(os.listdir(str(tmp_path))) == ["bad.bed"]


def test_refusals_at_the_command_line(built, toy3k, tmp_path):
    prefix, bed = toy3k[0], toy3k[3]
    command = [WORKFLOW, "-x", prefix + ".bam", "-g", prefix + ".gtf", "-a", prefix + ".fa", "-o", str(tmp_path / "fusions.tsv"), "-f", "blacklist"]
    result = _run(command + ["--rna-metrics", str(tmp_path / "missing" / "metrics.tsv")], 60)
    assert result.returncode == 1 and "parent directory of output file" in result.stderr and "metrics.tsv" in result.stderr
    result = _run(command + ["--rna-metrics", str(tmp_path / "metrics.tsv"), "--rrna-intervals", str(tmp_path / "none.bed")], 60)
    assert result.returncode == 1 and "file not found/readable" in result.stderr and "none.bed" in result.stderr
    result = _run(command + ["--rrna-intervals", bed], 60)
    assert result.returncode == 1 and "--rrna-intervals needs --rna-metrics" in result.stderr
    assert os.listdir(str(tmp_path)) == []
    usage = _run([WORKFLOW, "-h"], 60).stdout
    assert "--rna-metrics FILE [--rrna-intervals FILE.bed]" in usage


def test_cpp_driver_on_the_harness_says_that_it_has_no_device_library(built, emu_api, toy3k, tmp_path):
    """the test-only build of the C++ driver against the host stepping harness has no twin of the kernel of agpu_rnametrics.hip: it links all the same and says so before the feed"""
    prefix = toy3k[0]
    command = [_harness("workflow_on_harness"), "-x", prefix + ".bam", "-g", prefix + ".gtf", "-a", prefix + ".fa", "-o", str(tmp_path / "fusions.tsv"), "-f", "blacklist", "--rna-metrics", str(tmp_path / "metrics.tsv")]
    result = _run(command)
    assert result.returncode != 0 and "--rna-metrics needs the device library (agpu_rna_metrics)" in result.stderr
    assert not os.path.exists(str(tmp_path / "metrics.tsv")) and not os.path.exists(str(tmp_path / "metrics.tsv.tmp"))


def _driver_session(prefix):
    from arriba_amd import _capi
    driver = ctypes.CDLL(_harness("libworkflow_on_harness.so"))
    driver.arriba_workflow_open.restype = ctypes.c_void_p
    driver.arriba_workflow_last_error.restype = ctypes.c_char_p
    driver.arriba_workflow_rna_metrics.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p]
    options = _capi.WorkflowOptions()
    driver.arriba_workflow_default_options(ctypes.byref(options))
    options.assembly_file, options.gene_annotation_file = (prefix + ".fa").encode(), (prefix + ".gtf").encode()
    session = ctypes.c_void_p(driver.arriba_workflow_open(ctypes.byref(options)))
    assert session, driver.arriba_workflow_last_error()
    return driver, session


def test_a_sample_over_ranks_is_refused_before_the_feed(built, emu_api, toy3k, tmp_path):
    """one sample over several ranks: refused before a byte of the file is fed (the driver over the harness, a communicator of one rank that does nothing); and the interval file
    without the table"""
    from arriba_amd import _capi
    prefix, bed = toy3k[0], toy3k[3]
    driver, session = _driver_session(prefix)
    assert driver.arriba_workflow_rna_metrics(session, None, bed.encode()) == 0
    status = driver.arriba_workflow_sample(session, (prefix + ".bam").encode(), str(tmp_path / "fusions.tsv").encode(), None, None, None)
    assert status != 0 and "ERROR: --rrna-intervals needs --rna-metrics" in driver.arriba_workflow_last_error().decode()
    nothing = lambda *arguments: 0  # noqa: E731
    communicator = _capi.WorkflowCommunicator(0, 1, None, _capi.ALL_GATHER(nothing), _capi.ALL_REDUCE_INT64(nothing), _capi.ALL_REDUCE_MAX_BYTES(nothing), None)
    assert driver.arriba_workflow_set_communicator(session, ctypes.byref(communicator)) == 0
    assert driver.arriba_workflow_rna_metrics(session, str(tmp_path / "metrics.tsv").encode(), None) == 0
    status = driver.arriba_workflow_sample(session, (prefix + ".bam").encode(), str(tmp_path / "fusions.tsv").encode(), None, None, None)
    message = driver.arriba_workflow_last_error().decode()
    driver.arriba_workflow_close(session)
    assert status != 0 and "ERROR: rna metrics of one sample over several GPUs are not supported" in message
    assert os.listdir(str(tmp_path)) == []


# ---- GPU tier -----------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pipelines(sessions, cases, tmp_path_factory):
    """key of an annotation -> one device pipeline on it for every case that is ingested here"""
    cache, directory = {}, tmp_path_factory.mktemp("pipelines")

    def get(key):
        if key not in cache:
            sample = str(directory / ("first_%s.bam" % key))
            first = cases("hand_made" if key == "hand_made" else "seed%d" % key)
            lib.write_bgzf(sample, first[0] + first[1], 0)
            cache[key] = lib.stream_pipeline(sessions(key), sample)
        return cache[key]
    yield get
    for made in cache.values():
        made.close()


@pytest.fixture(scope="module")
def toy3k_pipeline(toy3k):
    from arriba_amd.pipeline import DevicePipeline, HostSession
    prefix = toy3k[0]
    made = DevicePipeline(HostSession(prefix + ".fa", prefix + ".gtf", interesting_contigs="1 2 3 4"), bam=prefix + ".bam")
    yield made
    made.close()


KNOBS = [{}, {"ARRIBA_INGEST_WINDOWS": "1048576,65536"}, {"ARRIBA_RNAMETRICS_PLAIN_ATOMICS": "1"}]


def _set(knobs, monkeypatch):
    for knob in ("ARRIBA_INGEST_WINDOWS", "ARRIBA_RNAMETRICS_PLAIN_ATOMICS"):
        if knob in knobs:
            monkeypatch.setenv(knob, knobs[knob])
        else:
            monkeypatch.delenv(knob, raising=False)


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["committed_and_made", "seeded"])
@pytest.mark.parametrize("knobs", KNOBS, ids=["no_knobs", "ingest_windows", "plain_atomics"])
def test_device_file_is_the_host_file(knobs, group, built, pipelines, annotations, cases, host_side, tmp_path, monkeypatch):
    """the file of agpu_rna_metrics equals the host stepping byte for byte and the statistics are equal: the committed case, 65 and 257 records, 20 000 identical records, the
    601-operation CIGAR, records of which none is primary, a header without a record; 50 seeded inputs on five seeded annotations; with the ingest cut into windows; with global
    atomics per lane in place of the LDS stage"""
    _set(knobs, monkeypatch)
    for name in (["hand_made"] + MADE if group == "committed_and_made" else SEEDED):
        key = _annotation_of(name)
        pipeline, bed = pipelines(key), annotations(key)[0] + ".bed"
        header, record_bytes = cases(name)[:2]
        sample = str(tmp_path / (name + ".bam"))
        lib.write_bgzf(sample, header + record_bytes, 0)
        pipeline.read_chimeric_alignments(sample)
        os.remove(sample)
        path = str(tmp_path / (name + ".tsv"))
        stats = pipeline.write_rna_metrics(path, bed)
        text, expected, _ = host_side(name)
        print(name, stats)
        assert open(path, "rb").read() == text and not os.path.exists(path + ".tmp"), name
        assert {key: stats[key] for key in COUNTED_BY_BOTH} == {key: expected[key] for key in COUNTED_BY_BOTH}, name
        assert stats["peak_bytes"] >= pipeline.rna_metrics_allocated_bytes() > 0, name  # (the track stays; the counter block and the lengths have gone)
        lib.check_invariants(text)
        if name == "hand_made":
            assert text == _golden("hand_made.tsv")


@pytest.mark.gpu
@pytest.mark.parametrize("knobs", KNOBS, ids=["no_knobs", "ingest_windows", "plain_atomics"])
def test_device_equals_host_on_toy3k(knobs, built, toy3k, toy3k_pipeline, toy3k_host, tmp_path, monkeypatch):
    _set(knobs, monkeypatch)
    toy3k_pipeline.read_chimeric_alignments(toy3k[0] + ".bam")
    path = str(tmp_path / "metrics.tsv")
    stats = toy3k_pipeline.write_rna_metrics(path, toy3k[3])
    text, expected = toy3k_host
    assert open(path, "rb").read() == text and os.listdir(str(tmp_path)) == ["metrics.tsv"]
    assert {key: stats[key] for key in COUNTED_BY_BOTH} == {key: expected[key] for key in COUNTED_BY_BOTH}
    lib.check_invariants(text)


@pytest.fixture(scope="module")
def without_the_option(toy3k, tmp_path_factory):
    """fusions.tsv and discarded.tsv of toy3k from a run of the command line without --rna-metrics"""
    directory = tmp_path_factory.mktemp("plain")
    outputs = [str(directory / "fusions.tsv"), str(directory / "discarded.tsv")]
    result = _command_line(toy3k[0] + ".bam", toy3k[0], outputs, [])
    assert result.returncode == 0, result.stderr[-2000:]
    assert "Collecting RNA-seq metrics" not in result.stdout
    return [open(path, "rb").read() for path in outputs]


def _command_line(sample, prefix, outputs, extra):
    command = [WORKFLOW, "-x", sample, "-g", prefix + ".gtf", "-a", prefix + ".fa", "-o", outputs[0], "-O", outputs[1], "-f", "blacklist"]
    return subprocess.run(["timeout", "-k", "10", "120"] + command + extra, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)


@pytest.mark.gpu
@pytest.mark.parametrize("container", ["stored_bgzf", "deflated_bgzf", "sam_text"])
def test_command_line_writes_the_table_next_to_the_fusions(container, built, toy3k, toy3k_host, without_the_option, tmp_path):
    prefix, stream, text, bed = toy3k
    os.mkdir(str(tmp_path / "in")); os.mkdir(str(tmp_path / "out"))
    sample = str(tmp_path / "in" / "sample.bam")
    if container == "sam_text":
        open(sample, "wb").write(text)
    else:
        lib.write_bgzf(sample, stream, 0 if container == "stored_bgzf" else 6)
    outputs = [str(tmp_path / "out" / "fusions.tsv"), str(tmp_path / "out" / "discarded.tsv")]
    result = _command_line(sample, prefix, outputs, ["--rna-metrics", str(tmp_path / "out" / "metrics.tsv"), "--rrna-intervals", bed])
    assert result.returncode == 0, result.stderr[-2000:]
    assert open(str(tmp_path / "out" / "metrics.tsv"), "rb").read() == toy3k_host[0]
    assert "Collecting RNA-seq metrics (records=%d, " % toy3k_host[1]["records"] in result.stdout
    assert [open(path, "rb").read() for path in outputs] == without_the_option
    assert sorted(os.listdir(str(tmp_path / "out"))) == ["discarded.tsv", "fusions.tsv", "metrics.tsv"]


@pytest.mark.gpu
def test_session_writes_the_table_of_the_sample_that_asked_for_it(built, toy3k, toy3k_host, without_the_option, tmp_path):
    """two samples in one session, the option on the first only: the second leaves no file"""
    from arriba_amd.pipeline import WorkflowSession
    prefix, bed = toy3k[0], toy3k[3]
    session = WorkflowSession(prefix + ".fa", prefix + ".gtf", params={"disable_filters": ["blacklist"]})
    os.mkdir(str(tmp_path / "first")); os.mkdir(str(tmp_path / "second"))
    session.submit(prefix + ".bam", rna_metrics_file=str(tmp_path / "first" / "metrics.tsv"), rrna_intervals_file=bed)
    session.submit(prefix + ".bam")
    session.sample(prefix + ".bam", str(tmp_path / "first" / "fusions.tsv"))
    assert session.timing["rna_metrics"] > 0
    session.sample(prefix + ".bam", str(tmp_path / "second" / "fusions.tsv"))
    assert session.timing["rna_metrics"] == 0
    allocated = []
    for context in session._lane_contexts():
        count = ctypes.c_uint64(1)
        assert session.api.rna_metrics_allocated_bytes(context, ctypes.byref(count)) == 0
        allocated.append(count.value)
    session.close()
    assert sorted(allocated)[0] == 0 or len(allocated) == 1  # (only the lane that ran the option keeps a track)
    assert sorted(os.listdir(str(tmp_path / "first"))) == ["fusions.tsv", "metrics.tsv"] and os.listdir(str(tmp_path / "second")) == ["fusions.tsv"]
    assert open(str(tmp_path / "first" / "metrics.tsv"), "rb").read() == toy3k_host[0]
    for directory in ("first", "second"):
        assert open(str(tmp_path / directory / "fusions.tsv"), "rb").read() == without_the_option[0]


@pytest.mark.gpu
def test_refusals_and_the_off_switch(built, toy3k, toy3k_host, tmp_path, monkeypatch):
    """with the option off no kernel whose name begins with rnametrics is in the kernel profile and no buffer of it exists; before an ingest, for a part of a sample and when the
    stream was given back agpu_rna_metrics is refused with a message"""
    from arriba_amd import _capi
    from arriba_amd.pipeline import ArribaError, DevicePipeline, HostSession
    prefix, bed = toy3k[0], toy3k[3]
    made = DevicePipeline(HostSession(prefix + ".fa", prefix + ".gtf"), bam=prefix + ".bam")
    api, params = made.api, _capi.Params()
    api.default_params(ctypes.byref(params))
    fresh = api.create(0, ctypes.byref(params))
    assert fresh, api.last_error()
    track, room = _capi.RegionTrack(), np.zeros(_capi.RNA_METRICS_WORDS, dtype=np.uint64)
    assert made.session._lib.ahost_region_track(made.session._session, None, ctypes.byref(track), None) == 0
    refused = api.rna_metrics(fresh, ctypes.byref(track), None, 0, room.ctypes.data, None)  # before an ingest
    message = api.last_error()
    api.destroy(fresh)
    assert refused != 0 and b"agpu_rna_metrics: the record stream of the last ingest is not on the device any more" in message
    made.set_profiling(True)
    made.read_chimeric_alignments(prefix + ".bam")
    made.run_workflow(str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv"))
    assert made.kernel_profile() and not [launch for launch in made.kernel_profile() if launch[0].startswith("rnametrics")] and made.rna_metrics_allocated_bytes() == 0
    # ... and on, through the stages of the pipeline
    made.read_chimeric_alignments(prefix + ".bam")
    made.run_workflow(str(tmp_path / "again.tsv"), None, rna_metrics_file=str(tmp_path / "metrics.tsv"), rrna_intervals_file=bed)
    assert "rnametrics_record_kernel" in set(launch[0] for launch in made.kernel_profile())
    assert open(str(tmp_path / "metrics.tsv"), "rb").read() == toy3k_host[0] and open(str(tmp_path / "again.tsv")).read() == open(str(tmp_path / "fusions.tsv")).read()
    with pytest.raises(ArribaError, match="--rrna-intervals needs --rna-metrics"):
        made.run_workflow(str(tmp_path / "never.tsv"), None, rrna_intervals_file=bed)
    # a part of a sample
    made._ingest_records(prefix + ".bam", False, 100, 64 << 20, part=0, parts=2)
    with pytest.raises(ArribaError, match="rna metrics of one sample over several GPUs are not supported"):
        made.write_rna_metrics(str(tmp_path / "part.tsv"))
    # the stream was given back behind the ingest
    monkeypatch.setenv("ARRIBA_RELEASE_INGEST_BUFFERS", "1")
    made.read_chimeric_alignments(prefix + ".bam")
    monkeypatch.delenv("ARRIBA_RELEASE_INGEST_BUFFERS")
    with pytest.raises(ArribaError, match="agpu_rna_metrics: the record stream of the last ingest is not on the device any more"):
        made.write_rna_metrics(str(tmp_path / "gone.tsv"))
    made.close()
    assert sorted(os.listdir(str(tmp_path))) == ["again.tsv", "discarded.tsv", "fusions.tsv", "metrics.tsv"]
