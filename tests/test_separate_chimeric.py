"""-c: the chimeric alignments of STAR --chimOutType SeparateSAMold in a file of their own, read in front of -x as the reference reads them (source/arriba.cpp:123-130,
source/read_chimeric_alignments.cpp:560-773 with separate_chimeric_bam_file = true).

CPU tier: the refusals of the command line, the two passes of the host ingest (host/ingest.cpp) against the goldens of the unmodified reference (tests/golden/separate_*:
`arriba_ref -c C -x R`, C and R split off the generated WithinBAM file by tools/split_chimeric.py) and against the live reference where its oracle build is there, and one case per
rule of the loop on records written by hand (SAM text).
GPU tier: the role-templated kernels, the name look-up and the merge (agpu_ingest.hip) give the batch of the host ingest column by column, and the whole workflow with -c gives the
reference's files byte for byte."""
import gzip
import os
import subprocess
import sys

import pytest

import conftest
import datasets
import separate_chimeric_lib as lib

sys.path.insert(0, os.path.join(conftest.ROOT, "tools"))
from bam_to_sam import bam_to_sam  # noqa: E402

NO_CHIMERIC = "no split reads or discordant mates found"
SIDE_OUTPUTS = ["--sorted-bam", "--supporting-alignments", "--virus-expression", "--coverage", "--gene-counts", "--splice-junctions", "--allele-counts", "--realign-reads", "--rna-metrics"]


@pytest.fixture(scope="module")
def inputs(dataset_files):
    """(dataset, variant, keep_multimappers) -> (prefix, C, R); split once per module"""
    cache = {}

    def get(name, variant="clean", keep_multimappers=False):
        key = (name, variant, keep_multimappers)
        if key not in cache:
            prefix = dataset_files(name)
            cache[key] = (prefix,) + lib.split_files(prefix, variant, keep_multimappers)
        return cache[key]
    return get


def host_session(prefix, chimeric, main):
    from arriba_amd.pipeline import HostSession
    session = HostSession(prefix + ".fa", prefix + ".gtf")
    session.read_chimeric_alignments(main, separate_chimeric=chimeric)
    return session


# ---- the command line ------------------------------------------------------------------------------------------------------------------------------

def run_binary(arguments):
    return subprocess.run([lib.WORKFLOW] + arguments, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)


@pytest.mark.parametrize("option", SIDE_OUTPUTS)
def test_side_outputs_are_refused_with_c(option, built, inputs, tmp_path):
    """what reads the resident stream of ONE file is refused by its name, before anything is loaded (no GPU is needed to be told)"""
    prefix, chimeric, main = inputs("toy3k")
    outputs = (str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv"))
    extra = [option, str(tmp_path / "side")] + (["--allele-sites", prefix + ".gtf"] if option == "--allele-counts" else [])
    result = run_binary(lib.workflow_command(prefix, chimeric, main, outputs, extra)[1:])
    assert result.returncode == 1
    assert "ERROR: -c (separate chimeric alignments) and %s exclude each other" % option in result.stderr
    assert not os.path.exists(outputs[0]) and not os.path.exists(outputs[1])


def test_c_takes_readable_files_but_no_cram(built, inputs, tmp_path):
    prefix, chimeric, main = inputs("toy3k")
    outputs = (str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv"))
    missing = run_binary(lib.workflow_command(prefix, str(tmp_path / "nothing.sam"), main, outputs)[1:])
    assert missing.returncode == 1 and "ERROR: file not found/readable: " + str(tmp_path / "nothing.sam") in missing.stderr
    cram = str(tmp_path / "chimeric.cram")
    open(cram, "wb").write(b"CRAM")
    refused = run_binary(lib.workflow_command(prefix, cram, main, outputs)[1:])
    assert refused.returncode == 1 and "CRAM is not" in refused.stderr
    twice = run_binary(lib.workflow_command(prefix, chimeric, main, outputs, ["-c", chimeric])[1:])
    assert twice.returncode == 1 and "option -c specified too often" in twice.stderr
    usage = run_binary(["-h"])
    assert usage.returncode == 0 and " -c FILE  chimeric alignments of STAR run with --chimOutType SeparateSAMold" in usage.stdout
    assert "is not supported: run STAR with --chimOutType WithinBAM" not in open(os.path.join(conftest.ROOT, "arriba_amd", "csrc", "workflow", "main.cpp")).read()


def test_c_over_several_ranks_is_refused(built, emu_api, inputs, tmp_path):
    """a session over the ranks of a job (two gloo ranks, the workflow library over the stepping harness): arriba_workflow_sample_separate and a session with
    separate_chimeric_file set both end with the message, on every rank, and write nothing"""
    import json
    prefix, chimeric, main = inputs("toy3k")
    subprocess.run(["make", "-s", "-C", os.path.join(conftest.ROOT, "tests", "emu"), "libworkflow_on_harness.so"], check=True)
    command = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29677",
               os.path.join(conftest.ROOT, "tests", "separate_ranks_worker.py"), prefix + ".fa", prefix + ".gtf", str(tmp_path), chimeric, main]
    result = subprocess.run(command, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=600)
    assert result.returncode == 0, result.stdout[-3000:]
    for rank in range(2):
        report = json.load(open(str(tmp_path / ("rank%d.json" % rank))))
        assert report["world"] == 2
        for key in ("sample_separate", "option"):
            assert "ERROR: -c (separate chimeric alignments) of one sample over several ranks is not supported" in report[key], report
    assert not os.path.exists(str(tmp_path / "never.tsv"))


# ---- the host ingest against the reference ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", lib.DATASETS)
def test_host_ingest_counts_what_the_reference_counts(name, built, inputs):
    """the fragments behind pass C and behind pass R are the two "(total=N)" of the reference's log, the malformed counts its two WARNING lines; the conditions on the inputs
    are asserted on the reference's own output, so that a split that moves nothing cannot pass"""
    prefix, chimeric, main = inputs(name)
    log = lib.read_golden(name, "reference.log")
    totals, malformed = lib.totals_of(log)
    assert len(totals) == 2 and totals[0] > 0 and totals[1] > totals[0]  # (pass R added read-throughs or tandem duplications to what pass C brought)
    assert len(lib.read_golden(name, "fusions.tsv").splitlines()) > 1    # (the reference calls at least one fusion from the split input)
    session = host_session(prefix, chimeric, main)
    assert session.separate_counts == (totals[0], malformed[0])
    assert session.fragment_count == totals[1]
    names = session.fragment_names()
    assert names == sorted(names)
    if name == "itd6k":
        assert any(n.endswith(",1ITD") for n in names)  # (an ITD fragment is kept, under the name pass R gives it)


def test_main_alignments_do_not_load_twice_and_read_throughs_are_blocked(built, inputs, tmp_path):
    """variant full: -x is the WithinBAM file as it was.  Its supplementary records, discordant mates and SA pairs add nothing; its "ITD" entries sit beside the fragment of
    the same QNAME from pass C (the blocked read-through has tests of its own below)"""
    prefix, chimeric, main = inputs("itd6k", "full")
    session = host_session(prefix, chimeric, main)
    names = session.fragment_names()
    assert len(names) == len(set(names))
    held = set(names)
    assert any(n.endswith("ITD") and n[:-3] in held for n in names)  # one QNAME in both inputs: "X,1" of pass C, "X,1ITD" of pass R


def test_read_throughs_are_blocked_by_names_of_the_chimeric_file_on_shuffled2k(built, dataset_files, tmp_path):
    """the condition "at least one read-through is blocked by a name of C": the main alignments of shuffled2k as they were (variant full) insert fewer fragments behind the real C
    than behind a C of one group -- the difference are the read-throughs whose names C holds (nine of them; toy3k and itd6k block none).  The device runs the same input in
    test_device_batch_equals_the_batch_of_the_host[full-shuffled2k]."""
    prefix = dataset_files("shuffled2k")
    chimeric, main = lib.split_files(prefix, "full", tag="condition")
    session = host_session(prefix, chimeric, main)
    lines = bam_to_sam(open(chimeric, "rb").read())[0].decode().split("\n")
    first_name = next(l for l in lines if l and not l.startswith("@")).split("\t")[0]
    small = str(tmp_path / "one_group.sam")
    open(small, "w").write("\n".join([l for l in lines if l.startswith("@")] + [l for l in lines if l.split("\t")[0] == first_name]) + "\n")
    control = host_session(prefix, small, main)
    assert control.separate_counts[0] == 1
    assert control.fragment_count - 1 > session.fragment_count - session.separate_counts[0]
    if lib.reference_available():  # (the reference's own second total says the same)
        outputs = (str(tmp_path / "ref.fusions.tsv"), str(tmp_path / "ref.discarded.tsv"))
        assert lib.totals_of(lib.run_reference(prefix, chimeric, main, outputs)[0])[0] == [session.separate_counts[0], session.fragment_count]


def test_keep_multimappers_collapse_and_are_malformed(built, inputs):
    """--keep-multimappers: pass C ignores HI, the hits of one read are one name with too many alignments -- dropped and counted, as the reference's first WARNING says (live
    where the oracle build is there)"""
    prefix, chimeric, main = inputs("toy3k", "clean", True)
    session = host_session(prefix, chimeric, main)
    assert session.separate_counts[1] > 0
    assert all(n.endswith(",1") or n.endswith(",1ITD") for n in session.fragment_names())  # (pass R ignores HI as well: separate_chimeric_bam_file is true there, too)
    if lib.reference_available():
        outputs = (prefix + ".mm.ref.fusions.tsv", prefix + ".mm.ref.discarded.tsv")
        totals, malformed = lib.totals_of(lib.run_reference(prefix, chimeric, main, outputs)[0])
        assert malformed[0] > 0
        assert session.separate_counts == (totals[0], malformed[0]) and session.fragment_count == totals[1]


@pytest.mark.parametrize("name", lib.DATASETS)
@pytest.mark.parametrize("variant", ["clean", "full"])
def test_host_workflow_gives_the_files_of_the_reference(name, variant, built, emu_api, inputs, tmp_path):
    """the host ingest with -c, then the stages stepped on the host: fusions.tsv and discarded.tsv of `arriba_ref -c C -x R` byte for byte -- the committed goldens (clean), the live
    reference where its oracle build is there (both variants)"""
    from arriba_amd.pipeline import DevicePipeline
    prefix, chimeric, main = inputs(name, variant)
    if variant == "clean":
        expected = [lib.read_golden(name, "fusions.tsv"), lib.read_golden(name, "discarded.tsv")]
    elif lib.reference_available():
        outputs = (str(tmp_path / "ref.fusions.tsv"), str(tmp_path / "ref.discarded.tsv"))
        lib.run_reference(prefix, chimeric, main, outputs)
        expected = [open(path).read() for path in outputs]
    else:
        pytest.skip("the full variant has no committed golden: it is compared with the live reference (oracle/_ref/arriba_ref), which is not built here")
    session = host_session(prefix, chimeric, main)
    pipeline = DevicePipeline(session, api=emu_api)
    mine = (str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv"))
    pipeline.run_workflow(mine[0], mine[1])
    assert [open(path).read() for path in mine] == expected


# ---- records written by hand: one case per rule of the loop ---------------------------------------------------------------------------------------------

class Cases(object):
    """groups of SAM lines taken from the split toy3k files, to be edited: a paired split read (mate, clipped mate, 0x100 record), a discordant pair, a normal pair"""
    def __init__(self, prefix, chimeric, main):
        self.prefix = prefix
        lines = bam_to_sam(open(chimeric, "rb").read())[0].decode().split("\n")
        self.header = [l for l in lines if l.startswith("@")]
        body = [l.split("\t") for l in lines if l and not l.startswith("@")]
        groups = {}
        for fields in body:
            groups.setdefault(fields[0], []).append(fields)
        self.split_read = next(g for g in groups.values() if len(g) == 3 and any(int(f[1]) & 0x100 for f in g))
        self.discordant = next(g for g in groups.values() if len(g) == 2 and not any(int(f[1]) & 0x100 for f in g))
        normal = [l.split("\t") for l in bam_to_sam(open(main, "rb").read())[0].decode().split("\n") if l and not l.startswith("@")]
        fragments = set(host_session(prefix, chimeric, main).fragment_names())
        quiet = next(f[0] for f in normal if f[0] + ",1" not in fragments and f[0] + ",1ITD" not in fragments and int(f[1]) & 2)  # a proper pair that pass R makes no fragment of
        self.normal = [f for f in normal if f[0] == quiet]
        view = host_session(prefix, chimeric, main)
        self.n_aln = {name: int(view.batch_view.contents.n_aln[i]) for i, name in enumerate(view.fragment_names())}
        read_through = next(f[0] for f in normal if f[0] + ",1" in fragments and f[0] not in groups and f[0] + ",1ITD" not in fragments)  # a pair pass R extracts as a read-through
        self.read_through = [f for f in normal if f[0] == read_through]
        # ... by branch (2) of extract_read_through_alignment (neither mate spliced across the genes: two alignments) and by branch (1) / (1') (a mate spliced across: three)
        is_read_through = lambda f: f[0] + ",1" in fragments and f[0] not in groups and f[0] + ",1ITD" not in fragments
        unspliced = next(f[0] for f in normal if is_read_through(f) and self.n_aln[f[0] + ",1"] == 2)
        spliced = next(f[0] for f in normal if is_read_through(f) and self.n_aln[f[0] + ",1"] == 3)
        self.read_through_by_branch = {2: [f for f in normal if f[0] == unspliced], 1: [f for f in normal if f[0] == spliced]}
        tandem = next(f[0] for f in normal if f[0] + ",1ITD" in fragments and f[0] + ",1" not in fragments)  # a pair pass R makes an "ITD" entry of, and nothing else
        self.tandem = [f for f in normal if f[0] == tandem]

    def write(self, path, groups):
        open(path, "w").write("\n".join(self.header + ["\t".join(fields) for group in groups for fields in group]) + "\n")
        return path


def strip_tags(fields, tags=("HI", "NH")):
    return fields[:11] + [t for t in fields[11:] if t[:2] not in tags]


def with_flag(fields, flag):
    return fields[:1] + [str(flag)] + fields[2:]


@pytest.fixture(scope="module")
def cases(inputs):
    return Cases(*inputs("itd6k"))


def hand_built(cases, tmp_path, kind):
    """(C.sam, R.sam, expected names, expected n_aln, expected malformed counts (pass C, pass R)) of one case"""
    split_name, pair_name = cases.split_read[0][0], cases.discordant[0][0]
    chimeric, main = str(tmp_path / (kind + ".C.sam")), str(tmp_path / (kind + ".R.sam"))
    cases.write(main, [cases.normal])
    if kind == "paired_split_read":  # three records of one name: the fragment has three alignments
        cases.write(chimeric, [cases.split_read, cases.discordant])
        return chimeric, main, sorted([split_name + ",1", pair_name + ",1"]), {split_name + ",1": 3, pair_name + ",1": 2}, (0, 0)
    if kind == "secondary_without_hi":  # a 0x100 record without HI is kept (no missing-HI rule in pass C)
        cases.write(chimeric, [[strip_tags(f) for f in cases.split_read]])
        return chimeric, main, [split_name + ",1"], {split_name + ",1": 3}, (0, 0)
    if kind == "hi_2_is_still_1":  # HI is ignored: the name ends in ",1"
        cases.write(chimeric, [[strip_tags(f) + ["HI:i:2"] for f in cases.split_read]])
        return chimeric, main, [split_name + ",1"], {split_name + ",1": 3}, (0, 0)
    if kind == "third_paired_record":  # the third paired record of a name parks again and is never added
        cases.write(chimeric, [cases.discordant + [cases.discordant[0]]])
        return chimeric, main, [pair_name + ",1"], {pair_name + ",1": 2}, (0, 0)
    if kind == "single_end":  # two unpaired records, one of them 0x100: a fragment of pass C, removed by the second sanity check (its three alignments fail the size test there)
        clipped = next(f for f in cases.split_read if not int(f[1]) & 0x100 and ("S" in f[5] or "H" in f[5]))
        secondary = next(f for f in cases.split_read if int(f[1]) & 0x100)
        cases.write(chimeric, [[with_flag(clipped, int(clipped[1]) & 16), with_flag(secondary, 0x100 | (int(secondary[1]) & 16))], cases.discordant])
        return chimeric, main, [pair_name + ",1"], {pair_name + ",1": 2}, (0, 1)
    if kind == "malformed_in_c":  # a lone record of a pair-less name: malformed in pass C, gone before pass R
        cases.write(chimeric, [[with_flag(cases.discordant[0], int(cases.discordant[0][1]) & ~1 & 0xFFF)], cases.split_read])
        return chimeric, main, [split_name + ",1"], {split_name + ",1": 3}, (1, 0)
    through_name, tandem_name = cases.read_through[0][0], cases.tandem[0][0]
    renamed = lambda group, name: [[name] + f[1:] for f in group]
    if kind == "read_through_free":  # pass R extracts the pair as a read-through: nothing of that name in pass C
        cases.write(chimeric, [cases.split_read])
        cases.write(main, [cases.normal, cases.read_through])
        return chimeric, main, sorted([split_name + ",1", through_name + ",1"]), {split_name + ",1": 3, through_name + ",1": cases.n_aln[through_name + ",1"]}, (0, 0)
    if kind == "read_through_blocked":  # the same pair with a fragment of its name in pass C (a discordant pair): the insert fails, the fragment of pass C stays as it was
        cases.write(chimeric, [renamed(cases.discordant, through_name)])
        cases.write(main, [cases.normal, cases.read_through])
        return chimeric, main, [through_name + ",1"], {through_name + ",1": 2}, (0, 0)
    if kind == "read_through_after_malformed_c":  # the name was in pass C but did not survive its sanity check: it blocks nothing
        lone = with_flag(cases.discordant[0], int(cases.discordant[0][1]) & ~1 & 0xFFF)
        cases.write(chimeric, [renamed([lone], through_name), cases.split_read])
        cases.write(main, [cases.normal, cases.read_through])
        return chimeric, main, sorted([split_name + ",1", through_name + ",1"]), {split_name + ",1": 3, through_name + ",1": cases.n_aln[through_name + ",1"]}, (1, 0)
    if kind == "itd_in_r_for_name_in_c":  # one QNAME in both inputs: "X,1" of pass C, "X,1ITD" of pass R, one read-name group
        cases.write(chimeric, [renamed(cases.discordant, tandem_name)])
        cases.write(main, [cases.normal, cases.tandem])
        return chimeric, main, [tandem_name + ",1", tandem_name + ",1ITD"], {tandem_name + ",1": 2, tandem_name + ",1ITD": cases.n_aln[tandem_name + ",1ITD"]}, (0, 0)
    if kind == "multimappers_of_r_collapse":  # pass R ignores HI as well (l. 618): two hits of a read are one name, the second read-through finds the name taken by the first
        cases.write(chimeric, [cases.split_read])
        cases.write(main, [cases.normal, [strip_tags(f) + ["NH:i:2", "HI:i:1"] for f in cases.read_through], [strip_tags(f) + ["NH:i:2", "HI:i:2"] for f in cases.read_through]])
        return chimeric, main, sorted([split_name + ",1", through_name + ",1"]), {split_name + ",1": 3, through_name + ",1": cases.n_aln[through_name + ",1"]}, (0, 0)
    if kind == "sa_pair_in_r_adds_nothing":  # the mates of a split read in -x, the clipped one with its SA tag: the SA test holds, nothing is added (and no read-through is tried)
        mates = [f + (["SA:Z:1,100,+,50M50S,255,0;"] if ("S" in f[5] or "H" in f[5]) and not any(t.startswith("SA:") for t in f[11:]) else []) for f in cases.split_read if not int(f[1]) & 0x100]
        cases.write(chimeric, [cases.discordant])
        cases.write(main, [cases.normal, mates])
        return chimeric, main, [pair_name + ",1"], {pair_name + ",1": 2}, (0, 0)
    raise KeyError(kind)


HAND_BUILT = ["paired_split_read", "secondary_without_hi", "hi_2_is_still_1", "third_paired_record", "single_end", "malformed_in_c", "read_through_free", "read_through_blocked",
              "read_through_after_malformed_c", "itd_in_r_for_name_in_c", "multimappers_of_r_collapse", "sa_pair_in_r_adds_nothing"]


def coverage_marks(session):
    """(windows with a fragment start, windows with a fragment end) of coverage_t: add_fragment sets them for a fragment that is not chimeric -- not a read-through -- alone"""
    view = session._lib.ahost_coverage_view(session._session).contents
    windows = int(view.window_offset[view.n_contigs])
    return sum(view.fragment_starts[w] for w in range(windows)), sum(view.fragment_ends[w] for w in range(windows))


def blocked_branch_inputs(cases, tmp_path, branch, blocked):
    """a read-through pair of -x taken by `branch`, with (blocked) or without a fragment of its name in -c"""
    pair = cases.read_through_by_branch[branch]
    tag = "branch%d_%s" % (branch, "blocked" if blocked else "free")
    chimeric = cases.write(str(tmp_path / (tag + ".C.sam")), [[[pair[0][0]] + f[1:] for f in cases.discordant]] if blocked else [cases.split_read])
    return chimeric, cases.write(str(tmp_path / (tag + ".R.sam")), [cases.normal, pair])


def check_blocked_branches_in_coverage(ingest, cases, tmp_path):
    """source/read_chimeric_alignments.cpp:139-187: branch (2) returns true although the insert failed, branches (1) / (1') return false then -- and that value is is_chimeric of
    coverage.add_fragment.  Free, both pairs are read-throughs: no start and no end window.  Blocked, the pair of branch (2) still leaves none, the pair of branch (1) leaves both."""
    for branch, expected in ((2, (0, 0)), (1, (1, 1))):
        free = coverage_marks(ingest(*blocked_branch_inputs(cases, tmp_path, branch, False)))
        blocked = coverage_marks(ingest(*blocked_branch_inputs(cases, tmp_path, branch, True)))
        assert (blocked[0] - free[0], blocked[1] - free[1]) == expected, (branch, free, blocked)


def viral_inputs(cases, tmp_path, with_sa):
    """a pair on a viral contig of the header in -x: one mate 100M (a pristine alignment), the other clipped at the end the SA test looks at, with or without its SA tag"""
    viral = next(l.split("\t")[1][3:] for l in cases.header if l.startswith("@SQ") and l.split("\t")[1].startswith("SN:NC_"))
    forward, reverse = sorted(cases.normal, key=lambda f: int(f[1]) & 16)
    sequence = ("ACGTTGCATGCCATGAATCGGATTACAGCTAGCTTAGGCATCGATCCGTAAGCTTGCAACGTTAGCCTAGGATCCATGCAAGTCGATTGCACGTAGCTAGGCTAAC" * 2)
    pair = [[forward[0], forward[1], viral, "1000", "255", "20S%dM" % (len(forward[9]) - 20), "=", "1300", "400", sequence[:len(forward[9])], forward[10]] + (["SA:Z:1,100,+,20M80S,255,0;"] if with_sa else []),
            [reverse[0], reverse[1], viral, "1300", "255", "%dM" % len(reverse[9]), "=", "1000", "-400", sequence[7:7 + len(reverse[9])], reverse[10]]]
    tag = "viral_sa" if with_sa else "viral"
    return cases.write(str(tmp_path / (tag + ".C.sam")), [cases.split_read]), cases.write(str(tmp_path / (tag + ".R.sam")), [cases.read_through, pair])


def check_sa_pair_suppresses_the_viral_count(ingest, cases, tmp_path):
    """l. 723-739: without the SA tag the pair is neither chimeric nor a tandem duplication, so its pristine mate is counted on the viral contig; with the tag the SA branch is
    taken, which adds nothing with -c and never reaches the count"""
    plain = ingest(*viral_inputs(cases, tmp_path, False))
    tagged = ingest(*viral_inputs(cases, tmp_path, True))
    assert plain.viral_read_total == 1 and tagged.viral_read_total == 0
    assert plain.fragment_names() == tagged.fragment_names() == sorted([cases.split_read[0][0] + ",1", cases.read_through[0][0] + ",1"])


def host_ingest_of(cases):
    return lambda chimeric, main: host_session(cases.prefix, chimeric, main)


def test_blocked_branches_in_coverage_on_the_host(built, cases, tmp_path):
    check_blocked_branches_in_coverage(host_ingest_of(cases), cases, tmp_path)


def test_sa_pair_suppresses_the_viral_count_on_the_host(built, cases, tmp_path):
    check_sa_pair_suppresses_the_viral_count(host_ingest_of(cases), cases, tmp_path)


def same_mate_flags(cases, tmp_path):
    """a paired split read of C whose two mates both say first-in-pair (the 0x100 record says second): the second sanity check of the reference would swap the mates once more"""
    clipped = lambda f: "S" in f[5] or "H" in f[5]
    mates = sorted((f for f in cases.split_read if not int(f[1]) & 0x100), key=clipped)  # the clipped mate last: it is added first and survives the first sanity check as the split read
    group = [with_flag(f, (int(f[1]) & ~0xC0) | (0x80 if int(f[1]) & 0x100 else 0x40)) for f in mates + [f for f in cases.split_read if int(f[1]) & 0x100]]
    return cases.write(str(tmp_path / "same_flags.C.sam"), [group]), cases.write(str(tmp_path / "same_flags.R.sam"), [cases.normal])


def test_two_names_with_one_key(stand_alone, cases, tmp_path):
    """agpu_ingest_config has no seed for the keys of the look-up, so no input makes two names meet in one key; the stand-alone program calls name_is_taken on a table whose key is
    forced -- the key of one name over the bytes of another -- and the bytes decide"""
    chimeric = raw_stream(lib.split_files(cases.prefix, "clean", tag="key")[0])
    main = cases.write(str(tmp_path / "R.sam"), [cases.normal])
    result = subprocess.run([stand_alone, cases.prefix + ".fa", cases.prefix + ".gtf", chimeric, main, str(tmp_path), "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert result.returncode == 0, result.stderr[-1000:]
    assert "two names with one key do not block each other" in result.stdout


def test_same_mate_flags_are_refused_on_the_host(built, cases, tmp_path):
    from arriba_amd.pipeline import ArribaError
    chimeric, main = same_mate_flags(cases, tmp_path)
    with pytest.raises(ArribaError, match="two mates with the same first-in-pair flag"):
        host_session(cases.prefix, chimeric, main)


def check_hand_built(session, expected_names, expected_n_aln):
    names = session.fragment_names()
    assert names == expected_names
    view = session.batch_view.contents
    assert {name: int(view.n_aln[i]) for i, name in enumerate(names)} == expected_n_aln


@pytest.mark.parametrize("kind", HAND_BUILT)
def test_rules_of_the_loop_on_the_host(kind, built, cases, tmp_path, capfd):
    chimeric, main, names, n_aln, malformed = hand_built(cases, tmp_path, kind)
    session = host_session(cases.prefix, chimeric, main)
    check_hand_built(session, names, n_aln)
    assert session.separate_counts[1] == malformed[0]
    warnings = [line for line in capfd.readouterr().err.splitlines() if "SAM records were malformed" in line]
    assert warnings == ["WARNING: %d SAM records were malformed and ignored" % count for count in malformed if count > 0]


def test_refusals_of_the_ingest_on_the_host(built, cases, tmp_path):
    """a record of -c without a reference, headers that differ, and a -c file without chimeric alignments: each an error by its message"""
    from arriba_amd.pipeline import ArribaError, HostSession
    main = cases.write(str(tmp_path / "R.sam"), [cases.normal])
    unplaced = cases.discordant[0][:2] + ["*", "0"] + cases.discordant[0][4:]
    for chimeric, message in ((cases.write(str(tmp_path / "unplaced.sam"), [cases.split_read, [unplaced]]), "a record of the separate chimeric file (-c) is damaged or has no reference sequence"),
                              (cases.write(str(tmp_path / "empty.sam"), []), NO_CHIMERIC)):
        with pytest.raises(ArribaError, match=message.replace("(", r"\(").replace(")", r"\)")):
            HostSession(cases.prefix + ".fa", cases.prefix + ".gtf").read_chimeric_alignments(main, separate_chimeric=chimeric)
    other = Cases(cases.prefix, *lib.split_files(cases.prefix, "clean", tag="other"))
    other.header = [l for l in cases.header if not l.startswith("@SQ")] + [l for l in cases.header if l.startswith("@SQ")][::-1]
    swapped = other.write(str(tmp_path / "swapped.sam"), [[f[:2] + ["*", "0"] + f[4:6] + ["*", "0", "0"] + f[9:] for f in cases.normal]])
    with pytest.raises(ArribaError, match="do not list the same reference sequences in the same order"):
        HostSession(cases.prefix + ".fa", cases.prefix + ".gtf").read_chimeric_alignments(swapped, separate_chimeric=cases.write(str(tmp_path / "C.sam"), [cases.split_read]))


# ---- the stand-alone program (tools/separate_chimeric_main.cpp; under ASan + UBSan: tools/sanitize_separate_chimeric.sh) ---------------------------------------------------------

@pytest.fixture(scope="module")
def stand_alone(built, tmp_path_factory):
    """the program linked against the built host library (the sanitizer build compiles the host sources in instead)"""
    binary = str(tmp_path_factory.mktemp("stand_alone") / "separate_chimeric_main")
    library = os.path.join(conftest.ROOT, "arriba_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-pthread", "-Wno-parentheses", "-o", binary, os.path.join(conftest.ROOT, "tools", "separate_chimeric_main.cpp"), "-L" + library, "-larriba_host", "-Wl,-rpath," + library], check=True)
    return binary


def raw_stream(path):
    from bam_to_sam import inflate_all
    out = path + ".raw"
    open(out, "wb").write(inflate_all(open(path, "rb").read()))
    return out


@pytest.mark.parametrize("name", lib.DATASETS)
@pytest.mark.parametrize("variant", ["clean", "full"])
def test_stand_alone_program_steps_the_device_loop(name, variant, stand_alone, inputs, tmp_path):
    """the host ingest on (C, R); both passes of the device's loop body (replay_group_as with its role, name_is_taken over the names of pass C, normalize_plan) stepped over the same
    bytes give its fragments, name by name with the number of alignments, and its malformed count of pass C; the key of the look-up is the key of the record"""
    prefix, chimeric, main = inputs(name, variant)
    result = subprocess.run([stand_alone, prefix + ".fa", prefix + ".gtf", raw_stream(chimeric), raw_stream(main), str(tmp_path), "0"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=120)
    assert result.returncode == 0, result.stderr[-1000:]
    assert "pass C stepped with the device code" in result.stdout and "as the host ingest" in result.stdout
    assert "both passes stepped with the device code" in result.stdout and "names and alignment counts as the host ingest" in result.stdout


def test_stand_alone_program_refuses_a_chimeric_file_cut_short(stand_alone, cases, tmp_path):
    """C cut at every byte of its last three records: inside a record refused ("failed to load alignments"), between two records a shorter file"""
    chimeric = raw_stream(lib.split_files(cases.prefix, "clean", tag="cut")[0])
    main = cases.write(str(tmp_path / "R.sam"), [cases.normal])
    result = subprocess.run([stand_alone, cases.prefix + ".fa", cases.prefix + ".gtf", chimeric, main, str(tmp_path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert result.returncode == 0, result.stderr[-1000:]
    assert "3 cuts between records accepted" in result.stdout


# ---- the device ---------------------------------------------------------------------------------------------------------------------------------------------

def device_and_host_batches(prefix, chimeric, main):
    from arriba_amd.pipeline import DevicePipeline, HostSession
    from test_host_and_device_logic import _batch_columns, _device_batch_columns
    host = host_session(prefix, chimeric, main)
    expected = _batch_columns(host)
    expected["coverage"] = int(host._lib.ahost_coverage_checksum(host._session))
    session = HostSession(prefix + ".fa", prefix + ".gtf")
    pipeline = DevicePipeline(session, bam=main, separate_chimeric=chimeric, piece_bytes=2 << 20)
    mine = _device_batch_columns(session, pipeline)
    counts = (int(pipeline.separate_result.fragments), int(pipeline.separate_result.malformed_count), int(pipeline.ingest_result.malformed_count))
    return mine, expected, counts, host


@pytest.mark.gpu
@pytest.mark.parametrize("name", lib.DATASETS)
@pytest.mark.parametrize("variant", ["clean", "full"])
def test_device_batch_equals_the_batch_of_the_host(name, variant, built, inputs):
    """role ingest of C, name keys, role ingest of R with the look-up, merge: every column, pool and name, coverage_t and mapped_reads as the host comparator has them"""
    mine, expected, counts, host = device_and_host_batches(*inputs(name, variant))
    assert counts[:2] == host.separate_counts
    for key in sorted(expected):
        assert mine[key] == expected[key], key


@pytest.mark.gpu
def test_device_batch_with_collapsed_multimappers(built, inputs):
    mine, expected, counts, host = device_and_host_batches(*inputs("toy3k", "clean", True))
    assert counts[:2] == host.separate_counts and counts[1] > 0
    assert mine == expected


@pytest.mark.gpu
@pytest.mark.parametrize("kind", HAND_BUILT)
def test_rules_of_the_loop_on_the_device(kind, built, cases, tmp_path):
    chimeric, main, names, n_aln, malformed = hand_built(cases, tmp_path, kind)
    mine, expected, counts, host = device_and_host_batches(cases.prefix, chimeric, main)
    assert mine == expected and mine["names"] == names
    assert (counts[1], counts[2]) == malformed


def split_chimeric_module():
    import split_chimeric
    return split_chimeric


def run_workflow_binary(prefix, chimeric, main, directory, extra=(), stdin=None):
    outputs = (os.path.join(directory, "fusions.tsv"), os.path.join(directory, "discarded.tsv"))
    result = subprocess.run(lib.workflow_command(prefix, chimeric, main, outputs, extra), stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert result.returncode == 0, result.stderr[-2000:]
    return [open(path).read() for path in outputs], lib.strip_times(result.stdout), result.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("name", lib.DATASETS)
def test_workflow_with_c_gives_the_goldens(name, built, inputs, tmp_path):
    """arriba_gpu_workflow -c C -x R: both files of the reference byte for byte, the two (total=N) of its ingest and every (remaining=N) of its log; --host-ingest gives the same"""
    prefix, chimeric, main = inputs(name)
    expected = [lib.read_golden(name, "fusions.tsv"), lib.read_golden(name, "discarded.tsv")]
    log = lib.read_golden(name, "reference.log")
    for extra in ([], ["--host-ingest"]):
        directory = tmp_path / ("host" if extra else "device")
        directory.mkdir()
        files, mine_log, _ = run_workflow_binary(prefix, chimeric, main, str(directory), extra)
        assert files == expected, extra
        assert lib.totals_of(mine_log)[0] == lib.totals_of(log)[0]
        assert lib.remaining_of(mine_log) == lib.remaining_of(log), extra


@pytest.mark.gpu
def test_workflow_with_c_takes_every_container_and_sam_text(built, inputs, tmp_path):
    """C as SAM text, gzip of the BAM stream, stored BGZF (what the split writes) and the uncompressed BAM stream: the same files; and a plain -x run on the same data gives what
    it gave before and after (nothing of the roles stays behind in a fresh process, nor in one context: the device-batch test above runs -x and -c through one library)"""
    from bam_to_sam import inflate_all
    prefix, chimeric, main = inputs("toy3k")
    expected = [lib.read_golden("toy3k", "fusions.tsv"), lib.read_golden("toy3k", "discarded.tsv")]
    stream = inflate_all(open(chimeric, "rb").read())
    text = bam_to_sam(open(chimeric, "rb").read())[0]
    variants = {"sam": text, "gzip": gzip.compress(stream, 1), "raw": stream, "deflated_bgzf": lib.bgzf_deflated(stream), "sam_gzip": gzip.compress(text, 1), "sam_bgzf": lib.bgzf_deflated(text),
                "sam_stored_bgzf": split_chimeric_module().bgzf_stored(text)}
    for kind, data in variants.items():
        path = str(tmp_path / ("chimeric." + kind))
        open(path, "wb").write(data)
        directory = tmp_path / kind
        directory.mkdir()
        assert run_workflow_binary(prefix, path, main, str(directory))[0] == expected, kind


@pytest.mark.gpu
def test_plain_x_is_unchanged_around_a_c_run(built, inputs, tmp_path):
    """one context: -x alone, then -c, then -x alone again -- the batch of -x is what it was (no role state leaks), and -c in between is the host comparator's"""
    from arriba_amd.pipeline import DevicePipeline, HostSession
    from test_host_and_device_logic import _device_batch_columns
    prefix, chimeric, main = inputs("toy3k")
    session = HostSession(prefix + ".fa", prefix + ".gtf")
    pipeline = DevicePipeline(session, bam=prefix + ".bam", piece_bytes=2 << 20)
    before = _device_batch_columns(session, pipeline)
    pipeline.read_chimeric_alignments_separate(chimeric, main, piece_bytes=2 << 20)
    between = _device_batch_columns(session, pipeline)
    pipeline.read_chimeric_alignments(prefix + ".bam", piece_bytes=2 << 20)
    assert _device_batch_columns(session, pipeline) == before
    assert between["n"] == host_session(prefix, chimeric, main).fragment_count and between != before


@pytest.mark.gpu
def test_workflow_with_c_equals_the_live_reference(built, tmp_path):
    """a sample of 60 000 fragments against `arriba_ref -c` run now (where the oracle build travelled): both files byte for byte"""
    if not lib.reference_available():
        pytest.skip("oracle/_ref/arriba_ref is not built here")
    spec = {"args": ["--seed", "67", "--fragments", "60000", "--normal-mult", "0.4", "--contigs", "6", "--contig-len", "500000", "--junctions", "700", "--dup", "0.15", "--itd-hotspots", "3", "--itd-hotspot-frac", "0.03"]}
    prefix = datasets.generate(spec, str(tmp_path))
    chimeric, main = lib.split_files(prefix, "clean")
    outputs = (str(tmp_path / "ref.fusions.tsv"), str(tmp_path / "ref.discarded.tsv"))
    log, _ = lib.run_reference(prefix, chimeric, main, outputs)
    files, mine_log, _ = run_workflow_binary(prefix, chimeric, main, str(tmp_path))
    assert files == [open(path).read() for path in outputs]
    assert lib.totals_of(mine_log)[0] == lib.totals_of(log)[0]


@pytest.mark.gpu
def test_same_mate_flags_are_refused_on_the_device(built, cases, tmp_path):
    from arriba_amd.pipeline import ArribaError, DevicePipeline, HostSession
    chimeric, main = same_mate_flags(cases, tmp_path)
    with pytest.raises(ArribaError, match="two mates with the same first-in-pair flag"):
        DevicePipeline(HostSession(cases.prefix + ".fa", cases.prefix + ".gtf"), bam=main, separate_chimeric=chimeric, piece_bytes=2 << 20)


@pytest.mark.gpu
def test_refusals_of_the_ingest_through_the_binary(built, cases, tmp_path):
    """on the device path, by their messages and before any output: a record of -c without a reference, headers that differ, a -c file without chimeric alignments"""
    main = cases.write(str(tmp_path / "R.sam"), [cases.normal])
    unplaced = cases.discordant[0][:2] + ["*", "0"] + cases.discordant[0][4:]
    reversed_header = Cases.__new__(Cases)
    reversed_header.header = [l for l in cases.header if not l.startswith("@SQ")] + [l for l in cases.header if l.startswith("@SQ")][::-1]
    swapped = reversed_header.write(str(tmp_path / "swapped.sam"), [[f[:2] + ["*", "0"] + f[4:6] + ["*", "0", "0"] + f[9:] for f in cases.normal]])
    good = cases.write(str(tmp_path / "C.sam"), [cases.split_read])
    outputs = (str(tmp_path / "fusions.tsv"), str(tmp_path / "discarded.tsv"))
    for chimeric, rna, message in ((cases.write(str(tmp_path / "unplaced.sam"), [cases.split_read, [unplaced]]), main, "a record of the separate chimeric file (-c) is damaged or has no reference sequence"),
                                   (good, swapped, "do not list the same reference sequences in the same order"),
                                   (cases.write(str(tmp_path / "empty.sam"), []), main, NO_CHIMERIC)):
        result = run_binary(lib.workflow_command(cases.prefix, chimeric, rna, outputs)[1:])
        assert result.returncode == 1 and "ERROR: " in result.stderr and message in result.stderr, result.stderr[-600:]
        assert not os.path.exists(outputs[0]) and not os.path.exists(outputs[1])


@pytest.mark.gpu
def test_session_sample_separate(built, inputs, tmp_path):
    """arriba_workflow_sample_separate: the goldens through a resident session; the sample behind it is an ordinary -x sample again; refused with a sample submitted ahead and with
    the ingest finished ahead"""
    from arriba_amd.pipeline import ArribaError, WorkflowSession
    prefix, chimeric, main = inputs("toy3k")
    expected = [lib.read_golden("toy3k", "fusions.tsv"), lib.read_golden("toy3k", "discarded.tsv")]
    whole = [gzip.open(os.path.join(conftest.ROOT, "tests", "golden", "toy3k", name + ".gz"), "rt").read() for name in ("fusions.tsv", "discarded.tsv")]
    session = WorkflowSession(prefix + ".fa", prefix + ".gtf", params={"disable_filters": ["blacklist"]})
    try:
        files = lambda tag: (str(tmp_path / (tag + ".fusions.tsv")), str(tmp_path / (tag + ".discarded.tsv")))
        session.sample_separate(chimeric, main, *files("separate"))
        assert [open(path).read() for path in files("separate")] == expected
        session.sample(prefix + ".bam", *files("whole"))  # (separate_chimeric_file of the lanes is reset)
        assert [open(path).read() for path in files("whole")] == whole
        session.sample_separate(chimeric, main, *files("again"))
        assert [open(path).read() for path in files("again")] == expected
        session.finish_ahead(True)
        with pytest.raises(ArribaError, match="-c and arriba_workflow_finish_ahead exclude each other"):
            session.sample_separate(chimeric, main, *files("refused"))
        session.finish_ahead(False)
        session.submit(prefix + ".bam")
        with pytest.raises(ArribaError, match="samples are submitted already"):
            session.sample_separate(chimeric, main, *files("refused"))
        session.sample(prefix + ".bam", *files("submitted"))
        assert [open(path).read() for path in files("submitted")] == whole
    finally:
        session.close()


def device_ingest_of(cases):
    def ingest(chimeric, main):
        from arriba_amd.pipeline import DevicePipeline, HostSession
        session = HostSession(cases.prefix + ".fa", cases.prefix + ".gtf")
        session.pipeline = DevicePipeline(session, bam=main, separate_chimeric=chimeric, piece_bytes=2 << 20)  # (coverage_t and the viral counts come back to the session)
        session.fragment_names = lambda: [n for n in _names_of(session.pipeline)]
        return session
    return ingest


def _names_of(pipeline):
    arrays, _ = pipeline.batch_rows()
    text, offsets = arrays["names"].tobytes().decode(), arrays["name_offset"]
    return [text[offsets[i]:offsets[i + 1]] for i in range(arrays["n"])]


@pytest.mark.gpu
def test_blocked_branches_in_coverage_on_the_device(built, cases, tmp_path):
    check_blocked_branches_in_coverage(device_ingest_of(cases), cases, tmp_path)


@pytest.mark.gpu
def test_sa_pair_suppresses_the_viral_count_on_the_device(built, cases, tmp_path):
    check_sa_pair_suppresses_the_viral_count(device_ingest_of(cases), cases, tmp_path)
