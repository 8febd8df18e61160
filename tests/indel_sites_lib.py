"""What tests/test_indel_sites.py needs beside the project: a restatement of the rule of --indel-sites in plain Python -- dicts by (reference, anchor, type,
length, bases) and by (reference, position), string operations for the normalisation, no keys, no packing, no sort of words --, and the cases that are made at test time on the
committed assembly (tests/golden/indel_sites/hand_made.{fa,gtf}: a homopolymer run i1 12..19, a dinucleotide repeat i1 31..42, a homopolymer that runs into lower case i1 47..54, an
N at i1 65, a homopolymer at the start of chr2, and orphan, which the header knows and the assembly lacks).  It is written from the rule, not from indel_core.hpp, and shares no code
with the project; it is the independent side for inputs made at test time only because it gives tests/golden/indel_sites/hand_made.tsv, which a reader can check by eye, from
hand_made.sam.

A case is a dict: "references" a list of (name, LN); "records" as in allele_counts_lib (qname, flag, rname or "*", 1-based pos, mapq, cigar text or "*", seq, qual); "min_mapq",
"min_alt", "min_percent"; "max_shift" (the cap of rule 4; the tests set ARRIBA_INDEL_MAX_SHIFT to it where it is not 4096)."""
import os
import random
import re

from allele_counts_lib import bam_header, bam_records, load_assembly as _load, parse_sam, stream_pipeline, write_bgzf  # noqa: F401 (the record writer and the containers)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "indel_sites")
COMMITTED_CONTIGS = "i1 2"
HEADER = [("i1", 120), ("chr2", 50), ("orphan", 700)]  # of the committed case: chr2 is 2 in the assembly, orphan is not in it
HEADER_LINE = "#CONTIG\tPOS\tREF\tTYPE\tLENGTH\tBASES\tSUPPORT\tDEPTH\n"
COUNTED = ("records", "contributing", "operations", "events", "unkeyed_insertions", "shift_capped", "runs", "candidates", "sites", "reported")
COMMITTED_THRESHOLDS = {"min_mapq": 20, "min_alt": 2, "min_percent": 20}
DEFAULTS = {"min_mapq": 20, "min_alt": 3, "min_percent": 5, "max_shift": 4096}


def load_assembly():
    return _load(os.path.join(GOLDEN, "hand_made.fa"))


def committed_case():
    case = parse_sam(open(os.path.join(GOLDEN, "hand_made.sam"), "rb").read())
    del case["sites"], case["min_baseq"]
    case.update(DEFAULTS)
    case.update(COMMITTED_THRESHOLDS)
    return case


# ---- the rule -------------------------------------------------------------------------------------------------------------------------------------------------------

def operations_of(cigar):
    return [(int(count), op) for count, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]


def counts(record, min_mapq):
    """rule 1"""
    qname, flag, rname, pos, mapq, cigar, seq, qual = record
    if flag & (0x4 | 0x100 | 0x200 | 0x400) or rname == "*" or mapq < min_mapq or cigar == "*" or seq == "*":
        return False
    return sum(count for count, op in operations_of(cigar) if op in "MIS=X") == len(seq)


def ref_base(assembly, reference, position):
    """REF at a 0-based position of a reference of the header: upper case, N where the assembly holds nothing"""
    bases = assembly.get(reference[3:] if reference.startswith("chr") else reference, "")
    return bases[position].upper() if 0 <= position < len(bases) else "N"


def normalise(ref, kind, anchor, length, bases, max_shift):
    """rule 4 -> (anchor, bases, whether the cap stopped it); ref: position -> base"""
    steps = 0
    while anchor >= 1 and ref(anchor) in "ACGT" and (ref(anchor) == ref(anchor + length) if kind == "DEL" else bases[-1] == ref(anchor)):
        if steps == max_shift:
            return anchor, bases, True
        if kind == "INS":
            bases = bases[-1] + bases[:-1]
        anchor -= 1
        steps += 1
    return anchor, bases, False


def restate(assembly, case):
    """-> (text of the file, the statistics of COUNTED)"""
    references = case["references"]
    index_of = {name: k for k, (name, _) in enumerate(references)}
    support, depth = {}, {}  # (reference, anchor, type, length, bases) -> records; (reference, position) -> records with a base or a deletion there
    stats = dict.fromkeys(COUNTED, 0)
    stats["records"] = len(case["records"])
    for record in case["records"]:
        if record[2] != "*" and record[2] not in index_of or not counts(record, case["min_mapq"]):
            continue
        stats["contributing"] += 1
        qname, flag, rname, pos, mapq, cigar, seq, qual = record
        operations, length, index = operations_of(cigar), dict(references)[rname], index_of[rname]
        aligned = [k for k, (count, op) in enumerate(operations) if op in "M=X" and count >= 1]
        at, i = pos - 1, 0
        for k, (count, op) in enumerate(operations):
            if op in "ID" and count >= 1 and aligned and aligned[0] < k < aligned[-1] and 0 <= at - 1 < length and (op == "I" or at + count <= length):  # rule 2
                stats["operations"] += 1
                inserted = seq[i:i + count] if op == "I" else ""
                if op == "I" and (count > 28 or any(base not in "ACGT" for base in inserted)):  # rule 3
                    stats["unkeyed_insertions"] += 1
                else:
                    anchor, inserted, capped = normalise(lambda position: ref_base(assembly, rname, position), "INS" if op == "I" else "DEL", at - 1, count, inserted, case["max_shift"])
                    stats["events"] += 1
                    stats["shift_capped"] += capped
                    event = (index, anchor, "INS" if op == "I" else "DEL", count, inserted)
                    support[event] = support.get(event, 0) + 1
            if op in "M=XD":
                for position in range(max(at, 0), min(at + count, length)):
                    depth[(index, position)] = depth.get((index, position), 0) + 1
            at += count if op in "M=XDN" else 0
            i += count if op in "M=XIS" else 0
    stats["runs"] = len(support)
    lines, sites = [HEADER_LINE], set()
    for event in sorted(support, key=lambda e: (e[0], e[1], e[2] == "INS", e[3], e[4])):  # rule 5: by site, deletions first, by length, by bases
        index, anchor, kind, length, inserted = event
        if support[event] < case["min_alt"]:  # rule 6
            continue
        stats["candidates"] += 1
        sites.add((index, anchor))
        at_anchor = depth.get((index, anchor), 0)
        if support[event] * 100 < case["min_percent"] * at_anchor:  # rule 7
            continue
        stats["reported"] += 1
        name = references[index][0]
        bases = inserted if kind == "INS" else "".join(ref_base(assembly, name, anchor + 1 + j) for j in range(length)) if length <= 64 else "."
        lines.append("%s\t%d\t%s\t%s\t%d\t%s\t%d\t%d\n" % (name, anchor + 1, ref_base(assembly, name, anchor), kind, length, bases, support[event], at_anchor))
    stats["sites"] = len(sites)
    return "".join(lines).encode(), stats


# ---- cases made at test time ------------------------------------------------------------------------------------------------------------------------------------------

def _case(records, references=None, **thresholds):
    case = {"references": list(HEADER if references is None else references), "records": records}
    case.update(DEFAULTS)
    case.update(thresholds)
    return case


def read(assembly, name, contig, pos, cigar, inserted="", flag=0, mapq=30, clip="T"):
    """a record that shows the assembly from 1-based `pos` on under its aligned blocks (N where the assembly holds nothing, A in front of the reference), the bases of `inserted`
    one after the other under its I operations and `clip` under S"""
    seq, at, taken = "", pos - 1, 0
    for count, op in operations_of(cigar):
        if op in "M=X":
            seq += "".join(ref_base(assembly, contig, at + j) if at + j >= 0 else "A" for j in range(count))
        elif op == "I":
            seq += inserted[taken:taken + count]
            taken += count
        elif op == "S":
            seq += clip * count
        at += count if op in "M=XDN" else 0
    assert taken == len(inserted), (name, cigar, inserted)
    return (name, flag, contig, pos, mapq, cigar, seq, "I" * len(seq))


FOUR_EVENTS = "5M1I5M1D5M2I5M3D5M"  # on i1 from 81 on: nothing there can shift


def wavefront_case(n):
    """n records: plain ones, and records with events at the lanes the fill pass can go wrong at -- lane 0 (a record with four events), lane 63 (62 of 63 records), the first lane
    of the next wavefront; with 129 records the wavefront in the middle has none"""
    def make(assembly):
        carriers = {min(63, n - 1): ("6M2D6M", ""), 64: ("6M3I6M", "GAT"), 128: ("4M1D8M", ""), 0: (FOUR_EVENTS, "GTC")}
        if n == 129:
            del carriers[64]
        records = []
        for k in range(n):
            cigar, inserted = carriers.get(k, ("12M", ""))
            records.append(read(assembly, "w%03d" % k, "i1", 81, cigar, inserted) if k in carriers else read(assembly, "w%03d" % k, "i1", 1 + k % 100, cigar))
        return _case(records, min_alt=1, min_percent=0)
    return make


def insertions_case(assembly):
    """insertions of 1, 27, 28 and 29 bases (the last has no key), one with an N, and the same insertion at an even and at an odd read index behind a soft clip of three bases"""
    long_one = "ACGTTGCATGCAGGCTTAGCATCGATCGA"  # 29 bases
    records = [read(assembly, "one", "i1", 81, "6M1I6M", "G"), read(assembly, "l27", "i1", 81, "6M27I6M", long_one[:27]), read(assembly, "l28", "i1", 81, "6M28I6M", long_one[:28]),
               read(assembly, "l28b", "i1", 81, "6M28I6M", long_one[:27] + "T"), read(assembly, "l29", "i1", 81, "6M29I6M", long_one), read(assembly, "withn", "i1", 81, "6M3I6M", "ANC"),
               read(assembly, "even", "i1", 101, "3S5M2I6M", "GT", clip="C"), read(assembly, "odd", "i1", 102, "3S4M2I6M", "GT", clip="C"), read(assembly, "odd3", "i1", 102, "3S4M3I6M", "GTA"),
               read(assembly, "iupac", "i1", 81, "6M2I6M", "AR")]
    return _case(records, min_alt=1, min_percent=0)


def normalisation_case(assembly):
    """a deletion and an insertion moved to the start of the homopolymer i1 12..19; a shift stopped at anchor 0 (chr2 1..8 is A); one stopped at the N of i1 65; one across lower
    case (i1 47..54); the rotation of an inserted dinucleotide in i1 31..42; the same deletion placed at both ends of the homopolymer by two records: one line, support 2; a
    deletion of two bases of the dinucleotide repeat; an insertion that cannot move"""
    records = [read(assembly, "t_left", "i1", 6, "7M1D10M"), read(assembly, "t_right", "i1", 6, "13M1D4M"), read(assembly, "t_ins", "i1", 6, "12M1I6M", "T"), read(assembly, "t_ins2", "i1", 6, "12M2I6M", "TT"),
               read(assembly, "t_two", "i1", 6, "10M2D6M"), read(assembly, "zero", "chr2", 1, "5M1D6M"), read(assembly, "zero_ins", "chr2", 1, "6M2I6M", "AA"), read(assembly, "at_n", "i1", 61, "8M1D5M"),
               read(assembly, "lower", "i1", 43, "11M1D6M"), read(assembly, "lower_ins", "i1", 43, "12M1I6M", "A"), read(assembly, "ca_right", "i1", 26, "17M2I4M", "CA"), read(assembly, "ca_middle", "i1", 26, "8M2I13M", "AC"),
               read(assembly, "ca_del", "i1", 26, "15M2D4M"), read(assembly, "ca_four", "i1", 26, "17M4I4M", "CACA"), read(assembly, "stays", "i1", 81, "6M1I6M", "T"), read(assembly, "cag", "i1", 26, "17M3I4M", "CAG")]
    return _case(records, min_alt=1, min_percent=0)


def capped_case(assembly):
    """the same records with at most two steps per event: the events that were due a third step are counted, and the two ends of the homopolymer do not meet any more"""
    case = normalisation_case(assembly)
    case["max_shift"] = 2
    return case


def edges_case(assembly):
    """a deletion that ends at LN and one that ends one behind it; an anchor of -1; leading and trailing I and D; an I between S and M and one between M and S; I next to D and D
    next to I; an I in front of an N; H and P beside them; a reference the assembly lacks (REF N, nothing shifts); a deletion of 70 bases (BASES '.'); an M of span 0 is no block"""
    records = [read(assembly, "ends_at_ln", "i1", 111, "7M3D4M"), read(assembly, "behind_ln", "i1", 111, "7M4D4M"), read(assembly, "ins_at_ln", "i1", 111, "10M2I4M", "GG"), read(assembly, "ins_behind_ln", "i1", 111, "11M2I4M", "GG"),
               read(assembly, "anchor_minus_one", "i1", 0, "1M2D6M"), read(assembly, "anchor_minus_one_ins", "i1", 0, "1M2I6M", "GG"), read(assembly, "anchor_zero", "i1", 1, "1M2D6M"),
               read(assembly, "leading_i", "i1", 81, "2I10M", "GG"), read(assembly, "leading_d", "i1", 81, "2D10M"), read(assembly, "trailing_i", "i1", 81, "10M2I", "GG"), read(assembly, "trailing_d", "i1", 81, "10M2D"),
               read(assembly, "s_i_m", "i1", 81, "3S2I10M", "GG"), read(assembly, "m_i_s", "i1", 81, "10M2I3S", "GG"), read(assembly, "m_d_s", "i1", 81, "10M2D3S"), read(assembly, "zero_m", "i1", 81, "0M2I10M", "GG"),
               read(assembly, "i_d", "i1", 21, "5M1I2D5M", "T"), read(assembly, "d_i", "i1", 21, "5M2D1I5M", "T"), read(assembly, "i_n", "i1", 81, "5M2I10N5M", "GG"), read(assembly, "n_d", "i1", 81, "5M10N2D5M"),
               read(assembly, "hard", "i1", 81, "2H5M1D5M3H"), read(assembly, "pad", "i1", 81, "5M1P1I5M", "G"), read(assembly, "long_del", "i1", 21, "5M70D5M"), read(assembly, "zero_d", "i1", 81, "5M0D5M")]
    records += [read(assembly, "orphan%d" % k, "orphan", 10, "5M1D5M") for k in range(2)] + [read(assembly, "orphan_ins", "orphan", 10, "5M2I5M", "AC")]
    return _case(records, min_alt=1, min_percent=0)


def filters_case(assembly):
    """each excluded flag; MAPQ one below the threshold and at it; no SEQ; an l_seq that disagrees with the CIGAR; a supplementary and a reverse record count"""
    records = [read(assembly, "flag%d" % flag, "i1", 81, "6M2D6M", flag=flag) for flag in (0x4, 0x100, 0x200, 0x400, 0x704, 0x800, 0x10)]
    records += [read(assembly, "mapq%d_%d" % (mapq, k), "i1", 21, "5M1I5M", "T", mapq=mapq) for k, mapq in enumerate((19, 20, 19, 255, 0))]
    records += [("noseq", 0, "chr2", 11, 30, "5M1D5M", "*", "*")]
    disagrees = read(assembly, "short", "chr2", 11, "5M1D4M")
    records += [disagrees[:5] + ("5M1D5M",) + disagrees[6:], read(assembly, "agrees", "chr2", 11, "5M1D5M")]
    return _case(records, min_alt=1, min_percent=0)


def support_case(assembly):
    """support > depth: two records begin inside the homopolymer at the start of chr2 and their deletion moves to anchor 0, in front of their own start; two more span it.  The
    percent test: 2 of 11 at 20 percent is not reported, 2 of 10 is; support of min_alt - 1 is no candidate; a site with a deletion and two insertions of which one passes"""
    records = [read(assembly, "inside%d" % k, "chr2", 7, "1M1D5M") for k in range(2)] + [read(assembly, "spans%d" % k, "chr2", 1, "5M1D6M") for k in range(2)]
    records += [read(assembly, "p%d" % k, "i1", 71, "5M1I5M", "A") for k in range(2)] + [read(assembly, "plain%d" % k, "i1", 71, "10M") for k in range(9)]
    records += [read(assembly, "q%d" % k, "i1", 101, "5M1I5M", "A") for k in range(2)] + [read(assembly, "plainq%d" % k, "i1", 101, "10M") for k in range(8)]
    records += [read(assembly, "once", "i1", 81, "6M2D6M")] + [read(assembly, "site%d" % k, "i1", 21, cigar, inserted) for k, (cigar, inserted) in enumerate([("5M2D5M", ""), ("5M2D5M", ""), ("5M1I5M", "T"), ("5M1I5M", "T"), ("5M1I5M", "G")])]
    return _case(records, min_alt=2, min_percent=20)


HOT = [("i1", 15, 1, ""), ("i1", 17, 1, ""), ("i1", 36, 2, "CA"), ("i1", 38, 2, "AC"), ("i1", 50, 1, ""), ("i1", 90, 1, "G"), ("chr2", 4, 1, ""), ("chr2", 30, 3, "")]  # (contig, 0-based start, size, inserted bases or "" for a deletion)


def seeded_case(assembly, seed=2200, n=2000):
    """2 000 records on i1 and chr2, about a third of them with an insertion or a deletion of one to four bases -- many inside the repeats, where they move --, some with two, some
    clipped, some that the filter drops, and a few events that many records share (HOT: placed at different ends of a repeat, they meet at one anchor); min_alt 3 and 2 percent"""
    generator = random.Random(seed)
    records = []
    for t in range(n):
        contig = generator.choice(("i1", "i1", "i1", "chr2"))
        length_of = dict(HEADER)[contig]
        length = generator.randint(20, 60 if contig == "i1" else 40)
        pos = generator.randint(1, max(1, length_of - length + generator.randint(0, 4)))
        cigar, inserted = "%dM" % length, ""
        hot = [(point - (pos - 1), size, bases) for name, point, size, bases in HOT if name == contig and pos - 1 + 2 <= point <= pos - 1 + length - 3 - size]
        if hot and generator.random() < 0.3:  # an event many records share, placed where the read happens to show it
            point, size, bases = generator.choice(hot)
            cigar, inserted = "%dM%d%s%dM" % (point, size, "I" if bases else "D", length - point), bases
        elif generator.random() < 0.35:
            cut = sorted(generator.sample(range(2, length - 2), 2 if generator.random() < 0.2 else 1))
            cigar, before = "", 0
            for point in cut:
                size = generator.randint(1, 4)
                if generator.random() < 0.5:
                    cigar += "%dM%dI" % (point - before, size)
                    inserted += "".join(generator.choice("ACGTTTAAN" if generator.random() < 0.05 else "ACGT") for _ in range(size)) if generator.random() < 0.5 else "".join(ref_base(assembly, contig, pos - 1 + point - size + j).replace("N", "A") for j in range(size))
                else:
                    cigar += "%dM%dD" % (point - before, size)
                before = point
            cigar += "%dM" % (length - before)
        if generator.random() < 0.1:
            cigar = "%dS" % generator.randint(1, 5) + cigar
        records.append(read(assembly, "s%04d" % t, contig, pos, cigar, inserted, flag=generator.choice((0, 0, 0, 16, 99, 147, 2048, 1024, 256)), mapq=generator.choice((0, 19, 20, 60, 60, 255))))
    return _case(records, min_percent=2)


def no_records_case(assembly):
    return _case([])


def no_events_case(assembly):
    """records without an I or D: the header line alone"""
    return _case([read(assembly, "m%02d" % k, "i1" if k % 3 else "chr2", 1 + k % 30, "20M" if k % 2 else "8M30N8M") for k in range(40)], min_alt=1, min_percent=0)


def no_references_case(assembly):
    return _case([], references=[])


MADE = {"wave_1": wavefront_case(1), "wave_63": wavefront_case(63), "wave_64": wavefront_case(64), "wave_65": wavefront_case(65), "wave_129": wavefront_case(129), "insertions": insertions_case,
        "normalisation": normalisation_case, "capped": capped_case, "edges": edges_case, "filters": filters_case, "support": support_case, "seeded": seeded_case, "no_records": no_records_case,
        "no_events": no_events_case, "no_references": no_references_case}
