"""What tests/test_variant_sites.py needs beside the project: a restatement of the rule of --variant-sites in plain Python -- a dict by (reference, position) with
eight counters and four event counts, a loop over every base of every CIGAR operation, no sort, no search, no key --, and the cases that are made at test time on the committed
assembly (tests/golden/allele_counts/hand_made.{fa,gtf}).  It is written from the rule, not from variant_core.hpp, and shares no code with the project; it is the independent side
for inputs made at test time only because it gives tests/golden/variant_sites/hand_made.tsv, which a reader can check by eye, from hand_made.sam.

A case is a dict: "references" a list of (name, LN); "records" as in allele_counts_lib (qname, flag, rname or "*", 1-based pos, mapq, cigar text or "*", seq, qual); "min_mapq",
"min_baseq", "min_alt", "min_percent"."""
import os
import random
import re

from allele_counts_lib import COMMITTED_CONTIGS, HEADER, bam_header, bam_records, load_assembly, parse_sam, qualities, stream_pipeline, write_bgzf  # noqa: F401 (the record writer and the containers)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "variant_sites")
ALLELE_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "allele_counts")
HEADER_LINE = "#CONTIG\tPOS\tREF\tALT\tA\tC\tG\tT\tN\tDEL\tSKIP\tLOWQ\n"
COUNTED = ("records", "contributing", "events", "runs", "candidates", "reported")
COMMITTED_THRESHOLDS = {"min_mapq": 20, "min_baseq": 13, "min_alt": 2, "min_percent": 50}
DEFAULTS = {"min_mapq": 20, "min_baseq": 13, "min_alt": 3, "min_percent": 5}


def committed_case():
    case = parse_sam(open(os.path.join(GOLDEN, "hand_made.sam"), "rb").read())
    del case["sites"]
    case.update(COMMITTED_THRESHOLDS)
    return case


# ---- the rule -------------------------------------------------------------------------------------------------------------------------------------------------------

def counts(record, min_mapq):
    """rule 1"""
    qname, flag, rname, pos, mapq, cigar, seq, qual = record
    if flag & (0x4 | 0x100 | 0x200 | 0x400) or rname == "*" or mapq < min_mapq or cigar == "*" or seq == "*":
        return False
    return sum(int(length) for length, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar) if op in "MIS=X") == len(seq)


def ref_base(assembly, reference, position):
    """REF at a 0-based position of a reference of the header: upper case, N where the assembly holds nothing"""
    bases = assembly.get(reference[3:] if reference.startswith("chr") else reference, "")
    return bases[position].upper() if position < len(bases) else "N"


def restate(assembly, case):
    """-> (text of the file, {"records", "contributing", "events", "runs", "candidates", "reported"})"""
    references = case["references"]
    index_of = {name: k for k, (name, _) in enumerate(references)}
    table, support = {}, {}  # (reference, position) -> eight counters; -> events by A, C, G, T
    contributing = 0
    for record in case["records"]:
        if record[2] != "*" and record[2] not in index_of or not counts(record, case["min_mapq"]):
            continue
        contributing += 1
        qname, flag, rname, pos, mapq, cigar, seq, qual = record
        quals, at, i, length = qualities(qual, len(seq)), pos - 1, 0, dict(references)[rname]
        for count, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar):
            for _ in range(int(count)):
                if op in "M=XDN" and 0 <= at < length:
                    row = table.setdefault((index_of[rname], at), [0] * 8)
                    if op == "D":
                        row[5] += 1
                    elif op == "N":
                        row[6] += 1
                    elif quals[i] < case["min_baseq"]:
                        row[7] += 1
                    elif seq[i] not in "ACGT":
                        row[4] += 1
                    else:
                        row["ACGT".index(seq[i])] += 1
                        reference = ref_base(assembly, rname, at)
                        if reference in "ACGT" and reference != seq[i]:  # rule 2: a mismatch event
                            support.setdefault((index_of[rname], at), [0] * 4)["ACGT".index(seq[i])] += 1
                at += 1 if op in "M=XDN" else 0
                i += 1 if op in "M=XIS" else 0
    lines, candidates, reported = [HEADER_LINE], 0, 0
    for index, (name, length) in enumerate(references):  # rule 7: by reference in header order, then by position
        for position in range(length):
            events = support.get((index, position))
            if events is None or max(events) < case["min_alt"]:  # rule 4
                continue
            candidates += 1
            row = table[(index, position)]
            depth = row[0] + row[1] + row[2] + row[3]
            alts = [base for base, number in zip("ACGT", events) if number >= case["min_alt"] and number * 100 >= case["min_percent"] * depth]  # rule 6
            assert all(number == 0 or number == row[k] for k, number in enumerate(events))
            if alts:
                reported += 1
                lines.append("%s\t%d\t%s\t%s\t%s\n" % (name, position + 1, ref_base(assembly, name, position), ",".join(alts), "\t".join(str(number) for number in row)))
    stats = {"records": len(case["records"]), "contributing": contributing, "events": sum(sum(events) for events in support.values()),
             "runs": sum(sum(1 for number in events if number) for events in support.values()), "candidates": candidates, "reported": reported}
    return "".join(lines).encode(), stats


def sites_of(text):
    """the sites file of --allele-counts for the lines of a table, and what --allele-counts must print for them: the table without its ALT column"""
    rows = [line.split("\t") for line in text.decode().split("\n")[1:-1]]
    sites = "".join("%s\t%s\n" % (row[0], row[1]) for row in rows).encode()
    expected = "#CONTIG\tPOS\tREF\tA\tC\tG\tT\tN\tDEL\tSKIP\tLOWQ\n" + "".join("\t".join(row[:3] + row[4:]) + "\n" for row in rows)
    return sites, expected.encode()


# ---- cases made at test time ------------------------------------------------------------------------------------------------------------------------------------------

def _case(records, references=None, **thresholds):
    case = {"references": list(HEADER if references is None else references), "records": records}
    case.update(DEFAULTS)
    case.update(thresholds)
    return case


def _other(base, k=0):
    return [b for b in "ACGT" if b != base][k % 3]


def _read(assembly, name, contig, pos, length, subs=(), cigar=None, front="", qual=None, flag=0, mapq=30, alt=0):
    """a read of `length` aligned bases that shows the assembly from 1-based `pos` on (N where the assembly holds nothing), with another base at the offsets of `subs` (a dict
    gives the base); `front`: bases in front of them (for S and I the caller writes the CIGAR)"""
    bases = [ref_base(assembly, contig, pos - 1 + j) if pos - 1 + j >= 0 else "A" for j in range(length)]
    for offset in subs:
        bases[offset] = subs[offset] if isinstance(subs, dict) else _other(bases[offset] if bases[offset] in "ACGT" else "A", alt)
    seq = front + "".join(bases)
    return (name, flag, contig, pos, mapq, cigar or "%dM" % length, seq, "I" * len(seq) if qual is None else qual)


def lanes_case(assembly):
    """l_seq of 1, 63, 64, 65, 128 and 129 (the longer ones behind a soft clip: a1 has 100 bases), a mismatch at the first and the last base of every record and at lanes 0, 63
    and 64 of a block; an odd l_seq; a soft clip of odd length; a block that begins at read index 40; an I between two M; = and X; every event is a candidate (min_alt 1)"""
    records = []
    for l_seq in (1, 63, 64, 65, 128, 129):
        aligned = min(l_seq, 100)
        clip = l_seq - aligned
        subs = sorted(set(j for j in (0, 63, 64, aligned - 1) if j < aligned))
        records.append(_read(assembly, "l%d" % l_seq, "a1", 1, aligned, subs, cigar=("%dS" % clip if clip else "") + "%dM" % aligned, front="ACGTN"[l_seq % 5] * clip, alt=l_seq))
    records.append(_read(assembly, "odd7", "a1", 3, 7, [0, 6]))
    records.append(_read(assembly, "clip3", "a1", 12, 10, [0, 1, 9], cigar="3S10M", front="TTT"))
    records.append(_read(assembly, "at40", "a1", 31, 50, [0, 23, 24, 49], cigar="40S50M", front="G" * 40))
    inserted = _read(assembly, "ins", "a1", 5, 60, [0, 39, 40, 59])
    records.append(inserted[:5] + ("40M5I20M", inserted[6][:40] + "CCCCC" + inserted[6][40:], "I" * 65))
    records.append(_read(assembly, "eqx", "chr2", 3, 25, [10, 12, 14], cigar="10=5X10="))
    records.append(_read(assembly, "eqx2", "chr2", 3, 25, [0, 24], cigar="10=5X10=", alt=1))
    return _case(records, min_alt=1, min_percent=0)


def edges_case(assembly):
    """a block cut at LN; POS 0 (position -1); orphan, which the assembly lacks; lower-case bases of the assembly (a1 21..30); N in the assembly (a1 55); N and an ambiguity code
    in the read over a base, and a base over them"""
    records = [_read(assembly, "cut%d" % k, "a1", 95, 10, {3: "A", 5: "C", 6: "G", 9: "T"}) for k in range(2)]
    records += [_read(assembly, "cut2", "chr2", 48, 8, [0, 2, 3, 7])]
    records += [_read(assembly, "neg%d" % k, "a1", 0, 10, [0, 1, 2]) for k in range(2)]
    records += [_read(assembly, "orphan%d" % k, "orphan", 10 + k, 30, {j: "ACGT"[(j + k) % 4] for j in range(30)}) for k in range(3)]
    records += [_read(assembly, "lower%d" % k, "a1", 18, 16, [3, 4, 8, 12]) for k in range(2)]
    records += [_read(assembly, "overn%d" % k, "a1", 52, 8, {3: "ACGT"[k], 4: "ACGT"[k]}) for k in range(4)]
    records += [_read(assembly, "iupac%d" % k, "a1", 61, 12, {2: "N", 3: "R", 4: "=", 5: "Y", 6: _other("C", k)}) for k in range(3)]
    return _case(records, min_alt=1, min_percent=0)


def long_header_case(assembly):
    """a header whose a1 is longer (LN 150) than the contig of the assembly (100 bases): REF is N behind it, and a block of 129 bases runs over the end of the assembly"""
    records = [_read(assembly, "long%d" % k, "a1", 11, 129, {0: "T", 63: "A", 64: "C", 89: "G", 90: "A", 128: "C"}) for k in range(3)]
    records += [_read(assembly, "behind%d" % k, "a1", 101, 50, {j: "ACGT"[j % 4] for j in range(50)}) for k in range(3)]
    return _case(records, references=[("a1", 150), ("chr2", 50), ("orphan", 700)], min_alt=1, min_percent=0)


def filters_case(assembly):
    """each excluded flag; MAPQ one below the threshold and at it; a quality one below min_baseq at a mismatch (no event, one LOWQ) and at it; quality 0xFF; no SEQ; an l_seq that
    disagrees with the CIGAR; a supplementary record counts"""
    records = [_read(assembly, "flag%d" % flag, "a1", 31, 10, [2], flag=flag) for flag in (0x4, 0x100, 0x200, 0x400, 0x704, 0x800, 0x10)]
    records += [_read(assembly, "mapq%d" % mapq, "a1", 41, 10, [2], mapq=mapq) for mapq in (19, 20, 19, 255, 0)]
    records += [_read(assembly, "q12", "chr2", 1, 10, [4], qual=b"\x28" * 4 + b"\x0c" + b"\x28" * 5), _read(assembly, "q13", "chr2", 1, 10, [4], qual=b"\x28" * 4 + b"\x0d" + b"\x28" * 5),
                _read(assembly, "q255", "chr2", 1, 10, [4, 5], qual="*"), _read(assembly, "q0", "chr2", 1, 10, [5], qual=bytes(10))]
    records += [("noseq", 0, "chr2", 11, 30, "10M", "*", "*")]
    disagrees = _read(assembly, "short", "chr2", 11, 9, [3])
    records += [disagrees[:5] + ("10M",) + disagrees[6:], _read(assembly, "agrees", "chr2", 11, 10, [3])]
    return _case(records, min_alt=1, min_percent=0)


def counting_case(assembly):
    """200 supporting records in a row over a1 50 (several wavefronts of the counter kernel, one run); at a1 10, 12 and 14 (min_alt 3) two and three alts of which two, one and none
    pass (three of three at a1 70, 71 and 72); support of min_alt - 1 (a1 20) and of min_alt (a1 21); a D and an N over the candidate a1 50; candidates in neighbouring positions (a1 70, 71, 72) and on two references"""
    records = [_read(assembly, "hot%03d" % k, "a1", 46 + k % 5, 10, {50 - (46 + k % 5): "G"}) for k in range(200)]
    records += [_read(assembly, "del%d" % k, "a1", 47, 6, cigar="3M1D3M") for k in range(2)] + [_read(assembly, "skip", "a1", 48, 4, cigar="2M1N2M")]
    for k, (at10, at12, at14) in enumerate([("A", "A", "A"), ("A", "A", "A"), ("A", "A", "C"), ("T", "A", "C"), ("T", "C", "G"), ("T", "C", "G"), ("C", "G", "T"), ("C", "T", "T")]):
        records.append(_read(assembly, "alts%d" % k, "a1", 8, 10, {2: at10, 4: at12, 6: at14}))  # REF a1 10 = C, 12 = T, 14 = C: a base equal to REF is no event
    records += [_read(assembly, "two%d" % k, "a1", 18, 6, {2: "A"} if k < 2 else {3: "T"}) for k in range(5)]  # a1 20 (REF T): 2 x A; a1 21 (REF a): 3 x T
    records += [_read(assembly, "row%d" % k, "a1", 66, 10, {4: "ACGT"[k % 4], 5: "ACGT"[(k + 1) % 4], 6: "ACGT"[(k + 2) % 4]}) for k in range(12)]
    records += [_read(assembly, "two_refs%d" % k, "chr2", 20, 10, [0, 1, 2]) for k in range(4)]
    return _case(records)


def percent_case(assembly):
    """min_percent 5 with min_alt 1: one of 20 passes (a1 10), one of 21 does not (a1 70); one of one does (chr2 5)"""
    records = [_read(assembly, "a%02d" % k, "a1", 8, 5, [2] if k == 0 else []) for k in range(20)]
    records += [_read(assembly, "b%02d" % k, "a1", 68, 5, [2] if k == 7 else []) for k in range(21)]
    records += [_read(assembly, "c", "chr2", 3, 5, [2])]
    return _case(records, min_alt=1, min_percent=5)


def seeded_case(assembly, seed=2100, n=2000):
    """about 2 000 records on a1 and chr2 with about 1 % substitutions (most of them at a few positions, so that sites pass), some low qualities, I, D, N and S, some records that
    the filter drops; the default thresholds"""
    generator = random.Random(seed)
    hot = {("a1", 17): "G", ("a1", 44): "C", ("a1", 45): "A", ("a1", 83): "T", ("chr2", 25): "C", ("chr2", 26): "T"}
    records = []
    for t in range(n):
        contig = generator.choice(("a1", "a1", "a1", "chr2"))
        length_of = dict(HEADER)[contig]
        length = generator.randint(20, 100 if contig == "a1" else 45)
        pos = generator.randint(1, max(1, length_of - length + generator.randint(0, 6)))
        subs = {}
        for j in range(length):
            site = (contig, pos + j)
            if site in hot and generator.random() < 0.3:
                subs[j] = hot[site]
            elif generator.random() < 0.004:
                subs[j] = generator.choice("ACGTN")
        record = _read(assembly, "s%04d" % t, contig, pos, length, subs, flag=generator.choice((0, 0, 0, 16, 99, 147, 2048, 1024, 256)), mapq=generator.choice((0, 19, 20, 60, 60, 255)))
        kind, seq = generator.random(), record[6]
        if kind < 0.1 and length > 12:  # an insertion of three bases behind the first five, a deletion or a skip behind the next five
            cigar = "5M3I%dM" % (length - 5) if kind < 0.04 else "5M%d%s%dM" % (generator.randint(1, 4), "D" if kind < 0.07 else "N", length - 5)
            if kind >= 0.04:  # (the bases behind the gap show the assembly behind it)
                gap = int(cigar[2])
                seq = seq[:5] + "".join(ref_base(assembly, contig, pos - 1 + 5 + gap + j) for j in range(length - 5))
            else:
                seq = seq[:5] + "GCA" + seq[5:]
            record = record[:5] + (cigar, seq, "I" * len(seq))
        elif kind < 0.2:
            clip = generator.randint(1, 9)
            record = record[:5] + ("%dS%s" % (clip, record[5]), "T" * clip + seq, "I" * (clip + len(seq)))
        if generator.random() < 0.2:
            record = record[:7] + (bytes(generator.choice((2, 12, 13, 30, 40, 40, 40)) for _ in record[6]),)
        records.append(record)
    return _case(records)


def no_records_case(assembly):
    return _case([])


def no_mismatch_case(assembly):
    """records that show the assembly: the header line alone"""
    return _case([_read(assembly, "m%02d" % k, "a1" if k % 3 else "chr2", 1 + k % 30, 20) for k in range(40)], min_alt=1, min_percent=0)


def no_references_case(assembly):
    return _case([], references=[])


MADE = {"lanes": lanes_case, "edges": edges_case, "long_header": long_header_case, "filters": filters_case, "counting": counting_case, "percent": percent_case, "seeded": seeded_case,
        "no_records": no_records_case, "no_mismatch": no_mismatch_case, "no_references": no_references_case}
