"""What tests/test_splice_junctions.py shares with tools/: a restatement of the rule of --splice-junctions in plain Python -- lists of tokens per CIGAR, dicts by
junction and sets of read names, no sort of tuples, no table --, and the cases that are made at test time on the committed annotation and assembly
(tests/golden/splice_junctions/hand_made.{gtf,fa}).  It is written from the rule, not from junction_core.hpp, and shares no code with the project; it is the independent side for
inputs made at test time only because it gives tests/golden/splice_junctions/hand_made.tab, which a reader can check by eye, from hand_made.sam.  The SAM reader and the BAM writer
are those of tests/gene_counts_lib.py, and so is the form of a case: (references, records), references a list of (name, LN), records a list of
(qname, flag, rname or "*", 1-based pos, cigar text or "*", tags)."""
import os
import random
import re
import struct

from gene_counts_lib import bam_header, bam_records, nh_of, parse_sam, sam_text, stream_pipeline, write_bgzf  # noqa: F401 (the containers, for the tests)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "splice_junctions")
COMMITTED_CONTIGS = "j1 j2 j3"
HEADER = [("j2", 100), ("j1", 600), ("orphan", 5000), ("j3", 300)]  # of the committed case: not the order of the assembly; j3 is longer than the assembly has it; orphan is not in it
MOTIFS = {("GT", "AG"): 1, ("CT", "AC"): 2, ("GC", "AG"): 3, ("CT", "GC"): 4, ("AT", "AC"): 5, ("GT", "AT"): 6}
COUNTED = ("records", "contributing", "crossings", "pairs", "junctions", "annotated")


def load_annotation(gtf=os.path.join(GOLDEN, "hand_made.gtf"), fasta=os.path.join(GOLDEN, "hand_made.fa")):
    """-> {"sequences": contig -> bases in upper case, "introns": (contig, s, e) -> set of "+" / "-": the room between an exon and the next exon of its transcript, 0-based closed,
    with the strands of the genes that have it}.  Only GTFs of the kind the fixtures promise are read: that is asserted."""
    sequences, name = {}, None
    for line in open(fasta):
        if line.startswith(">"):
            name = line[1:].strip()
            sequences[name] = ""
        else:
            sequences[name] += line.strip().upper()
    transcripts, strand_of = {}, {}
    for line in open(gtf):
        if not line.strip() or line.startswith("#"):
            continue
        fields = line.rstrip("\n").split("\t")
        assert len(fields) == 9 and fields[2] == "exon" and fields[6] in "+-", line
        attributes = dict(re.findall(r'(\w+) "([^"]*)"', fields[8]))
        assert fields[0] in sequences and 1 <= int(fields[3]) <= int(fields[4]) <= len(sequences[fields[0]]), line
        key = (attributes["gene_id"], attributes["transcript_id"], fields[0])
        assert strand_of.setdefault(attributes["gene_id"], fields[6]) == fields[6], line
        transcripts.setdefault(key, []).append((int(fields[3]) - 1, int(fields[4]) - 1))  # GTF is 1-based closed
    introns = {}
    for (gene, _, contig), exons in transcripts.items():
        exons.sort()
        for (_, end), (start, _) in zip(exons, exons[1:]):
            assert end + 1 <= start - 1, "the exons of a transcript of the fixtures neither touch nor overlap"
            introns.setdefault((contig, end + 1, start - 1), set()).add(strand_of[gene])
    return {"sequences": sequences, "introns": introns}


# ---- the rule -------------------------------------------------------------------------------------------------------------------------------------------------------

def junctions_of(pos, cigar, length):
    """the kept introns of a CIGAR walked from 0-based pos on a reference of `length` bases: [(s, e, overhang)]"""
    tokens, at = [], pos  # ("m", bases) / ("n", s, e) / ("d",): what I, S, H and P leave of the CIGAR
    for count, op in ([] if cigar == "*" else re.findall(r"(\d+)([MIDNSHP=X])", cigar)):
        count = int(count)
        if op in "M=X":
            tokens.append(("m", count))
        elif op == "N" and count >= 1:
            if tokens and tokens[-1][0] == "n":  # nothing but I, S, H and P between them: one intron
                tokens[-1] = ("n", tokens[-1][1], at + count - 1)
            else:
                tokens.append(("n", at, at + count - 1))
        elif op == "D":
            tokens.append(("d",))
        if op in "M=XDN":
            at += count
    kept = []
    for k, token in enumerate(tokens):
        if token[0] != "n":
            continue
        left = right = 0
        for before in reversed(tokens[:k]):
            if before[0] == "n":
                break
            left += before[1] if before[0] == "m" else 0
        for behind in tokens[k + 1:]:
            if behind[0] == "n":
                break
            right += behind[1] if behind[0] == "m" else 0
        if left > 0 and right > 0 and 0 <= token[1] and token[2] < length:
            kept.append((token[1], token[2], min(left, right)))
    return kept


def restate(annotation, case):
    """-> (text of the file, {"records", "contributing", "crossings", "pairs", "junctions", "annotated"})"""
    references, records = case
    index_of, length_of = {name: k for k, (name, _) in enumerate(references)}, dict(references)
    templates, overhang = {}, {}  # (reference index, s, e) -> {qname: multimapping}; -> the largest overhang
    stats = {"records": len(records), "contributing": 0, "crossings": 0}
    for qname, flag, rname, pos, cigar, tags in records:
        if flag & 4 or flag & 0x800 or rname not in index_of or pos - 1 < 0:
            continue
        stats["contributing"] += 1
        for s, e, least in junctions_of(pos - 1, cigar, length_of[rname]):
            stats["crossings"] += 1
            key = (index_of[rname], s, e)
            crossed = templates.setdefault(key, {})
            crossed[qname] = crossed.get(qname, False) or nh_of(tags) > 1
            overhang[key] = max(overhang.get(key, 0), least)
    lines, annotated = [], 0
    for key in sorted(templates):
        name, s, e = references[key[0]][0], key[1], key[2]
        bases = annotation["sequences"].get(name, "")
        motif = MOTIFS.get((bases[s:s + 2], bases[e - 1:e + 1]), 0) if e - s + 1 >= 4 and e < len(bases) else 0
        strands = annotation["introns"].get((name, s, e), set())
        annotated += 1 if strands else 0
        strand = (1 if motif % 2 else 2) if motif else 1 if strands == {"+"} else 2 if strands == {"-"} else 0
        multimapping = sum(1 for is_multimapping in templates[key].values() if is_multimapping)
        lines.append("%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\n" % (name, s + 1, e + 1, strand, motif, 1 if strands else 0, len(templates[key]) - multimapping, multimapping, overhang[key]))
    stats.update({"pairs": sum(len(crossed) for crossed in templates.values()), "junctions": len(templates), "annotated": annotated})
    return "".join(lines).encode(), stats


# ---- cases made at test time ------------------------------------------------------------------------------------------------------------------------------------------

def known_introns(annotation):
    """the introns of j1 a seeded input aims at: the annotated ones and the six motifs of the committed assembly, sorted; none overlaps another"""
    found = set((s, e) for (contig, s, e) in annotation["introns"] if contig == "j1") | set([(60, 79), (140, 159), (180, 199), (220, 239), (430, 433)])
    return sorted(found)


def _tags(generator):
    choice = generator.random()
    if choice < 0.55:
        return []
    if choice < 0.7:
        return [("NH", "C", 1)]
    kind = generator.choice("cCsSiIZ")
    value = {"c": generator.choice((-1, 1, 2, 127)), "C": generator.choice((0, 1, 2, 255)), "s": generator.choice((-300, 1, 300)), "S": generator.choice((1, 300)),
             "i": generator.choice((-70000, 1, 70000)), "I": generator.choice((1, 70000)), "Z": "7"}[kind]
    front = generator.choice(([], [("XZ", "Z", "some text")], [("XB", "B", ("s", [1, -2, 3]))], [("XA", "C", 9), ("XB", "B", ("I", []))]))
    return front + [("NH", kind, value)] + generator.choice(([], [("HI", "C", 1)]))


def random_case(seed, annotation=None, max_records=400):
    """at most 400 records under the committed header: most reads cross one to three of the known introns of j1 in a row with small overhangs, so that junctions are shared by many
    templates; introns are written as one N, as two with an insertion between them, with a deletion or an insertion beside them; reads begin or end with N, carry = and X, clips
    and padding; others lie anywhere, on every reference of the header, also around its end.  Templates are single reads, pairs whose mates often cross the same junction,
    reads with secondary and supplementary company, unmapped reads; a part carries NH in every type, behind other fields or as text; a part of the mates is moved to the end"""
    annotation = annotation or load_annotation()
    generator = random.Random(seed)
    known, length_of = known_introns(annotation), dict(HEADER)

    def matched(bases):
        if bases > 2 and generator.random() < 0.15:
            cut = generator.randint(1, bases - 1)
            return "%d=%dX" % (cut, bases - cut)
        return "%dM" % bases

    def intron(bases):
        choice = generator.random()
        if choice < 0.1 and bases >= 2:
            cut = generator.randint(1, bases - 1)
            return "%dN%d%s%dN" % (cut, generator.randint(1, 3), generator.choice("IPS"), bases - cut)
        return "%dN" % bases

    def aimed():
        first = generator.randrange(len(known))
        count = min(generator.choice((1, 1, 1, 2, 3)), len(known) - first)
        left = generator.choice((0, 1, 2, 3, 5, 8, 12)) if generator.random() < 0.9 else 0
        ops, before = [], left
        if generator.random() < 0.15:
            ops.append("%d%s" % (generator.randint(1, 5), generator.choice("SH")))
        if left:
            ops.append(matched(left))
        if left and generator.random() < 0.1:
            gap = generator.randint(1, 2)
            ops.append("%dD" % gap)
            before += gap
        if generator.random() < 0.1:
            ops.append("%dI" % generator.randint(1, 3))
        for k in range(first, first + count):
            s, e = known[k]
            ops.append(intron(e - s + 1))
            if k + 1 < first + count:
                ops.append(matched(known[k + 1][0] - e - 1))
        if generator.random() < 0.1:
            ops.append("%dI" % generator.randint(1, 3))
        if generator.random() < 0.92:
            ops.append(matched(generator.choice((1, 2, 3, 5, 8, 12))))
        if generator.random() < 0.15:
            ops.append("%dS" % generator.randint(1, 5))
        return "j1", known[first][0] - before + 1, "".join(ops)

    def anywhere():
        contig = generator.choice(HEADER)[0]
        if generator.random() < 0.5:
            pos = generator.randint(1, length_of[contig])
        else:
            pos = max(1, length_of[contig] - generator.randint(-5, 60))  # around the end of the reference, also behind it
        ops = []
        for piece in range(generator.choice((1, 2, 2, 3, 4))):
            if piece:
                ops.append("%d%s" % (generator.choice((1, 3, 4, 10, 20, generator.randint(1, 60))), generator.choice("NNNNDIP")))
            ops.append(matched(generator.choice((1, 5, 20, generator.randint(1, 30)))))
        return contig, pos, "".join(ops)

    def alignment():
        contig, pos, cigar = aimed() if generator.random() < 0.75 else anywhere()
        return contig, max(1, pos), cigar

    records, late, t = [], [], 0
    while len(records) + len(late) < max_records - 6:
        qname = "t%d_%d" % (seed, t)
        t += 1
        kind = generator.random()
        if kind < 0.35:  # a single read
            records.append((qname, generator.choice((0, 16, 1024, 512)),) + alignment() + (_tags(generator),))
        elif kind < 0.75:  # a pair; the second mate often lies where the first does
            first = alignment()
            second = first if generator.random() < 0.4 else alignment()
            flags = generator.choice(((99, 147), (83, 163), (65, 129)))
            mates = [(qname, flags[0]) + first + (_tags(generator),), (qname, flags[1]) + second + (_tags(generator),)]
            if generator.random() < 0.1:  # one mate unmapped, with the place and the CIGAR of the other
                mates[1] = (qname, (flags[1] & ~0x32) | 4) + first + ([],)
            if generator.random() < 0.5:
                mates.reverse()
            records.append(mates[0])
            (late if generator.random() < 0.2 else records).append(mates[1])
        elif kind < 0.8:  # unmapped
            records.append((qname, 4, "*", 0, "*", []))
        else:  # a read with company: secondary, supplementary, a second primary; the company often lies where the read does
            first = alignment()
            records.append((qname, generator.choice((0, 16)),) + first + (_tags(generator),))
            for _ in range(generator.randint(1, 3)):
                (late if generator.random() < 0.3 else records).append((qname, generator.choice((256, 272, 2048, 2064, 0)),) + (first if generator.random() < 0.5 else alignment()) + (_tags(generator),))
    generator.shuffle(late)
    return list(HEADER), records + late


def hot_case():
    """70 001 templates over 20..39 of j1 -- a count above 2^16 on one row --, every seventh with a second mate over it and every thousandth multimapping, then a wavefront's
    worth over the next two junctions"""
    records = []
    for k in range(70001):
        tags = [("NH", "C", 4)] if k % 1000 == 999 else []
        if k % 7 == 0:
            records += [("h%05d" % k, 99, "j1", 11, "10M20N%dM" % (1 + k % 9), tags), ("h%05d" % k, 147, "j1", 16, "5M20N7M", [])]
        else:
            records.append(("h%05d" % k, 0, "j1", 11, "10M20N%dM" % (1 + k % 9), tags))
    records += [("w%02d" % k, 16 if k & 4 else 0, "j1", (51, 131)[k % 2], "10M20N10M", []) for k in range(64)]
    return list(HEADER), records


def wavefront_case():
    """65 templates, one past a wavefront, over one junction, the last one multimapping"""
    return list(HEADER), [("v%02d" % k, 0, "j1", 51, "10M20N%dM" % (1 + k % 11), [("NH", "C", 2)] if k == 64 else []) for k in range(65)]


def long_cigar_case():
    """one record with 300 N operations on orphan (601 operations), between records that have none and records that have one: every place of the scan is used"""
    long_one = ("long", 0, "orphan", 101, "2M" + "3N2M" * 300, [])
    plain = [("p%d" % k, 0, "j1", 1 + k, "30M", []) for k in range(70)]
    spliced = [("s%d" % k, 0, "j1", 51, "10M20N10M", []) for k in range(5)]
    return list(HEADER), plain[:40] + spliced[:2] + [long_one] + plain[40:] + spliced[2:] + [("long", 256, "orphan", 101, "2M3N2M", [("NH", "C", 2)])]


def aux_case():
    """the corners of the NH walk of DESIGN.md 4.15, every read over 60..79 of j1: NH:Z in front of NH:i (the first field named NH decides: 1); a B array that announces more
    elements than the record holds, a field of an unknown type and a Z field without its NUL in front of NH:i:5 (the walk ends there: 1); NH:i:5 alone and behind a well-formed B
    array (multimapping)"""
    five = ("NH", "C", 5)
    tags = [[("NH", "Z", "9"), five], [("XB", "raw", b"Bs" + struct.pack("<I", 1000) + b"\1\0"), five], [("XQ", "raw", b"?\7"), five], [("XZ", "raw", b"Zno end")],
            [five], [("XB", "B", ("s", [1, 2])), five]]
    return list(HEADER), [("x%d" % k, 0, "j1", 51, "10M20N10M", fields) for k, fields in enumerate(tags)]


def no_n_case():
    """the committed case with every N turned into D: the same records and names, no junction"""
    references, records = parse_sam(open(os.path.join(GOLDEN, "hand_made.sam"), "rb").read())
    return references, [record[:4] + (record[4].replace("N", "D"),) + record[5:] for record in records]


def no_records_case():
    """a header and nothing behind it"""
    return list(HEADER), []


def empty_case():
    """no reference and no record"""
    return [], []
