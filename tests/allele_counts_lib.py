"""What tests/test_allele_counts.py shares with tools/: a restatement of the rule of --allele-counts in plain Python -- a dict by (reference, position) with a list
of eight numbers, a loop over every base of every CIGAR operation, no sort, no search, no bitmap --, a writer of BAM records with real SEQ and QUAL, and the cases that are made at
test time on the committed assembly (tests/golden/allele_counts/hand_made.{fa,gtf}).  It is written from the rule, not from allele_core.hpp, and shares no code with the project;
it is the independent side for inputs made at test time only because it gives tests/golden/allele_counts/hand_made.tsv, which a reader can check by eye, from hand_made.sam and
hand_made.sites.

A case is a dict: "references" a list of (name, LN); "records" a list of (qname, flag, rname or "*", 1-based pos, mapq, cigar text or "*", seq, qual) -- seq a text over
"=ACMGRSVTWYHKDBN", "*" for none; qual a text of SAM quality characters, "*" for none (every byte 0xFF), or bytes with the values themselves --; "sites" the bytes of the sites
file; "min_mapq" and "min_baseq"."""
import os
import random
import re
import struct

from splice_junctions_lib import bam_header, stream_pipeline, write_bgzf  # noqa: F401 (the containers, for the tests)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "allele_counts")
COMMITTED_CONTIGS = "a1 2"
HEADER = [("a1", 100), ("chr2", 50), ("orphan", 700)]  # of the committed case: chr2 is 2 in the assembly, orphan is not in it
COMMITTED_THRESHOLDS = (20, 13)  # --allele-min-mapq, --allele-min-baseq of the committed case
HEADER_LINE = "#CONTIG\tPOS\tREF\tA\tC\tG\tT\tN\tDEL\tSKIP\tLOWQ\n"
COLUMNS = ("A", "C", "G", "T", "N", "DEL", "SKIP", "LOWQ")
COUNTED = ("records", "contributing", "hits", "sites", "placed", "covered")
CODES = "=ACMGRSVTWYHKDBN"
CIGAR_OPS = "MIDNSHP=X"


def load_assembly(fasta=os.path.join(GOLDEN, "hand_made.fa")):
    """-> contig -> bases as the file has them"""
    sequences, name = {}, None
    for line in open(fasta):
        if line.startswith(">"):
            name = line[1:].strip()
            sequences[name] = ""
        else:
            sequences[name] += line.strip()
    return sequences


def parse_sam(text, min_mapq=COMMITTED_THRESHOLDS[0], min_baseq=COMMITTED_THRESHOLDS[1], sites=b""):
    references, records = [], []
    for line in text.decode().split("\n"):
        if line.startswith("@SQ\t"):
            fields = dict(field.split(":", 1) for field in line.split("\t")[1:])
            references.append((fields["SN"], int(fields["LN"])))
        elif line and not line.startswith("@"):
            f = line.split("\t")
            records.append((f[0], int(f[1]), f[2], int(f[3]), int(f[4]), f[5], f[9], f[10]))
    return {"references": references, "records": records, "sites": sites, "min_mapq": min_mapq, "min_baseq": min_baseq}


def committed_case():
    return parse_sam(open(os.path.join(GOLDEN, "hand_made.sam"), "rb").read(), sites=open(os.path.join(GOLDEN, "hand_made.sites"), "rb").read())


def qualities(qual, l_seq):
    """the quality bytes of a record as a list of numbers"""
    if isinstance(qual, bytes):
        return list(qual)
    return [0xFF] * l_seq if qual == "*" else [ord(c) - 33 for c in qual]


def bam_record(index_of, record):
    qname, flag, rname, pos, mapq, cigar, seq, qual = record
    ref = -1 if rname == "*" else index_of[rname]
    ops = [] if cigar == "*" else [(int(length), CIGAR_OPS.index(op)) for length, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]
    nibbles = [] if seq == "*" else [CODES.index(c) for c in seq]
    quals = qualities(qual, len(nibbles))
    assert len(quals) == len(nibbles), record
    body = struct.pack("<iiBBHHHiiii", ref, pos - 1, len(qname) + 1, mapq, 4680, len(ops), flag, len(nibbles), -1, -1, 0)
    body += qname.encode() + b"\0" + b"".join(struct.pack("<I", length << 4 | op) for length, op in ops)
    body += bytes((nibbles[i] << 4) | (nibbles[i + 1] if i + 1 < len(nibbles) else 0) for i in range(0, len(nibbles), 2)) + bytes(quals)
    return struct.pack("<i", len(body)) + body


def bam_records(case):
    index_of = {name: k for k, (name, _) in enumerate(case["references"])}
    return b"".join(bam_record(index_of, record) for record in case["records"])


# ---- the rule -------------------------------------------------------------------------------------------------------------------------------------------------------

def parse_sites(text):
    """-> [(contig as spelled, 1-based position)]; ValueError("line N") where the project refuses the file"""
    sites = []
    for number, line in enumerate(text.decode("latin-1").split("\n"), 1):
        if line == "" or line.startswith("#"):
            continue
        fields = line.split("\t")
        if len(fields) < 2 or fields[1] == "" or not all(c in "0123456789" for c in fields[1]) or not 1 <= int(fields[1]) <= 2 ** 31 - 1:
            raise ValueError("line %d" % number)
        sites.append((fields[0], int(fields[1])))
    return sites


def place(references, name, position):
    """the index of the reference a site lies on, or None"""
    names = [reference for reference, _ in references]
    for spelling in (name, name[3:] if name.startswith("chr") else "chr" + name):
        if spelling in names:
            index = names.index(spelling)
            return index if position <= references[index][1] else None
    return None


def counts(record, min_mapq):
    qname, flag, rname, pos, mapq, cigar, seq, qual = record
    if flag & (0x4 | 0x100 | 0x200 | 0x400) or rname == "*" or mapq < min_mapq or cigar == "*" or seq == "*":
        return False
    return sum(int(length) for length, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar) if op in "MIS=X") == len(seq)


def restate(assembly, case):
    """-> (text of the file, {"records", "contributing", "hits", "sites", "placed", "covered"})"""
    references, sites = case["references"], parse_sites(case["sites"])
    placed = [place(references, name, position) for name, position in sites]
    table = {(index, position - 1): [0] * 8 for index, (_, position) in zip(placed, sites) if index is not None}  # duplicate lines share a row
    index_of = {name: k for k, (name, _) in enumerate(references)}
    contributing = 0
    for record in case["records"]:
        if record[2] != "*" and record[2] not in index_of or not counts(record, case["min_mapq"]):
            continue
        contributing += 1
        qname, flag, rname, pos, mapq, cigar, seq, qual = record
        quals, at, i, length = qualities(qual, len(seq)), pos - 1, 0, dict(references)[rname]
        for count, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar):
            for _ in range(int(count)):
                row = table.get((index_of[rname], at)) if op in "M=XDN" and 0 <= at < length else None
                if row is not None:
                    if op == "D":
                        row[5] += 1
                    elif op == "N":
                        row[6] += 1
                    elif quals[i] < case["min_baseq"]:
                        row[7] += 1
                    else:
                        row["ACGT".index(seq[i]) if seq[i] in "ACGT" else 4] += 1
                at += 1 if op in "M=XDN" else 0
                i += 1 if op in "M=XIS" else 0
    lines, hits, covered = [HEADER_LINE], 0, 0
    for (name, position), index in zip(sites, placed):
        row = table[(index, position - 1)] if index is not None else [0] * 8
        if index is None:
            base = "."
        else:
            reference = references[index][0]
            bases = assembly.get(reference[3:] if reference.startswith("chr") else reference, "")
            base = bases[position - 1].upper() if position <= len(bases) else "N"
        lines.append("%s\t%d\t%s\t%s\n" % (name, position, base, "\t".join(str(number) for number in row)))
        hits += sum(row)
        covered += 1 if sum(row) else 0
    stats = {"records": len(case["records"]), "contributing": contributing, "hits": hits, "sites": len(sites), "placed": sum(1 for index in placed if index is not None), "covered": covered}
    return "".join(lines).encode(), stats


# ---- cases made at test time ------------------------------------------------------------------------------------------------------------------------------------------

def _case(records, sites, min_mapq=0, min_baseq=13, references=None):
    text = sites if isinstance(sites, bytes) else "".join("%s\t%d\n" % site for site in sites).encode()
    return {"references": list(HEADER if references is None else references), "records": records, "sites": text, "min_mapq": min_mapq, "min_baseq": min_baseq}


def random_case(seed, max_records=300):
    """at most 300 records under the committed header and some 70 sites: most reads lie on a1 or chr2, where the sites are dense, with M, =, X, I, D, N, S, H and P in any order,
    some beginning in front of the reference (POS 1 with a long clip does not: POS is never below 1) and many running past its end; SEQ holds the four bases, N, ambiguity codes
    and =; QUAL holds values around the threshold, 0xFF for the whole read or for single bases; flags, MAPQ, an empty SEQ and a CIGAR that disagrees with l_seq exercise the filter.
    The sites file has duplicates, names with and without chr, unplaced contigs, positions beyond LN, comment and empty lines and further fields; the thresholds vary by seed"""
    generator = random.Random(seed)
    min_mapq, min_baseq = generator.choice((0, 0, 20, 255)), generator.choice((0, 13, 13, 30, 255))
    length_of = dict(HEADER)
    records = []
    for t in range(generator.randint(max_records // 2, max_records)):
        contig = generator.choice(("a1", "a1", "a1", "chr2", "chr2", "orphan"))
        pos = generator.randint(1, length_of[contig] + 3) if generator.random() < 0.8 else max(1, length_of[contig] - generator.randint(0, 40))
        ops, l_seq = [], 0
        if generator.random() < 0.3:
            ops.append((generator.randint(1, 4), generator.choice("SH")))
        for piece in range(generator.choice((1, 1, 2, 3, 5))):
            if piece:
                ops.append((generator.choice((1, 2, 3, 10, generator.randint(1, 40))), generator.choice("IDNNDP")))
            ops.append((generator.choice((1, 2, 7, 20, generator.randint(1, 35))), generator.choice("MMMM=X")))
        if generator.random() < 0.3:
            ops.append((generator.randint(1, 4), generator.choice("SH")))
        l_seq = sum(count for count, op in ops if op in "MIS=X")
        kind = generator.random()
        if kind < 0.04:
            l_seq += generator.choice((-1, 1, 5))  # the CIGAR disagrees with l_seq
        seq = "".join(generator.choice("ACGT" * 6 + "N=RYKM") for _ in range(max(l_seq, 0))) or "*"
        if kind > 0.97:
            seq = "*"
        if seq == "*" or generator.random() < 0.1:
            qual = "*"
        else:
            qual = bytes(generator.choice((0, 12, 13, 14, 29, 30, 31, 40, 41, 93, 0xFF, min_baseq, max(min_baseq - 1, 0))) for _ in seq)
        flag = generator.choice((0, 0, 16, 99, 147, 83, 163, 2048, 2064, 4, 256, 512, 1024, 1040, 0x704))
        mapq = generator.choice((0, 3, 19, 20, 21, 60, 254, 255))
        records.append(("t%d_%d" % (seed, t), flag, contig, pos, mapq, "".join("%d%s" % op for op in ops), seq, qual))
    lines = ["# seed %d" % seed, ""]
    for _ in range(70):
        choice = generator.random()
        if choice < 0.55:
            name, position = "a1", generator.randint(1, 100)
        elif choice < 0.7:
            name, position = generator.choice(("chr2", "2")), generator.randint(1, 50)
        elif choice < 0.78:
            name, position = generator.choice(("orphan", "chrorphan")), generator.randint(1, 300)
        elif choice < 0.84:
            name, position = "chra1", generator.randint(95, 100)
        elif choice < 0.92:
            name, position = generator.choice(("a1", "chr2", "orphan")), generator.choice((101, 51, 701, 2 ** 31 - 1))
        else:
            name, position = generator.choice(("nowhere", "chrchr2", "A1", "")), generator.randint(1, 50)
        lines.append("%s\t%d" % (name, position) + generator.choice(("", "", "\t.\tA\tG", "\t")))
        if generator.random() < 0.1:
            lines.append(lines[-1])
        if generator.random() < 0.05:
            lines.append(generator.choice(("", "#a1\t5")))
    return _case(records, "\n".join(lines).encode() + (b"\n" if seed % 2 else b""), min_mapq, min_baseq)


def hot_case():
    """70 001 records over a1:50, the four bases mixed by a fixed pattern, every eleventh base below the threshold, every thirteenth record a deletion there,
    then 64 records that all show the same base at a1:60, so that every lane of a wavefront merges into one add, then a wavefront over the neighbours a1:70 and 71"""
    records = []
    for k in range(70001):
        start = 50 - k % 7
        if k % 13 == 0:
            records.append(("h%05d" % k, 0, "a1", start, 30, "%dM2D3M" % (50 - start), "A" * (53 - start), "I" * (53 - start)))
        else:
            seq = "".join("ACGT"[(k + j) % 4] for j in range(10))
            records.append(("h%05d" % k, 16 if k & 8 else 0, "a1", start, 30, "10M", seq, "".join("+" if (k + j) % 11 == 0 else "I" for j in range(10))))
    records += [("s%02d" % k, 0, "a1", 56, 30, "8M", "ACGTGCAT", "IIIIIIII") for k in range(64)]
    records += [("w%02d" % k, 0, "a1", 66 + k % 5, 30, "8M", "ACGTACGT", "IIIIIIII") for k in range(64)]
    return _case(records, [("a1", 50), ("a1", 60), ("a1", 70), ("a1", 71), ("chra1", 50)])


def wavefront_case():
    """65 records, one past a wavefront, over one site"""
    return _case([("v%02d" % k, 0, "a1", 41, 30, "10M", "ACGTACGTAC"[k % 3:] + "ACG"[:k % 3], "I" * 10) for k in range(65)], [("a1", 45)])


def dense_case():
    """one 150-base read over 150 sites in a row on orphan, a duplicate line among them, and a second read over the first 20 with ten bases inserted in front of them"""
    generator = random.Random(150)
    seq = "".join(generator.choice("ACGTN") for _ in range(150))
    qual = bytes(generator.choice((12, 13, 40)) for _ in range(150))
    sites = [("orphan", 101 + k) for k in range(150)]
    return _case([("long", 0, "orphan", 101, 30, "150M", seq, qual), ("short", 16, "orphan", 101, 30, "10I20M", seq[:30], qual[:30])], sites[:75] + [("orphan", 140)] + sites[75:])


def long_cigar_case():
    """one record of 601 operations on orphan (1M, then 300 times 1N 1M over half, 1D 1M over the rest) with sites in its first, a middle and its last block, under N and under D,
    between records that touch no site"""
    ops = ["1M"] + ["1N1M" if k < 150 else "1D1M" for k in range(300)]
    seq = "".join("ACGT"[k % 4] for k in range(301))
    plain = [("p%d" % k, 0, "a1", 1 + k % 50, 30, "20M", "A" * 20, "I" * 20) for k in range(70)]
    return _case(plain[:40] + [("long", 0, "orphan", 11, 30, "".join(ops), seq, "I" * 301)] + plain[40:], [("orphan", 11), ("orphan", 12), ("orphan", 311), ("orphan", 312), ("orphan", 611), ("orphan", 610), ("orphan", 612)])


def sparse_case():
    """400 records and 1 000 sites of which none is covered: the reads lie on a1 and on orphan 1..140, with long N over orphan 150..280, the sites on chr2 and on orphan 141..149
    and 281..300 and on contigs the header does not have"""
    records = [("r%03d" % k, 0, "a1", 1 + k % 90, 30, "10M", "ACGTACGTAC", "I" * 10) for k in range(200)]
    records += [("o%03d" % k, 0, "orphan", 1 + k % 130, 30, "10M", "ACGTACGTAC", "I" * 10) for k in range(200)]
    sites = [("chr2", 1 + k % 50) for k in range(500)] + [("orphan", 141 + k % 9) for k in range(200)] + [("orphan", 281 + k % 20) for k in range(200)] + [("elsewhere", 1 + k) for k in range(100)]
    return _case(records, sites)


def no_records_case():
    """a header and sites, and no record"""
    return _case([], [("a1", 5), ("chr2", 5), ("nowhere", 5)])


def no_sites_case():
    """records and an empty sites file: a file with only the header line"""
    return _case([("r%d" % k, 0, "a1", 1 + k, 30, "10M", "ACGTACGTAC", "I" * 10) for k in range(5)], b"")


def header_only_case():
    """no reference and no record: every site is unplaced"""
    return _case([], [("a1", 5), ("chr2", 7)], references=[])
