"""What tests/test_realign_split.py shares with tools/: a restatement of the rule of --realign-reads in plain Python -- dicts by read name, string formatting of
the SAM fields, and the regular expressions of the rule applied to the CIGAR *text* --, a writer of BAM records with mate fields, and the cases that are made at test time on the
committed assembly (tests/golden/realign_split/hand_made.{fa,gtf}).  It is written from the rule, not from realign_core.hpp, and shares no code with the project; it is the
independent side for inputs made at test time only because it gives tests/golden/realign_split/hand_made*.{realign,kept}.sam, which a reader can check by eye, from
hand_made*.sam.

A case is a dict: "references" a list of (name, LN); "records" a list of (qname, flag, rname or "*", 1-based pos, mapq, cigar text or "*", rnext ("=", "*" or a name), 1-based pnext,
tlen, seq over "=ACMGRSVTWYHKDBN" or "*", qual as SAM quality characters or "*")."""
import os
import random
import re
import struct

from gene_counts_lib import bam_header, stream_pipeline, write_bgzf  # noqa: F401 (the containers, for the tests)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "realign_split")
COMMITTED_CONTIGS = "a1 2"
HEADER = [("a1", 100), ("chr2", 50), ("orphan", 700)]  # of the committed cases: chr2 is 2 in the assembly, orphan is not in it
COUNTED = ("records", "templates", "realign_templates", "kept_templates", "dropped_secondary", "extra", "orphans", "placeholder_cigar", "realign_bytes", "kept_bytes", "layout")
CODES = "=ACMGRSVTWYHKDBN"
CIGAR_OPS = "MIDNSHP=X"


def load_assembly(fasta=os.path.join(GOLDEN, "hand_made.fa")):
    """-> [(contig as the file spells it, bases)] in the order of the file"""
    contigs = []
    for line in open(fasta):
        if line.startswith(">"):
            contigs.append([line[1:].split()[0], 0])
        else:
            contigs[-1][1] += len(line.rstrip("\n"))
    return [tuple(contig) for contig in contigs]


def parse_sam(text):
    references, records = [], []
    for line in text.decode().split("\n"):
        if line.startswith("@SQ\t"):
            fields = dict(field.split(":", 1) for field in line.split("\t")[1:])
            references.append((fields["SN"], int(fields["LN"])))
        elif line and not line.startswith("@"):
            f = line.split("\t")
            records.append((f[0], int(f[1]), f[2], int(f[3]), int(f[4]), f[5], f[6], int(f[7]), int(f[8]), f[9], f[10]))
    return {"references": references, "records": records}


def committed_case(name="hand_made"):
    return parse_sam(open(os.path.join(GOLDEN, name + ".sam"), "rb").read())


def bam_record(index_of, record):
    qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = record
    ref = -1 if rname == "*" else index_of[rname]
    next_ref = -1 if rnext == "*" else ref if rnext == "=" else index_of[rnext]
    ops = [] if cigar == "*" else [(int(length), CIGAR_OPS.index(op)) for length, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]
    nibbles = [] if seq == "*" else [CODES.index(c) for c in seq]
    quals = [0xFF] * len(nibbles) if qual == "*" else [ord(c) - 33 for c in qual]
    assert len(quals) == len(nibbles), record
    body = struct.pack("<iiBBHHHiiii", ref, pos - 1, len(qname) + 1, mapq, 4680, len(ops), flag, len(nibbles), next_ref, pnext - 1, tlen)
    body += qname.encode() + b"\0" + b"".join(struct.pack("<I", length << 4 | op) for length, op in ops)
    body += bytes((nibbles[i] << 4) | (nibbles[i + 1] if i + 1 < len(nibbles) else 0) for i in range(0, len(nibbles), 2)) + bytes(quals)
    return struct.pack("<i", len(body)) + body


def bam_records(case):
    index_of = {name: k for k, (name, _) in enumerate(case["references"])}
    return b"".join(bam_record(index_of, record) for record in case["records"])


def sam_text(case):
    lines = ["@HD\tVN:1.6\tSO:unsorted"] + ["@SQ\tSN:%s\tLN:%d" % reference for reference in case["references"]]
    return ("\n".join(lines + ["\t".join(str(field) for field in record) for record in case["records"]]) + "\n").encode()


# ---- the rule -------------------------------------------------------------------------------------------------------------------------------------------------------

def without_chr(name):
    return name[3:] if name.startswith("chr") else name


def kept_header(assembly, references):
    """@HD, then an @SQ line per contig of the assembly in its order: spelled as the input spells it where the input has it, with the length the assembly gives"""
    lines = ["@HD\tVN:1.4\tSO:unsorted\n"]
    for contig, length in assembly:
        spelled = [name for name, _ in references if without_chr(name) == without_chr(contig)]
        lines.append("@SQ\tSN:%s\tLN:%d\n" % (spelled[0] if spelled else contig, length))
    return "".join(lines)


def says_realign(record, paired, in_assembly):
    qname, flag, rname, pos, mapq, cigar = record[:6]
    return bool(flag & 0x4
                or not flag & 0x10 and re.search(r"^[0-9][0-9]+S", cigar)
                or flag & 0x10 and re.search(r"[0-9][0-9]S$", cigar)
                or not paired and re.search(r"[0-9][0-9]S", cigar)
                or paired and not flag & 0x2
                or without_chr(rname) not in in_assembly)


def line_of(record):
    qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = record
    if rname != "*" and rnext == rname:
        rnext = "="
    return "%s\t%d\t%s\t%d\t%d\t%s\t%s\t%d\t%d\t%s\t%s\n" % (qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual)


def is_placeholder(record):
    match = re.match(r"^(\d+)S(\d+)N$", record[5])
    return bool(match) and int(match.group(1)) == (0 if record[9] == "*" else len(record[9]))


def restate(assembly, case):
    """-> (the bytes of the file to realign, the bytes of the file of the kept templates with its header, the statistics)"""
    records = case["records"]
    in_assembly = set(without_chr(contig) for contig, _ in assembly)
    paired = bool(records) and bool(records[0][1] & 0x1)
    stats = dict.fromkeys(COUNTED, 0)
    stats["records"], stats["layout"] = len(records), "PE" if paired else "SE"
    primary = [(rank, record) for rank, record in enumerate(records) if not record[1] & 0x900]
    stats["dropped_secondary"] = len(records) - len(primary)
    templates = []  # (the rank that orders it, its records)
    if not paired:
        templates = [(rank, [record]) for rank, record in primary]
    else:
        slots = {}
        for rank, record in primary:
            slot = 1 if record[1] & 0x1 and record[1] & 0x80 else 0
            ends = slots.setdefault(record[0], {})
            if slot in ends:
                stats["extra"] += 1
            else:
                ends[slot] = (rank, record)
        for ends in slots.values():
            if len(ends) == 2:
                templates.append((ends[0][0], [ends[0][1], ends[1][1]]))
            else:
                stats["orphans"] += 1
    files = {True: [], False: []}
    for rank, ends in sorted(templates, key=lambda template: template[0]):
        realign = any(says_realign(end, paired, in_assembly) for end in ends)
        text = "".join(line_of(end) for end in ends)
        files[realign].append(text)
        stats["realign_templates" if realign else "kept_templates"] += 1
        stats["realign_bytes" if realign else "kept_bytes"] += len(text)
        stats["placeholder_cigar"] += sum(1 for end in ends if is_placeholder(end))
    stats["templates"] = len(templates) + stats["orphans"]
    return "".join(files[True]).encode(), (kept_header(assembly, case["references"]) + "".join(files[False])).encode(), stats


# ---- cases made at test time ------------------------------------------------------------------------------------------------------------------------------------------

def _case(records, references=None):
    return {"references": list(HEADER if references is None else references), "records": records}


def _bases(generator, length):
    return "".join(generator.choice("ACGT" * 5 + "N=RYKMSWBDHV") for _ in range(length)) or "*"


def _cigar(generator):
    """clips of 8 to 12 bases at either end, hard clips outside them, some operations between; -> (text, bases of SEQ)"""
    ops = []
    if generator.random() < 0.15:
        ops.append((generator.randint(1, 12), "H"))
    if generator.random() < 0.45:
        ops.append((generator.randint(8, 12), "S"))
    for piece in range(generator.choice((1, 1, 2, 3))):
        if piece:
            ops.append((generator.choice((1, 2, 10, 11, generator.randint(1, 30))), generator.choice("IDNP")))
        ops.append((generator.choice((1, 9, 10, 25, generator.randint(1, 40))), generator.choice("MMMM=X")))
    if generator.random() < 0.45:
        ops.append((generator.randint(8, 12), "S"))
    if generator.random() < 0.15:
        ops.append((generator.randint(1, 12), "H"))
    return "".join("%d%s" % op for op in ops), sum(length for length, op in ops if op in "MIS=X")


def random_case(seed, paired=None, max_templates=150):
    """a few hundred records under the committed header: every combination of the flag bits, clips of 8 to 12 bases, missing and repeated mates, repeated names, records without
    CIGAR, SEQ or QUAL, every form of RNEXT, shuffled so that the mates of a template lie anywhere in the file.  The seeds below 1810 are those that the GPU tier feeds through
    read_chimeric_alignments, which refuses a mapped record without a reference and is not made for one without a CIGAR: there such records carry 0x4; the other seeds keep them"""
    generator = random.Random(seed)
    ingestible = seed < 1810
    paired = bool(seed & 1) if paired is None else paired
    records, names = [], []
    for t in range(generator.randint(max_templates // 2, max_templates)):
        name = generator.choice(names) if names and generator.random() < 0.08 else "t%d_%d" % (seed, t)
        names.append(name)
        for mate in range(2 if paired else 1):
            if paired and generator.random() < 0.08:
                continue  # a missing mate
            for _ in range(2 if generator.random() < 0.05 else 1):  # a repeated mate
                flag = sum(bit for bit in (0x2, 0x4, 0x8, 0x10, 0x20, 0x100, 0x200, 0x400, 0x800) if generator.random() < (0.5 if bit in (0x2, 0x10, 0x20) else 0.07))
                if paired:
                    flag |= 0x1 | generator.choice((0x40, 0x40, 0x40, 0, 0xC0) if mate == 0 else (0x80, 0x80, 0x80, 0x80, 0xC0))
                elif generator.random() < 0.1:
                    flag |= generator.choice((0x1, 0x41, 0x81))
                if generator.random() < 0.6:
                    flag |= 0x2
                rname = generator.choice(("a1", "a1", "a1", "a1", "chr2", "chr2", "orphan", "*")) if generator.random() < 0.25 else "a1"
                cigar, l_seq = _cigar(generator)
                kind = generator.random()
                if kind < 0.05:
                    cigar = "*"
                    l_seq = generator.randint(0, 30)
                if ingestible and (rname == "*" or cigar == "*"):
                    flag |= 0x4
                seq = "*" if kind > 0.96 else _bases(generator, l_seq)
                qual = "*" if seq == "*" or generator.random() < 0.1 else "".join(chr(33 + generator.choice((0, 2, 13, 30, 40, 41, 93))) for _ in seq)
                rnext = generator.choice(("=", "=", "=", "*", "a1", "chr2", "orphan"))
                if rname == "*" and rnext == "=":
                    rnext = "*"
                records.append((name, flag, rname, generator.randint(0, 120), generator.choice((0, 1, 60, 255)), cigar, rnext, generator.randint(0, 700), generator.randint(-500, 500), seq, qual))
    generator.shuffle(records)
    for k, record in enumerate(records):  # the layout is that of the first record
        if bool(record[1] & 0x1) == paired:
            records[0], records[k] = records[k], records[0]
            break
    else:
        records = []
    return _case(records)


def _pair(name, first, second):
    """a proper pair on a1: (cigar, seq) per mate"""
    return [(name, 99, "a1", 11, 60, first[0], "=", 41, 50, first[1], "I" * len(first[1])), (name, 147, "a1", 41, 60, second[0], "=", 11, -50, second[1], "I" * len(second[1]))]


def templates_case(count, paired=True):
    """`count` templates, one past a wavefront or two: every third is clipped at its 5' end"""
    records = []
    for k in range(count):
        first = ("10S10M", "ACGTACGTAC" * 2) if k % 3 == 0 else ("20M", "ACGTACGTAC" * 2)
        records += _pair("w%03d" % k, first, ("20M", "TTGCA" * 4)) if paired else [("w%03d" % k, 0, "a1", 11, 60, first[0], "*", 0, 0, first[1], "I" * 20)]
    return _case(records)


def long_cigar_case():
    """one record of 601 operations (1M, then 300 times 1N 1M or 1D 1M) between plain pairs, and a mate with a 12S clip behind 600 operations"""
    ops = "1M" + "".join("1N1M" if k < 150 else "1D1M" for k in range(300))
    seq = "".join("ACGT"[k % 4] for k in range(301))
    plain = [record for k in range(40) for record in _pair("p%02d" % k, ("20M", "A" * 20), ("20M", "C" * 20))]
    long_pair = [("long", 99, "orphan", 11, 60, ops, "=", 11, 700, seq, "I" * 301), ("long", 147, "orphan", 11, 60, ops + "12S", "=", 11, -700, seq + "G" * 12, "I" * 313)]
    kept_long = [("long2", 99, "a1", 1, 60, ops, "=", 1, 700, seq, "I" * 301), ("long2", 147, "a1", 1, 60, "9S" + ops, "=", 1, -700, "G" * 9 + seq, "I" * 310)]
    return _case(plain[:40] + long_pair + plain[40:] + kept_long)


def long_name_case():
    """a name of 254 bytes, the longest a BAM record holds, kept and realigned"""
    return _case(_pair("n" * 254, ("20M", "A" * 20), ("20M", "C" * 20)) + _pair("m" * 254, ("12S8M", "A" * 20), ("20M", "C" * 20)) + _pair("short", ("20M", "A" * 20), ("20M", "C" * 20)))


def no_records_case():
    return _case([])


def header_only_case():
    """no reference and no record"""
    return _case([], references=[])


def all_kept_case():
    return _case([record for k in range(70) for record in _pair("k%02d" % k, ("20M", "ACGTA" * 4), ("5H20M", "TTGCA" * 4))])


def all_realign_case():
    return _case([record for k in range(70) for record in _pair("r%02d" % k, ("11S9M", "ACGTA" * 4), ("20M", "TTGCA" * 4))])


def single_end_case():
    """single-end reads whose lengths differ, so that the lines of a wavefront begin at any offset of a window"""
    generator = random.Random(77)
    records = []
    for k in range(200):
        length = generator.randint(1, 150)
        clip = generator.choice((0, 0, 9, 10, 30))
        cigar = "%dM" % length if clip == 0 or clip >= length else "%dM%dS" % (length - clip, clip)
        records.append(("se%03d" % k, generator.choice((0, 16)), "a1", 1 + k % 90, 60, cigar, "*", 0, 0, _bases(generator, length), "".join(chr(33 + generator.randint(0, 60)) for _ in range(length))))
    return _case(records)
