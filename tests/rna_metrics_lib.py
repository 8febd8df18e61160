"""What tests/test_rna_metrics.py shares with tools/: a brute-force restatement of the rule of --rna-metrics in plain Python -- sets of positions and dicts per
position, no runs, no search --, its own readers of GTF, BED and SAM text, its own BAM writer, and the annotations and inputs that are made at test time.  It is written from the
rule, not from rnametrics_core.hpp or region_track.cpp, and shares no code with the project; it is the independent side for inputs made at test time only because it gives
tests/golden/rna_metrics/hand_made.tsv from hand_made.{fa,gtf,bed,sam}.

An annotation is {"lengths": contig -> bases, "genes": [gene ids in order of first appearance], "strand", "contig", "exons": gene -> [(first, last)] 0-based inclusive,
"coding": contig -> set of positions, "rrna": contig -> set of positions, "unknown_intervals": lines of the BED file on a contig the annotation lacks}.
A case is (references, records): references a list of (name, LN); records a list of (qname, flag, rname or "*", 1-based pos, mapq, cigar text or "*", rnext ("*", "=" or a
name), 1-based pnext, tlen, l_seq, tags), tags a list of (two-letter name, type, value) as in tests/gene_counts_lib.py."""
import os
import random
import re
import struct

from gene_counts_lib import EOF_BLOCK, INTEGER_TYPES, PACK, bam_header, bam_tags, integer_type, stream_pipeline, write_bgzf  # noqa: F401  (containers only: nothing of the rule)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rna_metrics")
CIGAR_OPS = "MIDNSHP=X"
SCALARS = ("RECORDS", "SECONDARY", "SUPPLEMENTARY", "PRIMARY", "UNMAPPED", "MAPPED", "QC_FAIL", "DUPLICATE", "MULTIMAPPING", "PAIRED", "PROPER_PAIR", "READ1", "READ2", "MATE_UNMAPPED", "MATE_OTHER_CONTIG",
           "BASE_RECORDS", "BASES", "SOFT_CLIPPED_BASES", "INSERTED_BASES", "DELETED_BASES", "SKIPPED_BASES", "SPLICED_RECORDS", "ALIGNED_BASES", "RIBOSOMAL_BASES", "CODING_BASES", "UTR_BASES",
           "INTRONIC_BASES", "INTERGENIC_BASES", "UNKNOWN_CONTIG_BASES", "SENSE_STRAND_RECORDS", "ANTISENSE_STRAND_RECORDS", "AMBIGUOUS_STRAND_RECORDS", "NO_GENE_RECORDS", "INSERT_SIZE_PAIRS")
DERIVED = ("MEDIAN_INSERT_SIZE", "PCT_RIBOSOMAL_BASES", "PCT_CODING_BASES", "PCT_UTR_BASES", "PCT_INTRONIC_BASES", "PCT_INTERGENIC_BASES", "PCT_SENSE_STRAND", "PCT_MAPPED", "PCT_DUPLICATE", "PCT_MULTIMAPPING")
COMMITTED_CONTIGS = "r1 r2"
R, C, E, GP, GM = 1, 2, 4, 8, 16  # the bits of a base


# ---- the annotation -------------------------------------------------------------------------------------------------------------------------------------------------

def remove_chr(name):
    return name[3:] if name.startswith("chr") else name


def load_annotation(gtf=os.path.join(GOLDEN, "hand_made.gtf"), fasta=os.path.join(GOLDEN, "hand_made.fa"), bed=os.path.join(GOLDEN, "hand_made.bed")):
    lengths, name = {}, None
    for line in open(fasta):
        if line.startswith(">"):
            name = line[1:].strip()
            lengths[name] = 0
        else:
            lengths[name] += len(line.strip())
    genes, strand, contig, exons = [], {}, {}, {}
    transcripts = {}  # transcript id -> {"exons": [(first, last)], "cds": [(first, last)] in file order, "contig"}
    for line in open(gtf):
        if not line.strip() or line.startswith("#"):
            continue
        fields = line.rstrip("\n").split("\t")
        assert len(fields) == 9 and fields[2] in ("exon", "CDS") and fields[6] in "+-", line
        attributes = dict(re.findall(r'(\w+) "([^"]*)"', fields[8]))
        gene, transcript, first, last = attributes["gene_id"], attributes["transcript_id"], int(fields[3]) - 1, int(fields[4]) - 1  # GTF is 1-based closed
        assert "." not in gene and "gene_name" in attributes and fields[0] in lengths and 0 <= first <= last < lengths[fields[0]], line
        record = transcripts.setdefault(transcript, {"exons": [], "cds": [], "contig": fields[0], "gene": gene})
        assert record["contig"] == fields[0] and record["gene"] == gene, line
        if fields[2] == "CDS":
            record["cds"].append((first, last))
            continue
        if gene not in strand:
            genes.append(gene); strand[gene] = fields[6]; contig[gene] = fields[0]; exons[gene] = []
        assert strand[gene] == fields[6] and contig[gene] == fields[0], line  # a gene id is unique: one contig, one strand
        exons[gene].append((first, last))
        record["exons"].append((first, last))
    coding = {name: set() for name in lengths}
    for record in transcripts.values():
        for first, last in record["exons"]:
            piece = None
            for cds_first, cds_last in record["cds"]:  # the last CDS record of the transcript that overlaps the exon gives its coding part
                if cds_first <= last and cds_last >= first:
                    piece = (max(first, cds_first), min(last, cds_last))
            if piece:
                coding[record["contig"]].update(range(piece[0], piece[1] + 1))
    rrna, unknown_intervals, intervals = {name: set() for name in lengths}, 0, 0
    if bed:
        for line in open(bed):
            line = line.rstrip("\r\n")
            if not line or line.startswith("#") or line.startswith("track") or line.startswith("browser"):
                continue
            fields = line.split("\t")
            intervals += 1
            if remove_chr(fields[0]) not in lengths:
                unknown_intervals += 1
                continue
            rrna[remove_chr(fields[0])].update(range(int(fields[1]), int(fields[2])))  # BED is 0-based, half open
    return {"lengths": lengths, "genes": genes, "strand": strand, "contig": contig, "exons": exons, "coding": coding, "rrna": rrna, "intervals": intervals, "unknown_intervals": unknown_intervals}


def per_position(annotation):
    """-> {contig: {"bits": {position: bits, where not 0}, "body": {position: (gene, offset t, L)}}}: every base of the rule, one by one"""
    out = {name: {"bits": {}, "body": {}} for name in annotation["lengths"]}
    owners = {name: {} for name in annotation["lengths"]}
    for name in annotation["lengths"]:
        bits = out[name]["bits"]
        for p in annotation["rrna"][name]:
            bits[p] = bits.get(p, 0) | R
        for p in annotation["coding"][name]:
            bits[p] = bits.get(p, 0) | C
    for gene in annotation["genes"]:
        name, spans = annotation["contig"][gene], annotation["exons"][gene]
        bits = out[name]["bits"]
        for p in range(min(first for first, _ in spans), max(last for _, last in spans) + 1):
            bits[p] = bits.get(p, 0) | (GP if annotation["strand"][gene] == "+" else GM)
        for first, last in spans:
            for p in range(first, last + 1):
                bits[p] = bits.get(p, 0) | E
                owners[name].setdefault(p, set()).add(gene)
    for gene in annotation["genes"]:
        name = annotation["contig"][gene]
        positions = sorted(set(p for first, last in annotation["exons"][gene] for p in range(first, last + 1)))
        length = len(positions)
        if length < 100:
            continue
        for rank, p in enumerate(positions):
            if owners[name][p] == {gene}:
                out[name]["body"][p] = (gene, rank if annotation["strand"][gene] == "+" else length - 1 - rank, length)
    return out


def class_of(bits):
    return "RIBOSOMAL" if bits & R else "CODING" if bits & C else "UTR" if bits & E else "INTRONIC" if bits & (GP | GM) else "INTERGENIC"


# ---- containers -----------------------------------------------------------------------------------------------------------------------------------------------------

def query_length(cigar):
    return 0 if cigar == "*" else sum(int(length) for length, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar) if op in "MIS=X")


def parse_sam(text):
    references, records = [], []
    for line in text.decode().split("\n"):
        if line.startswith("@SQ\t"):
            fields = dict(field.split(":", 1) for field in line.split("\t")[1:])
            references.append((fields["SN"], int(fields["LN"])))
        elif line and not line.startswith("@"):
            f = line.split("\t")
            tags = []
            for field in f[11:]:
                name, kind, value = field.split(":", 2)
                assert kind in "iZ", field
                tags.append((name, integer_type(int(value)), int(value)) if kind == "i" else (name, "Z", value))
            records.append((f[0], int(f[1]), f[2], int(f[3]), int(f[4]), f[5], f[6], int(f[7]), int(f[8]), 0 if f[9] == "*" else len(f[9]), tags))
    return references, records


def sam_text(case):
    references, records = case
    lines = ["@HD\tVN:1.6\tSO:unsorted"] + ["@SQ\tSN:%s\tLN:%d" % reference for reference in references]
    for qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, l_seq, tags in records:
        fields = [qname, str(flag), rname, str(pos), str(mapq), cigar, rnext, str(pnext), str(tlen), "A" * l_seq if l_seq else "*", "*"]
        for name, kind, value in tags:
            fields.append("%s:%s:%s" % (name, "Z" if kind == "Z" else "i", value))
        lines.append("\t".join(fields))
    return ("\n".join(lines) + "\n").encode()


def bam_record(index_of, record):
    qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, l_seq, tags = record
    ref = -1 if rname == "*" else index_of[rname]
    next_ref = -1 if rnext == "*" else ref if rnext == "=" else index_of[rnext]
    ops = [] if cigar == "*" else [(int(length), CIGAR_OPS.index(op)) for length, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]
    body = struct.pack("<iiBBHHHiiii", ref, pos - 1, len(qname) + 1, mapq, 4680, len(ops), flag, l_seq, next_ref, pnext - 1, tlen)
    body += qname.encode() + b"\0" + b"".join(struct.pack("<I", length << 4 | op) for length, op in ops) + b"\x11" * ((l_seq + 1) // 2 - l_seq % 2) + (b"\x10" if l_seq % 2 else b"") + b"\xff" * l_seq + bam_tags(tags)
    return struct.pack("<i", len(body)) + body


def bam_records(case):
    index_of = {name: k for k, (name, _) in enumerate(case[0])}
    return b"".join(bam_record(index_of, record) for record in case[1])


# ---- the rule -------------------------------------------------------------------------------------------------------------------------------------------------------

def nh_of(tags):
    for name, kind, value in tags:
        if kind == "raw":
            return 1
        if name == "NH":
            return value if kind in INTEGER_TYPES else 1
    return 1


def fraction(numerator, denominator):
    return "NA" if denominator == 0 else "%.6f" % (float(numerator) / float(denominator))


def restate(annotation, case, bases=None):
    """-> (text of the file, {"records", "base_records", "blocks"}, counters: name -> number, and the three histograms under "MAPQ", "INSERT_SIZE", "GENE_BODY")"""
    references, records = case
    bases = bases or per_position(annotation)
    length_of = dict(references)
    n = dict((name, 0) for name in SCALARS)
    mapq_bins, insert_bins, body_bins, blocks = {}, {}, [0] * 100, 0
    for qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, l_seq, tags in records:
        n["RECORDS"] += 1
        if flag & 0x100:
            n["SECONDARY"] += 1
            continue
        if flag & 0x800:
            n["SUPPLEMENTARY"] += 1
            continue
        n["PRIMARY"] += 1
        if flag & 4 or rname == "*":
            n["UNMAPPED"] += 1
            continue
        mate_contig = None if rnext == "*" else rname if rnext == "=" else rnext
        n["MAPPED"] += 1
        n["QC_FAIL"] += bool(flag & 0x200)
        n["DUPLICATE"] += bool(flag & 0x400)
        n["MULTIMAPPING"] += nh_of(tags) > 1
        if flag & 1:
            n["PAIRED"] += 1
            n["PROPER_PAIR"] += bool(flag & 2)
            n["READ1"] += bool(flag & 0x40)
            n["READ2"] += bool(flag & 0x80)
            n["MATE_UNMAPPED"] += bool(flag & 8)
            n["MATE_OTHER_CONTIG"] += (not flag & 8) and mate_contig != rname
        mapq_bins[mapq] = mapq_bins.get(mapq, 0) + 1
        if flag & 0x200 or pos - 1 < 0:
            continue
        n["BASE_RECORDS"] += 1
        n["BASES"] += l_seq
        at, covered = pos - 1, set()
        ops = [] if cigar == "*" else [(int(length), op) for length, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]
        for length, op in ops:
            if op in "M=X":
                covered.update(range(max(at, 0), min(at + length, length_of[rname])))
            if op in "M=XDN":
                at += length
            n["SOFT_CLIPPED_BASES"] += length if op == "S" else 0
            n["INSERTED_BASES"] += length if op == "I" else 0
            n["DELETED_BASES"] += length if op == "D" else 0
            n["SKIPPED_BASES"] += length if op == "N" else 0
        n["SPLICED_RECORDS"] += any(op == "N" for _, op in ops)
        blocks += sum(1 for p in covered if p - 1 not in covered)
        n["ALIGNED_BASES"] += len(covered)
        known = bases.get(remove_chr(rname))
        seen = 0
        for p in covered:
            if known is None:
                n["UNKNOWN_CONTIG_BASES"] += 1
                continue
            bits = known["bits"].get(p, 0)
            n[class_of(bits) + "_BASES"] += 1
            seen |= bits & (GP | GM)
            if p in known["body"]:
                gene, t, length = known["body"][p]
                body_bins[(100 * t) // length] += 1
        read_forward = (not flag & 0x10) != bool(flag & 1 and flag & 0x80)
        if seen in (GP, GM):
            n["SENSE_STRAND_RECORDS" if (seen == GP) == read_forward else "ANTISENSE_STRAND_RECORDS"] += 1
        elif seen:
            n["AMBIGUOUS_STRAND_RECORDS"] += 1
        else:
            n["NO_GENE_RECORDS"] += 1
        if flag & 1 and flag & 0x40 and not flag & 8 and mate_contig == rname and tlen != 0:
            size = min(abs(tlen), 1001)
            insert_bins[size] = insert_bins.get(size, 0) + 1
            n["INSERT_SIZE_PAIRS"] += 1
    lines = ["## METRICS"] + ["%s\t%d" % (name, n[name]) for name in SCALARS]
    median = "NA"
    if n["INSERT_SIZE_PAIRS"]:
        half, total = (n["INSERT_SIZE_PAIRS"] + 1) // 2, 0
        for size in sorted(insert_bins):
            total += insert_bins[size]
            if total >= half:
                median = ">1000" if size == 1001 else str(size)
                break
    lines.append("MEDIAN_INSERT_SIZE\t" + median)
    for kind in ("RIBOSOMAL", "CODING", "UTR", "INTRONIC", "INTERGENIC"):
        lines.append("PCT_%s_BASES\t%s" % (kind, fraction(n[kind + "_BASES"], n["ALIGNED_BASES"])))
    lines.append("PCT_SENSE_STRAND\t" + fraction(n["SENSE_STRAND_RECORDS"], n["SENSE_STRAND_RECORDS"] + n["ANTISENSE_STRAND_RECORDS"]))
    lines.append("PCT_MAPPED\t" + fraction(n["MAPPED"], n["PRIMARY"]))
    lines.append("PCT_DUPLICATE\t" + fraction(n["DUPLICATE"], n["MAPPED"]))
    lines.append("PCT_MULTIMAPPING\t" + fraction(n["MULTIMAPPING"], n["MAPPED"]))
    lines.append("## MAPQ")
    lines += ["%d\t%d" % (q, mapq_bins[q]) for q in sorted(mapq_bins)]
    lines.append("## INSERT_SIZE")
    lines += ["%s\t%d" % (">1000" if size == 1001 else size, insert_bins[size]) for size in sorted(insert_bins)]
    lines.append("## GENE_BODY")
    lines += ["%d\t%d" % (k, body_bins[k]) for k in range(100)]
    counters = dict(n)
    counters.update({"MAPQ": mapq_bins, "INSERT_SIZE": insert_bins, "GENE_BODY": body_bins})
    return ("\n".join(lines) + "\n").encode(), {"records": n["RECORDS"], "base_records": n["BASE_RECORDS"], "blocks": blocks}, counters


def parse_table(text):
    """the file -> ({name: text of the value} of "## METRICS" in order as a list of pairs, {q: n}, {size or ">1000": n}, [100 numbers])"""
    sections, name = {}, None
    for line in text.decode().split("\n")[:-1]:
        if line.startswith("## "):
            name = line[3:]
            sections[name] = []
        else:
            sections[name].append(line.split("\t"))
    assert list(sections) == ["METRICS", "MAPQ", "INSERT_SIZE", "GENE_BODY"] and all(len(row) == 2 for rows in sections.values() for row in rows)
    return sections["METRICS"], {int(q): int(v) for q, v in sections["MAPQ"]}, {size: int(v) for size, v in sections["INSERT_SIZE"]}, [int(v) for _, v in sections["GENE_BODY"]]


def check_invariants(text):
    """the invariants of DESIGN.md 4.19 on a file; returns the scalar counters as numbers"""
    metrics, mapq, insert, body = parse_table(text)
    assert [name for name, _ in metrics] == list(SCALARS + DERIVED)
    n = {name: int(value) for name, value in metrics[:len(SCALARS)]}
    assert n["RIBOSOMAL_BASES"] + n["CODING_BASES"] + n["UTR_BASES"] + n["INTRONIC_BASES"] + n["INTERGENIC_BASES"] + n["UNKNOWN_CONTIG_BASES"] == n["ALIGNED_BASES"]
    assert n["SENSE_STRAND_RECORDS"] + n["ANTISENSE_STRAND_RECORDS"] + n["AMBIGUOUS_STRAND_RECORDS"] + n["NO_GENE_RECORDS"] == n["BASE_RECORDS"]
    assert sum(mapq.values()) == n["MAPPED"] and all(0 <= q <= 255 and v > 0 for q, v in mapq.items()) and list(mapq) == sorted(mapq)
    assert sum(insert.values()) == n["INSERT_SIZE_PAIRS"] and all(v > 0 for v in insert.values())
    sizes = [1001 if size == ">1000" else int(size) for size in insert]
    assert sizes == sorted(sizes) and all(1 <= size <= 1001 for size in sizes)
    assert len(body) == 100 and sum(body) <= n["CODING_BASES"] + n["UTR_BASES"] + n["RIBOSOMAL_BASES"]
    assert n["SECONDARY"] + n["SUPPLEMENTARY"] + n["PRIMARY"] == n["RECORDS"] and n["UNMAPPED"] + n["MAPPED"] == n["PRIMARY"]
    return n


# ---- annotations and cases made at test time --------------------------------------------------------------------------------------------------------------------------

def write_seeded_annotation(seed, directory):
    """a seeded annotation on two contigs: about 150 genes of both strands on s1 (30 kb), many of which overlap, with one or two transcripts of one to five exons, most with a
    coding part; a few short genes (fewer than 100 exonic bases); rRNA intervals over exons, introns and empty sequence, one spelled with "chr", one on a contig that does not
    exist.  Writes NAME.fa, NAME.gtf, NAME.bed into `directory`; returns their prefix"""
    generator = random.Random(seed)
    lengths = {"s1": 30000, "s2": 3000}
    prefix = os.path.join(directory, "seeded%d" % seed)
    with open(prefix + ".fa", "w") as out:
        for name in sorted(lengths):
            out.write(">%s\n" % name)
            sequence = "".join(generator.choice("ACGT") for _ in range(lengths[name]))
            out.write("\n".join(sequence[k:k + 100] for k in range(0, len(sequence), 100)) + "\n")
    lines = []
    for g in range(165):
        contig = "s1" if g < 150 else "s2"
        strand = generator.choice("+-")
        at = generator.randint(0, lengths[contig] - 2000)
        for t in range(generator.choice((1, 1, 2))):
            first = at + generator.randint(0, 60)
            spans = []
            for _ in range(generator.choice((1, 1, 2, 3, 5))):
                last = first + generator.choice((9, 19, 49, 99, generator.randint(5, 150)))
                spans.append((first, last))
                first = last + 1 + generator.choice((10, 50, generator.randint(1, 200)))
            has_cds = generator.random() < 0.7
            cds = (generator.randint(spans[0][0], spans[-1][1]), generator.randint(spans[0][0], spans[-1][1]))
            for first, last in spans:
                attributes = 'gene_id "G%03d"; transcript_id "T%03d_%d"; gene_name "N%03d";' % (g, g, t, g)
                lines.append("%s\ttest\texon\t%d\t%d\t.\t%s\t.\t%s" % (contig, first + 1, last + 1, strand, attributes))
                if has_cds and min(cds) <= last and max(cds) >= first:
                    lines.append("%s\ttest\tCDS\t%d\t%d\t.\t%s\t0\t%s" % (contig, max(first, min(cds)) + 1, min(last, max(cds)) + 1, strand, attributes))
    open(prefix + ".gtf", "w").write("\n".join(lines) + "\n")
    bed = ["# rRNA", "track name=rRNA", "browser position s1:1-100", ""]
    for _ in range(12):
        start = generator.randint(0, lengths["s1"] - 400)
        bed.append("%s\t%d\t%d\trRNA\t0\t+" % (generator.choice(("s1", "chrs1")), start, start + generator.choice((0, 1, 30, 300))))
    bed += ["s2\t100\t180", "nowhere\t5\t50", "chrnowhere\t1\t2"]
    open(prefix + ".bed", "w").write("\n".join(bed) + "\n")
    return prefix


def references_of(annotation):
    return sorted(annotation["lengths"].items()) + [("orphan", 500)]


def _exon_list(annotation):
    return [(annotation["contig"][gene], first, last) for gene in annotation["genes"] for first, last in annotation["exons"][gene]]


def random_case(seed, annotation, max_records=300):
    """a few hundred records on an annotation: reads that begin around the edges of exons, are spliced, clipped, deleted from and inserted into, run past the end of their contig,
    begin before it (POS 0) or lie on the reference without a contig; pairs with every combination of the pair flags and TLEN around 1000 and at the ends of its range; QC-fail,
    duplicate, secondary, supplementary and unmapped records; NH in several types; MAPQ over its whole range"""
    generator = random.Random(seed)
    references, exons = references_of(annotation), _exon_list(annotation)
    length_of = dict(references)
    records = []
    while len(records) < max_records:
        choice = generator.random()
        if choice < 0.8:
            contig, first, last = generator.choice(exons)
            pos = max(0, generator.choice((first, last)) + 1 + generator.randint(-40, 10))
        elif choice < 0.9:
            contig = generator.choice(references)[0]
            pos = generator.randint(0, length_of[contig])
        else:
            contig = generator.choice(references)[0]
            pos = max(1, length_of[contig] - generator.randint(-5, 60))
        ops = []
        if generator.random() < 0.2:
            ops.append("%d%s" % (generator.randint(1, 9), generator.choice("SH")))
        for piece in range(generator.choice((1, 1, 1, 2, 2, 3, 6))):
            if piece:
                ops.append("%d%s" % (generator.choice((1, 4, 10, 50, 100, 200, generator.randint(1, 300))), generator.choice("NNNDDIP")))
            ops.append("%d%s" % (generator.choice((1, 5, 20, 50, 75, generator.randint(1, 400))), generator.choice("MMMMM=X")))
        if generator.random() < 0.2:
            ops.append("%dS" % generator.randint(1, 9))
        cigar = "".join(ops) if generator.random() < 0.97 else "*"
        flag = generator.choice((0, 16, 0, 16, 99, 147, 83, 163, 97, 145, 65, 129, 81, 161, 73, 137, 89, 1, 3))
        flag |= generator.choice((0, 0, 0, 0, 0, 0, 0x200, 0x400, 0x100, 0x800, 0x900, 0x600))
        rnext = "*" if not flag & 1 else generator.choice(("=", "=", "=", generator.choice(references)[0]))
        tlen = generator.choice((0, 1, -1, 150, -150, 999, 1000, 1001, -1000, -1001, 70000, 2147483647, -2147483648, generator.randint(-1200, 1200)))
        tags = generator.choice(([], [], [], [("NH", "C", 1)], [("NH", "C", 3)], [("XZ", "Z", "text"), ("NH", "S", 300)], [("NH", "c", -1)], [("NH", "Z", "5")], [("HI", "C", 1), ("NH", "i", 70000)]))
        records.append(("q%d_%d" % (seed, len(records)), flag, contig, pos, generator.choice((0, 1, 3, 30, 60, 254, 255, generator.randint(0, 255))), cigar, rnext, generator.randint(1, 1000), tlen, query_length(cigar), tags))
        if generator.random() < 0.05:
            records.append(("u%d_%d" % (seed, len(records)), generator.choice((4, 77, 141, 4 | 0x200)), generator.choice(("*", contig)), 0 if generator.random() < 0.5 else pos, 0, "*", "*", 0, 0, 30, []))
    return references, records


def _sites(annotation, count):
    exons = _exon_list(annotation)
    return [exons[(7 * k) % len(exons)] for k in range(count)]


def spread_case(annotation, count):
    """`count` records over the exons in turn, alternating strands and mates: one past a wavefront (65) or one past a workgroup (257)"""
    out = []
    for k, (contig, first, last) in enumerate(_sites(annotation, count)):
        flag = (0, 16, 99, 147, 83, 163)[k % 6]
        out.append(("w%03d" % k, flag, contig, max(1, first + 1 - (k % 7)), k % 61, "30M", "=" if flag & 1 else "*", first + 1, (k % 5 - 2) * 300 if flag & 1 else 0, 30, []))
    return references_of(annotation), out


def hot_case(annotation):
    """20 000 identical records: every lane adds to the same counters and the same bins of all three histograms"""
    body = per_position(annotation)["s1"]["body"]
    start = min(body)
    return references_of(annotation), [("hot", 99, "s1", start + 1, 37, "25M5N25M", "=", start + 200, 321, 50, [])] * 20000


def long_cigar_case(annotation):
    """one record of 601 operations on s1: 301 blocks with N and D between them, from the first boundary of the annotation on; every block that is not long ends exactly on the
    last base before a boundary (an exon's first base, or the base behind its last), and the gap behind it makes the next block start exactly on the next boundary; every third
    block runs across five boundaries"""
    boundaries = sorted(set(b for contig, first, last in _exon_list(annotation) if contig == "s1" for b in (first, last + 1)))
    at, k, ops = boundaries[0], 0, []
    start = at
    for block in range(301):
        steps = 5 if block % 3 == 2 else 1
        while k < len(boundaries) and boundaries[k] <= at:
            k += 1
        end = boundaries[min(k + steps - 1, len(boundaries) - 1)] if k < len(boundaries) else at + 7
        if end <= at:
            end = at + 7
        ops.append("%dM" % (end - at))
        at = end
        if block == 300:
            break
        while k < len(boundaries) and boundaries[k] <= at:
            k += 1
        gap_end = boundaries[k] if k < len(boundaries) else at + 3
        ops.append("%d%s" % (gap_end - at, "ND"[block % 2]))
        at = gap_end
    assert len(ops) == 601 and at < annotation["lengths"]["s1"]
    cigar = "".join(ops)
    return references_of(annotation), [("long", 0, "s1", start + 1, 60, cigar, "*", 0, 0, query_length(cigar), []), ("after", 16, "s1", start + 1, 60, "50M", "*", 0, 0, 50, [])]


def empty_case(annotation):
    """records, but none that is primary"""
    return references_of(annotation), [("e1", 256, "s1", 111, 9, "20M", "*", 0, 0, 20, []), ("e2", 2048, "s2", 101, 9, "20M", "*", 0, 0, 20, [])]


def no_records_case(annotation):
    return references_of(annotation), []


def decode_track(track_arrays, annotation, contig_index):
    """the arrays of a track (numpy: contig_offset, run_start, run_bits, run_gene, run_rank, gene_body) back to per-base {"bits": {p: bits}, "body": {p: (gene index, t, L)}} per
    contig name; contig_index: name -> contig of the session"""
    contig_offset, run_start, run_bits, run_gene, run_rank, gene_body = track_arrays
    out = {}
    for name, length in annotation["lengths"].items():
        c = contig_index[name]
        bits, body = {}, {}
        begin, end = int(contig_offset[c]), int(contig_offset[c + 1])
        assert end > begin and run_start[begin] == 0
        for r in range(begin, end):
            first, last = int(run_start[r]), (int(run_start[r + 1]) if r + 1 < end else length) - 1
            assert r + 1 == end or run_start[r + 1] > run_start[r]
            assert r == begin or (run_bits[r], run_gene[r]) != (run_bits[r - 1], run_gene[r - 1])  # neighbours that are equal are merged
            for p in range(first, min(last, length - 1) + 1):
                if run_bits[r]:
                    bits[p] = int(run_bits[r])
                if run_gene[r] != 0xFFFFFFFF:
                    L, forward = int(gene_body[run_gene[r]]) & 0x7FFFFFFF, int(gene_body[run_gene[r]]) >> 31
                    rank = int(run_rank[r]) + p - first
                    body[p] = (int(run_gene[r]), rank if forward else L - 1 - rank, L)
        out[name] = {"bits": bits, "body": body}
    return out
