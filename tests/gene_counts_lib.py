"""What tests/test_gene_counts.py shares with tools/: a brute-force restatement of the rule of --gene-counts in plain Python -- a set of positions per gene, dicts by
read name, no index --, its own SAM reader and BAM writer (optional fields included), and the cases that are made at test time on the committed annotation
(tests/golden/gene_counts/hand_made.gtf).  It is written from the rule, not from genecount_core.hpp, and shares no code with the project; it is the independent side for inputs
made at test time only because it gives tests/golden/gene_counts/hand_made.tab, which a reader can check by eye, from hand_made.sam.

A case is (references, records): references a list of (name, LN); records a list of (qname, flag, rname or "*", 1-based pos, cigar text or "*", tags), tags a list of
(two-letter name, type, value) with type one of c C s S i I Z and B (value: (element type, list of numbers)), or "raw" (value: the bytes that follow the name in the record, type
byte included: a field that is malformed on purpose, at which every walk over the optional fields ends)."""
import os
import random
import re
import struct
import zlib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gene_counts")
SPECIAL = ("N_unmapped", "N_multimapping", "N_noFeature", "N_ambiguous")
INTEGER_TYPES = "cCsSiI"
CIGAR_OPS = "MIDNSHP=X"
PACK = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}


# ---- the annotation -------------------------------------------------------------------------------------------------------------------------------------------------

def load_annotation(gtf=os.path.join(GOLDEN, "hand_made.gtf"), fasta=os.path.join(GOLDEN, "hand_made.fa")):
    """-> {"genes": ids in the order in which an exon record first names them, "strand": id -> "+" / "-", "contig": id -> name, "positions": id -> set of 0-based positions,
    "lengths": contig -> bases of the FASTA}.  Only GTFs of the kind the fixtures promise are read: that is asserted."""
    lengths, name = {}, None
    for line in open(fasta):
        if line.startswith(">"):
            name = line[1:].strip()
            lengths[name] = 0
        else:
            lengths[name] += len(line.strip())
    genes, strand, contig, positions = [], {}, {}, {}
    for line in open(gtf):
        if not line.strip() or line.startswith("#"):
            continue
        fields = line.rstrip("\n").split("\t")
        assert len(fields) == 9 and fields[2] == "exon", line
        attributes = dict(re.findall(r'(\w+) "([^"]*)"', fields[8]))
        gene, start, end = attributes["gene_id"], int(fields[3]), int(fields[4])
        assert "." not in gene and "transcript_id" in attributes and "gene_name" in attributes and fields[6] in "+-", line
        assert fields[0] in lengths and 1 <= start <= end <= lengths[fields[0]], line  # everything lies inside its contig
        if gene not in strand:
            genes.append(gene); strand[gene] = fields[6]; contig[gene] = fields[0]; positions[gene] = set()
        assert strand[gene] == fields[6] and contig[gene] == fields[0], line  # a gene id is unique: one contig, one strand
        positions[gene].update(range(start - 1, end))  # GTF is 1-based closed
    assert 3 <= len(lengths) <= 5 and all(50 <= n <= 5000 for n in lengths.values())
    return {"genes": genes, "strand": strand, "contig": contig, "positions": positions, "lengths": lengths}


# ---- containers -----------------------------------------------------------------------------------------------------------------------------------------------------

def integer_type(value):
    """the type `samtools view -b` gives an integer of SAM text: the smallest that holds it"""
    if value < 0:
        return "c" if value >= -128 else "s" if value >= -32768 else "i"
    return "C" if value < 256 else "S" if value < 65536 else "I"


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
                if kind == "i":
                    tags.append((name, integer_type(int(value)), int(value)))
                elif kind == "B":
                    tags.append((name, "B", (value[0], [int(x) for x in value.split(",")[1:]])))
                else:
                    assert kind == "Z", field
                    tags.append((name, "Z", value))
            records.append((f[0], int(f[1]), f[2], int(f[3]), f[5], tags))
    return references, records


def sam_text(case):
    references, records = case
    lines = ["@HD\tVN:1.6\tSO:unsorted"] + ["@SQ\tSN:%s\tLN:%d" % reference for reference in references]
    for qname, flag, rname, pos, cigar, tags in records:
        fields = [qname, str(flag), rname, str(pos), "30" if rname != "*" else "0", cigar, "*", "0", "0", "*", "*"]
        for name, kind, value in tags:
            assert kind in INTEGER_TYPES and kind == integer_type(value) or kind == "Z", "SAM text cannot say the type of an integer"
            fields.append("%s:%s:%s" % (name, "Z" if kind == "Z" else "i", value))
        lines.append("\t".join(fields))
    return ("\n".join(lines) + "\n").encode()


def bam_header(references):
    text = b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join([b"@SQ\tSN:%s\tLN:%d\n" % (name.encode(), length) for name, length in references])
    return b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(references)) + b"".join(
        struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<I", length) for name, length in references)


def bam_tags(tags):
    out = b""
    for name, kind, value in tags:
        if kind == "raw":
            out += name.encode() + value
            continue
        out += name.encode() + kind.encode()
        if kind in PACK:
            out += struct.pack(PACK[kind], value)
        elif kind == "Z":
            out += value.encode() + b"\0"
        else:
            assert kind == "B"
            out += value[0].encode() + struct.pack("<I", len(value[1])) + b"".join(struct.pack(PACK[value[0]], x) for x in value[1])
    return out


def bam_record(index_of, record):
    qname, flag, rname, pos, cigar, tags = record
    ref = -1 if rname == "*" else index_of[rname]
    ops = [] if cigar == "*" else [(int(length), CIGAR_OPS.index(op)) for length, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]
    body = struct.pack("<iiBBHHHiiii", ref, pos - 1, len(qname) + 1, 30 if ref >= 0 else 0, 4680, len(ops), flag, 0, -1, -1, 0)
    body += qname.encode() + b"\0" + b"".join(struct.pack("<I", length << 4 | op) for length, op in ops) + bam_tags(tags)
    return struct.pack("<i", len(body)) + body


def bam_records(case):
    index_of = {name: k for k, (name, _) in enumerate(case[0])}
    return b"".join(bam_record(index_of, record) for record in case[1])


# ---- the rule -------------------------------------------------------------------------------------------------------------------------------------------------------

def nh_of(tags):
    for name, kind, value in tags:
        if kind == "raw":  # the walk ends on a malformed field: what lies behind it is not seen
            return 1
        if name == "NH":  # the first field of that name decides, whatever follows it
            return value if kind in INTEGER_TYPES else 1
    return 1


def restate(annotation, case):
    """-> (text of the file, counts: {row name: [c0, c1, c2]}, {"records", "templates", "without_primary", "ends", "blocks"})"""
    references, records = case
    length_of = dict(references)
    genes_at = {}  # (contig, position) -> the genes that own an exon there: made from the sets of positions, to look a position up once instead of once per gene
    for gene in annotation["genes"]:
        for position in annotation["positions"][gene]:
            genes_at.setdefault((annotation["contig"][gene], position), set()).add(gene)
    ends = {}  # qname -> {slot: record}: the first primary record of a slot in file order
    for record in records:
        slots = ends.setdefault(record[0], {})
        flag = record[1]
        if flag & 0x900:
            continue
        slots.setdefault(1 if flag & 1 and flag & 0x80 else 0, record)
    counts = {row: [0, 0, 0] for row in SPECIAL + tuple(annotation["genes"])}
    stats = {"records": len(records), "templates": len(ends), "without_primary": 0, "ends": 0, "blocks": 0}
    for qname, slots in ends.items():
        if not slots:
            stats["without_primary"] += 1
            continue
        mapped = {slot: record for slot, record in slots.items() if not record[1] & 4 and record[2] != "*"}
        stats["ends"] += len(mapped)
        if not mapped:
            row = ["N_unmapped"] * 3
        elif any(nh_of(record[5]) > 1 for record in mapped.values()):
            row = ["N_multimapping"] * 3
        else:
            sets = [set(), set(), set()]
            for slot, (_, flag, rname, pos, cigar, tags) in mapped.items():
                if pos - 1 < 0:
                    continue
                forward = (not flag & 0x10) != (slot == 1)
                at, covered = pos - 1, set()
                for length, op in ([] if cigar == "*" else re.findall(r"(\d+)([MIDNSHP=X])", cigar)):
                    if op in "M=X":
                        covered.update(range(max(at, 0), min(at + int(length), length_of[rname])))
                    if op in "M=XDN":
                        at += int(length)
                stats["blocks"] += sum(1 for position in covered if position - 1 not in covered)  # maximal runs of positions
                for position in covered:
                    for gene in genes_at.get((rname, position), ()):
                        sets[0].add(gene)
                        sets[1 if (annotation["strand"][gene] == "+") == forward else 2].add(gene)
            row = ["N_noFeature" if not found else min(found) if len(found) == 1 else "N_ambiguous" for found in sets]
        for c in range(3):
            counts[row[c]][c] += 1
    text = "".join("%s\t%d\t%d\t%d\n" % ((row,) + tuple(counts[row])) for row in SPECIAL + tuple(annotation["genes"])).encode()
    return text, counts, stats


# ---- cases made at test time ------------------------------------------------------------------------------------------------------------------------------------------

def _exons(annotation):
    """(contig, first, last) of the maximal runs of positions of every gene, 0-based"""
    out = []
    for gene in annotation["genes"]:
        positions = annotation["positions"][gene]
        for first in sorted(p for p in positions if p - 1 not in positions):
            last = first
            while last + 1 in positions:
                last += 1
            out.append((annotation["contig"][gene], first, last))
    return out


def references_of(annotation):
    return sorted(annotation["lengths"].items()) + [("orphan", 100)]


def random_case(seed, annotation=None, max_records=400):
    """at most 400 records on the committed annotation: single reads and pairs that begin around the edges of exons, are spliced, clipped and deleted from, run past the end of their
    contig or lie on the reference without a contig; some carry NH in every integer type, behind other fields or as text; some mates are unmapped, some templates have secondary and
    supplementary records, a second primary record or no primary record; a part of the mates is moved to the end of the file"""
    annotation = annotation or load_annotation()
    generator = random.Random(seed)
    references, exons = references_of(annotation), _exons(annotation)
    length_of = dict(references)

    def alignment():
        choice = generator.random()
        if choice < 0.8:
            contig, first, last = generator.choice(exons)
            pos = max(1, generator.choice((first, last)) + 1 + generator.randint(-25, 5))
        elif choice < 0.9:
            contig = generator.choice(references)[0]
            pos = generator.randint(1, length_of[contig])
        else:
            contig = generator.choice(references)[0]
            pos = max(1, length_of[contig] - generator.randint(-5, 30))  # around the end of the contig, also behind it
        ops = []
        if generator.random() < 0.2:
            ops.append("%d%s" % (generator.randint(1, 9), generator.choice("SH")))
        for piece in range(generator.choice((1, 1, 1, 2, 2, 3))):
            if piece:
                ops.append("%d%s" % (generator.choice((1, 4, 10, 50, 100, 200, generator.randint(1, 300))), generator.choice("NNNDDIP")))
            ops.append("%d%s" % (generator.choice((1, 5, 20, 20, 25, generator.randint(1, 70))), generator.choice("MMMMM=X")))
        if generator.random() < 0.2:
            ops.append("%dS" % generator.randint(1, 9))
        return contig, pos, "".join(ops)

    def tags():
        choice = generator.random()
        if choice < 0.6:
            return []
        if choice < 0.75:
            return [("NH", "C", 1)]
        kind = generator.choice(INTEGER_TYPES + "Z")
        value = {"c": generator.choice((-1, 1, 2, 127)), "C": generator.choice((0, 1, 2, 255)), "s": generator.choice((-300, 1, 300)), "S": generator.choice((1, 300)),
                 "i": generator.choice((-70000, 1, 70000)), "I": generator.choice((1, 70000)), "Z": "7"}[kind]
        front = generator.choice(([], [("XZ", "Z", "some text")], [("XB", "B", ("s", [1, -2, 3]))], [("XA", "C", 9), ("XB", "B", ("I", []))]))
        return front + [("NH", kind, value)] + generator.choice(([], [("HI", "C", 1)]))

    records, late = [], []
    t = 0
    while len(records) + len(late) < max_records - 6:
        qname = "t%d_%d" % (seed, t)
        t += 1
        kind = generator.random()
        if kind < 0.35:  # a single read
            contig, pos, cigar = alignment()
            records.append((qname, generator.choice((0, 16)), contig, pos, cigar, tags()))
        elif kind < 0.8:  # a pair
            first, second = alignment(), alignment()
            if generator.random() < 0.7:
                second = (first[0], max(1, first[1] + generator.randint(-30, 200)), second[2])
            flags = generator.choice(((99, 147), (83, 163), (97, 145), (65, 129), (81, 161)))
            mates = [(qname, flags[0], first[0], first[1], first[2], tags()), (qname, flags[1], second[0], second[1], second[2], tags())]
            if generator.random() < 0.15:  # one mate unmapped
                k = generator.randrange(2)
                mates[k] = (qname, (mates[k][1] & ~0x32) | 4, mates[1 - k][2], mates[1 - k][3], "*", [])
                mates[1 - k] = (qname, (mates[1 - k][1] & ~2) | 8, ) + mates[1 - k][2:]
            if generator.random() < 0.5:
                mates.reverse()
            records.append(mates[0])
            (late if generator.random() < 0.2 else records).append(mates[1])
        elif kind < 0.85:  # unmapped
            if generator.random() < 0.5:
                records.append((qname, 4, "*", 0, "*", []))
            else:
                records += [(qname, 77, "*", 0, "*", []), (qname, 141, "*", 0, "*", [])]
        elif kind < 0.9:  # no primary record
            contig, pos, cigar = alignment()
            records.append((qname, generator.choice((256, 272, 2048)), contig, pos, cigar, tags()))
        else:  # a primary record with company: secondary, supplementary, a second primary
            contig, pos, cigar = alignment()
            records.append((qname, generator.choice((0, 16)), contig, pos, cigar, tags()))
            for _ in range(generator.randint(1, 2)):
                contig, pos, cigar = alignment()
                (late if generator.random() < 0.3 else records).append((qname, generator.choice((256, 2048, 2064, 0)), contig, pos, cigar, tags()))
    generator.shuffle(late)
    return references, records + late


def hot_case(annotation=None):
    """70 001 templates on GK, then a wavefront's worth spread over GA, GB and GJ: a count above 2^16 on one address"""
    annotation = annotation or load_annotation()
    spread = (("g1", 111), ("g1", 611), ("g1", 1311))
    return references_of(annotation), [("h%05d" % k, 0, "g1", 1631, "20M", []) for k in range(70001)] + [("w%02d" % k, 16 if k & 4 else 0) + spread[k % 3] + ("20M", []) for k in range(64)]


def wavefront_case(annotation=None):
    """65 templates, one past a wavefront, over every gene in turn"""
    annotation = annotation or load_annotation()
    exons = _exons(annotation)
    return references_of(annotation), [("v%02d" % k, 16 if k % 5 == 0 else 0, exons[k % len(exons)][0], exons[k % len(exons)][1] + 1, "4M", []) for k in range(65)]


def aux_case(annotation=None):
    """the corners of the NH walk, every read in GK: NH:Z in front of NH:i (the first field named NH decides: 1); a B array that announces more elements than the record holds, a
    field of an unknown type and a Z field without its NUL in front of NH:i:5 (the walk ends there: 1); and, to show that the same reads do count as multimapping when nothing is
    in the way, NH:i:5 alone and behind a well-formed B array"""
    annotation = annotation or load_annotation()
    five = ("NH", "C", 5)
    tags = [[("NH", "Z", "9"), five], [("XB", "raw", b"Bs" + struct.pack("<I", 1000) + b"\1\0"), five], [("XQ", "raw", b"?\7"), five], [("XZ", "raw", b"Zno end")],
            [five], [("XB", "B", ("s", [1, 2])), five]]
    return references_of(annotation), [("x%d" % k, 0, "g1", 1631, "20M", fields) for k, fields in enumerate(tags)]


def no_records_case(annotation=None):
    """a header and nothing behind it"""
    return references_of(annotation or load_annotation()), []


EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
COMMITTED_CONTIGS = "g1 g2 g3"  # of the committed annotation (only an interesting contig needs a sequence in the assembly)


def write_bgzf(path, payload, level):
    """payload as a BGZF file: stored blocks at level 0"""
    with open(path, "wb") as out:
        for at in range(0, len(payload), 0xff00):
            piece = payload[at:at + 0xff00]
            deflater = zlib.compressobj(level, zlib.DEFLATED, -15)
            body = deflater.compress(piece) + deflater.flush()
            out.write(struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(body) + 25) + body + struct.pack("<II", zlib.crc32(piece), len(piece)))
        out.write(EOF_BLOCK)


def stream_pipeline(session, sample):
    """a device pipeline whose read_chimeric_alignments stops behind agpu_ingest_finish: the cases made here have no chimeric reads, which the host's adoption of an ingest
    refuses; the record stream in HBM is what matters"""
    from arriba_amd.pipeline import DevicePipeline

    class StreamPipeline(DevicePipeline):
        def read_chimeric_alignments(self, bam, external_duplicate_marking=False, max_itd_length=100, piece_bytes=64 << 20):
            self._ingest_records(bam, external_duplicate_marking, max_itd_length, piece_bytes)
            self.device_ingest = True
            return 0
    return StreamPipeline(session, bam=sample)


def empty_case(annotation=None):
    """records, but none that is primary: every number of the file is 0"""
    annotation = annotation or load_annotation()
    return references_of(annotation), [("e1", 256, "g1", 111, "20M", []), ("e1", 272, "g1", 611, "20M", []), ("e2", 2048, "g2", 101, "20M", [])]
