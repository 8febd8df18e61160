"""What tests/test_virus_expression.py and tools/make_virus_golden.py share: cases of --virus-expression as plain data (references and alignment lines), their SAM text and their
BAM records, a restatement of the rule of DESIGN.md 4.11 in plain Python -- the independent side for inputs made at test time, allowed to serve as such only because it equals every
committed table --, the seeded random cases and the hand-made one.

A case is (references, records): references a list of (name, LN); records a list of (qname, flag, rname or "*", 1-based pos, cigar text or "*", seq text or "*")."""
import random
import re
import struct

SEQ_ALPHABET = "=ACMGRSVTWYHKDBN"
CIGAR_OPS = "MIDNSHP=X"
KMER, SHARED_PCT, MIN_COVERED_PCT, MIN_COVERED_BASES = 12, 10, 5, 100
HEADER_LINE = "VIRUS\tGENOME_SIZE\tCOVERED_BASES\tCOVERED_GENOME_FRACTION\tHIGH_QUALITY_ALIGNMENTS\tRPKM\n"
TANDEM = re.compile("|".join(".?".join([x + y] * 8) for x in "ACGT" for y in "ACGT"))
DEFAULT_VIRAL = r"^[AN]C_"


# ---- containers --------------------------------------------------------------------------------------------------------------------------------------------------

def sam_text(case):
    """the header holds the @SQ lines only (the script counts every other header line into its total)"""
    references, records = case
    lines = ["@SQ\tSN:%s\tLN:%d" % reference for reference in references]
    for qname, flag, rname, pos, cigar, seq in records:
        lines.append("\t".join([qname, str(flag), rname, str(pos), "30" if rname != "*" else "0", cigar, "*", "0", "0", seq, "*"]))
    return ("\n".join(lines) + "\n").encode()


def parse_sam(text):
    references, records = [], []
    for line in text.decode().split("\n"):
        if line.startswith("@SQ\t"):
            fields = dict(field.split(":", 1) for field in line.split("\t")[1:])
            references.append((fields["SN"], int(fields["LN"])))
        elif line and not line.startswith("@"):
            f = line.split("\t")
            records.append((f[0], int(f[1]), f[2], int(f[3]), f[5], f[9]))
    return references, records


def bam_header(references):
    text = b"@HD\tVN:1.6\tSO:unsorted\n" + b"".join([b"@SQ\tSN:%s\tLN:%d\n" % (name.encode(), length) for name, length in references])
    return b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(references)) + b"".join(
        struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<I", length) for name, length in references)


def bam_record(references, record):
    qname, flag, rname, pos, cigar, seq = record
    ref = -1 if rname == "*" else [name for name, _ in references].index(rname)
    ops = [] if cigar == "*" else [(int(length), CIGAR_OPS.index(op)) for length, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar)]
    bases = "" if seq == "*" else seq
    packed = bytearray((len(bases) + 1) // 2)
    for k, base in enumerate(bases):
        packed[k >> 1] |= SEQ_ALPHABET.index(base) << (0 if k & 1 else 4)
    body = struct.pack("<iiBBHHHiiii", ref, pos - 1, len(qname) + 1, 30 if ref >= 0 else 0, 4680, len(ops), flag, len(bases), -1, -1, 0)
    body += qname.encode() + b"\0" + b"".join(struct.pack("<I", length << 4 | op) for length, op in ops) + bytes(packed) + b"\xff" * len(bases)
    return struct.pack("<i", len(body)) + body


def bam_records(case):
    return b"".join(bam_record(case[0], record) for record in case[1])


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------------------------------

def awk_number(value):
    return "%d" % value if value == int(value) else "%.6g" % value


def restate(case, viral=DEFAULT_VIRAL):
    """-> (table text, counters); counters: total, and per index of a viral contig in the header reads, covered, kmer_count; shared[(i, j)] over the viruses with reads"""
    references, records = case
    is_viral = [re.search(viral, name) is not None for name, _ in references]
    index_of = {name: k for k, (name, _) in enumerate(references)}
    total, reads, covered, kmers = 0, {}, {}, {}
    for qname, flag, rname, pos, cigar, seq in records:
        if flag & 4:
            continue
        total += 1
        if not (flag & 2 or not flag & 1) or rname not in index_of or not is_viral[index_of[rname]]:
            continue
        if not re.fullmatch(r"(\d+[MNX])+", cigar) or TANDEM.search(seq):
            continue
        v = index_of[rname]
        reads[v] = reads.get(v, 0) + 1
        kmers.setdefault(v, set()).update(seq[i:i + KMER] for i in range(len(seq) - KMER))  # the last 12-mer of a read is never taken
        at = pos
        for length, op in re.findall(r"(\d+)([MNX])", cigar):
            if op != "N":
                covered.setdefault(v, set()).update(range(at, at + int(length)))
            at += int(length)
    rpkm = {v: 1000000000 * reads[v] / references[v][1] / total for v in reads if references[v][1] > 0 and total > 0}
    shared = {(i, j): len(kmers.get(i, set()) & kmers.get(j, set())) for i in reads for j in reads if i != j}
    removed = set()
    for i in rpkm:
        for j in rpkm:
            if i != j and (rpkm[i] > rpkm[j] or (rpkm[i] == rpkm[j] and i < j)) and shared[(i, j)] * 100 > len(kmers.get(j, ())) * SHARED_PCT:
                removed.add(j)
    rows = []
    for v in rpkm:
        n_covered, size = len(covered.get(v, ())), references[v][1]
        if v not in removed and n_covered >= MIN_COVERED_BASES and n_covered / size > MIN_COVERED_PCT / 100:
            rows.append("\t".join([references[v][0], str(size), str(n_covered), awk_number(n_covered / size), str(reads[v]), awk_number(rpkm[v])]))
    rows.sort(key=lambda line: (-float(line.split("\t")[5]), line.encode()))
    counters = {"total": total, "reads": reads, "covered": {v: len(s) for v, s in covered.items()}, "kmer_count": {v: len(s) for v, s in kmers.items()}, "shared": shared,
                "viral": [k for k, flag in enumerate(is_viral) if flag], "rpkm": rpkm, "removed": removed}
    return (HEADER_LINE + "".join(row + "\n" for row in rows)).encode(), counters


# ---- cases -------------------------------------------------------------------------------------------------------------------------------------------------------

def _bases(generator, n):
    """n random bases without a tandem repeat"""
    while True:
        text = "".join(generator.choice("ACGT") for _ in range(n))
        if not TANDEM.search(text):
            return text


FLAGS = (0, 1, 3, 4, 16, 65, 77, 83, 99, 129, 147, 163, 256, 272, 2064)


def random_case(seed, max_records=400):
    """2-12 viral contigs (related strains: a genome copied and mutated), non-viral ones between them, up to max_records records with every kind of CIGAR, flag and sequence"""
    g = random.Random(seed)
    genomes = []
    for k in range(g.randrange(2, 13)):
        if genomes and g.random() < 0.5:
            parent = g.choice(genomes)[1]
            rate = g.choice((0.0, 0.01, 0.03, 0.1))
            genome = "".join(g.choice("ACGT") if g.random() < rate else base for base in parent)
        else:
            genome = _bases(g, g.randrange(250, 1200))
        genomes.append(("%s_%06d.%d" % (g.choice(("NC", "AC")), g.randrange(1000000), g.randrange(1, 4)), genome))
    references = [(name, len(genome) + g.randrange(0, 50)) for name, genome in genomes] + [("1", 5000), ("chrM", 900), ("GL000219.1", 700), ("NCX_1", 400)]
    g.shuffle(references)
    genome_of = dict(genomes)
    busy = [name for name, _ in genomes if g.random() < 0.8] or [genomes[0][0]]
    records = []
    for k in range(g.randrange(max_records // 2, max_records + 1)):
        flag = g.choice(FLAGS) if g.random() < 0.4 else g.choice((0, 16, 99, 147))
        if flag & 4 and g.random() < 0.5:
            records.append(("r%d" % k, flag, "*", 0, "*", _bases(g, 30)))
            continue
        name = g.choice(busy) if g.random() < 0.8 else g.choice(references)[0]
        genome = genome_of.get(name) or _bases(g, dict(references)[name])
        length = g.choice((11, 12, 13, 14, 25, 37, 50, 75, 76))
        length = min(length, len(genome) - 1)
        pos = g.randrange(1, len(genome) - length + 1)
        seq = genome[pos - 1:pos - 1 + length]
        kind, cigar = g.random(), "%dM" % length
        if kind < 0.08 and length > 20:
            a = g.randrange(1, length - 1)
            gap = g.randrange(1, max(2, len(genome) - pos - length))
            cigar = "%dM%dN%dM" % (a, gap, length - a)
            seq = genome[pos - 1:pos - 1 + a] + genome[pos - 1 + a + gap:pos - 1 + gap + length]
        elif kind < 0.14 and length > 4:
            cigar = "%s1X%dM" % (g.choice(("2M", "2=")), length - 3)
        elif kind < 0.24 and length > 8:
            cigar = g.choice(("3S%dM" % (length - 3), "%dM3H" % length, "2M1I%dM" % (length - 3), "2M1D%dM" % (length - 2), "*"))
        if g.random() < 0.06 and length > 30:  # a tandem repeat somewhere in the read, with and without gaps; sometimes one copy short
            unit = g.choice("ACGT") + g.choice("ACGT")
            repeat = "".join(unit + (g.choice("ACGTN") if g.random() < 0.3 else "") for _ in range(g.choice((7, 8, 8, 9))))
            at = g.randrange(0, length - len(repeat) + 1) if len(repeat) <= length else 0
            seq = (seq[:at] + repeat + seq[at + len(repeat):])[:length]
        if g.random() < 0.08:
            at = g.randrange(length)
            seq = seq[:at] + "N" + seq[at + 1:]
        if g.random() < 0.03:
            seq = "*"
        records.append(("r%d" % k, flag, name, pos, cigar, seq))
    return references, records


def hand_made_case():
    """the smallest shapes at which the code can go wrong (the list of the issue, one contig per concern); returns (case, expectations), the expectations checked against the restatement here"""
    g = random.Random(20261019)
    references, records, serial = [], [], [0]

    def contig(name, length):
        references.append((name, length))
        return name

    def read(rname, pos, cigar, seq, flag=0):
        serial[0] += 1
        records.append(("h%d" % serial[0], flag, rname, pos, cigar, seq))

    def plain(rname, pos, seq, flag=0):
        read(rname, pos, "%dM" % len(seq), seq, flag)

    first = contig("NC_first", 2000)          # a viral contig in front of the non-viral ones; 101 of 2 000 covered: kept
    contig("1", 5000)
    tie1, tie2 = contig("NC_tie1", 800), contig("NC_tie2", 800)  # an RPKM tie between related strains, indices 2 and 3
    contig("GL000219.1", 700)
    contig("NC_noreads", 500)
    cov100of2000 = contig("NC_fraction", 2000)  # 100 of 2 000: exactly 0.05, dropped
    cov99, cov100 = contig("NC_bases99", 1000), contig("NC_bases100", 1000)
    cover = contig("AC_cover", 300)
    misc = contig("NC_misc", 3000)
    a, b, c = contig("NC_chainA", 600), contig("NC_chainB", 600), contig("NC_chainC", 600)
    keep_i, keep_j, drop_i, drop_j = contig("NC_keepI", 1000), contig("NC_keepJ", 1000), contig("NC_dropI", 1000), contig("NC_dropJ", 1000)
    equal1, equal2 = contig("NC_equal1", 1000), contig("NC_equal2", 1000)
    integral, exponent = contig("NC_integral", 1000), contig("AC_exponent", 120)

    plain(first, 1, _bases(g, 50)); plain(first, 1000, _bases(g, 51))
    tie_reads = [_bases(g, 40) for _ in range(5)]
    for name in (tie2, tie1):
        for k, seq in enumerate(tie_reads):
            plain(name, 1 + 40 * k, seq)
    plain(cov100of2000, 1, _bases(g, 50)); plain(cov100of2000, 1951, _bases(g, 50))
    for k in range(3):
        plain(cov99, 1 + 100 * k, _bases(g, 33))
    for k in range(4):
        plain(cov100, 1 + 100 * k, _bases(g, 25))
    # coverage: first and last base, across a 32- and a 64-position boundary (0-based 31|32 and 63|64), two overlapping reads
    for pos, length in ((1, 10), (291, 10), (20, 26), (50, 26), (100, 30), (115, 30)):
        plain(cover, pos, _bases(g, length))
    # reads of every shape on one contig, each in a slot of 60 positions of its own
    slot = [0]

    def misc_read(cigar, seq, flag=0, rname=misc):
        slot[0] += 1
        read(rname, 1 + 60 * slot[0], cigar, seq, flag)

    for length in (11, 12, 13, 37):
        misc_read("%dM" % length, _bases(g, length))
    misc_read("30M", "*")
    with_n = _bases(g, 30)
    misc_read("30M", with_n[:8] + "N" + with_n[9:])
    for cigar in ("30M", "15M200N15M", "2M1X27M", "2=1X27M", "3S27M", "27M3H", "2M1I27M", "2M1D28M", "*"):
        query = sum(int(n) for n, op in re.findall(r"(\d+)([MIS=X])", cigar)) or 30
        misc_read(cigar, _bases(g, query))
    slot[0] += 4  # (15M200N15M reaches 230 positions on)
    for flag in (0, 16, 99, 147, 65, 3, 256, 2064, 4):
        misc_read("30M", _bases(g, 30), flag)
    read("*", 0, "*", _bases(g, 30), 4)
    read("*", 0, "*", _bases(g, 30), 77)
    left, right = "GATTACAGGCTTAGCA", "TGCATCGGATACCGTA"  # flanks that hold no repeat
    tandems = [
        ("eight", left + "AC" * 8 + right, True), ("seven", left + "AC" * 7 + "G" + right, False),
        ("gaps", left + "ACTACNACACGACACAACAC" + right, True), ("two_gap", left + "ACACACACTTACACACAC" + right, False),
        ("odd_start", "G" + "CA" * 8 + right, True), ("at_end", left + "TG" * 8, True), ("sixteen_a", left[:7] + "A" * 16 + "C" + right[:6], True), ("two_units", left + "ACACACACAGAGAGAG" + right, False),
    ]
    for name, seq, matches in tandems:
        assert (TANDEM.search(seq) is not None) == matches, name
        misc_read("%dM" % len(seq), seq)
    # related strains in a chain: A removes B, B -- removed itself -- removes C, A and C share nothing
    x, z, p, q = (_bases(g, 150) for _ in range(4))

    def tile(rname, at, region, copies=1, pieces=3):
        for _ in range(copies):
            for k in range(pieces):
                plain(rname, at + 50 * k, region[50 * k:50 * k + 50])

    tile(a, 1, x, 2); tile(a, 151, p, 2)
    tile(b, 1, x); tile(b, 151, z); tile(b, 1, x, pieces=2)
    tile(c, 1, z); tile(c, 151, q, pieces=1)
    # shared * 10 == kmer_count: kept; one k-mer more: removed
    for strong, weak, length in ((keep_i, keep_j, 22), (drop_i, drop_j, 23)):
        common = _bases(g, length)
        for k in range(6):
            plain(strong, 1 + 50 * k, common if k == 0 else _bases(g, 42))
        plain(weak, 1, common)
        for k in range(3):
            plain(weak, 101 + 50 * k, _bases(g, 42))
    for name in (equal2, equal1):
        for k in range(4):
            plain(name, 1 + 50 * k, _bases(g, 40))
    for k in range(3):
        plain(integral, 1 + 50 * k, _bases(g, 40))
    hundred = _bases(g, 100)
    for k in range(70):
        plain(exponent, 1, hundred)
    mapped = sum(1 for record in records if not record[1] & 4)
    assert mapped <= 500
    for k in range(500 - mapped):
        plain("1" if k % 3 else "GL000219.1", 1 + k, _bases(g, 20), (0, 16, 99, 147)[k % 4])

    case = (references, records)
    text, counters = restate(case)
    index = {name: k for k, (name, _) in enumerate(references)}
    rows = {line.split("\t")[0]: line.split("\t") for line in text.decode().split("\n")[1:] if line}
    assert counters["total"] == 500
    assert first in rows and rows[first][2] == "101" and cov100of2000 not in rows and counters["covered"][index[cov100of2000]] == 100
    assert cov99 not in rows and counters["covered"][index[cov99]] == 99 and rows[cov100][2] == "100"
    assert rows[cover][2] == "117" and "NC_noreads" not in rows and index["NC_noreads"] not in counters["reads"]
    assert tie1 in rows and tie2 not in rows and counters["rpkm"][index[tie1]] == counters["rpkm"][index[tie2]]
    assert a in rows and b not in rows and c not in rows and counters["shared"][(index[a], index[c])] == 0
    assert counters["shared"][(index[keep_i], index[keep_j])] * 10 == counters["kmer_count"][index[keep_j]] and keep_j in rows
    assert counters["shared"][(index[drop_i], index[drop_j])] * 10 == counters["kmer_count"][index[drop_j]] + 9 and drop_j not in rows and drop_i in rows
    assert rows[equal1][5] == rows[equal2][5] and text.index(equal1.encode()) < text.index(equal2.encode())
    assert rows[integral][5] == "6000" and "e+" in rows[exponent][5]
    assert counters["reads"][index[misc]] == 4 + 2 + 3 + 7 + 3  # lengths; `*` and N; 30M, N and X; the flags 0 16 99 147 3 256 2064; the three reads without a repeat
    return case


def fixture_cases():
    """name -> case: what tools/make_virus_golden.py writes under tests/golden/virus_expression (toy3k comes from its dataset, not from here)"""
    cases = {"random%d" % seed: random_case(seed) for seed in range(1, 9)}
    cases["hand_made"] = hand_made_case()
    return cases
