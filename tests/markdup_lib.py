"""What tests/test_mark_duplicates.py shares with tools/: a restatement of the rule of --mark-duplicates in plain Python dicts over parsed records, the SAM reader
and BAM writer of its cases (with qualities and mate fields, which tests/virus_expression_lib.py leaves out), a reader of the records of a written file, and the cases that are made
at test time.  The restatement is written from the rule, not from markdup_core.hpp, and shares nothing with the C++; it is the independent side for inputs made at test time only
because it gives tests/golden/mark_duplicates/hand_made.expected, which was worked out by hand, from hand_made.sam.

A case is (references, records): references a list of (name, LN); records a list of dicts with the eleven SAM fields qname, flag, rname, pos (1-based), mapq, cigar, rnext, pnext,
tlen, seq, qual."""
import random
import re
import struct
import zlib

from virus_expression_lib import CIGAR_OPS, SEQ_ALPHABET, bam_header  # noqa: F401

FIELDS = ("qname", "flag", "rname", "pos", "mapq", "cigar", "rnext", "pnext", "tlen", "seq", "qual")
DUPLICATE = 0x400


# ---- containers --------------------------------------------------------------------------------------------------------------------------------------------------

def parse_sam(text):
    references, records = [], []
    for line in text.decode().split("\n"):
        if line.startswith("@SQ\t"):
            fields = dict(field.split(":", 1) for field in line.split("\t")[1:])
            references.append((fields["SN"], int(fields["LN"])))
        elif line and not line.startswith("@"):
            f = line.split("\t")
            records.append({"qname": f[0], "flag": int(f[1]), "rname": f[2], "pos": int(f[3]), "mapq": int(f[4]), "cigar": f[5], "rnext": f[6], "pnext": int(f[7]), "tlen": int(f[8]), "seq": f[9], "qual": f[10]})
    return references, records


def sam_text(case):
    references, records = case
    lines = ["@HD\tVN:1.6\tSO:unsorted"] + ["@SQ\tSN:%s\tLN:%d" % reference for reference in references]
    lines += ["\t".join(str(record[field]) for field in FIELDS) for record in records]
    return ("\n".join(lines) + "\n").encode()


def bam_record(references, record):
    names = [name for name, _ in references]
    ref = -1 if record["rname"] == "*" else names.index(record["rname"])
    next_ref = -1 if record["rnext"] == "*" else ref if record["rnext"] == "=" else names.index(record["rnext"])
    ops = [] if record["cigar"] == "*" else [(int(length), CIGAR_OPS.index(op)) for length, op in re.findall(r"(\d+)([MIDNSHP=X])", record["cigar"])]
    bases = "" if record["seq"] == "*" else record["seq"]
    packed = bytearray((len(bases) + 1) // 2)
    for k, base in enumerate(bases):
        packed[k >> 1] |= SEQ_ALPHABET.index(base) << (0 if k & 1 else 4)
    qualities = b"\xff" * len(bases) if record["qual"] == "*" else bytes(ord(c) - 33 for c in record["qual"])
    assert len(qualities) == len(bases)
    qname = record["qname"].encode()
    body = struct.pack("<iiBBHHHiiii", ref, record["pos"] - 1, len(qname) + 1, record["mapq"], 4680, len(ops), record["flag"], len(bases), next_ref, record["pnext"] - 1, record["tlen"])
    body += qname + b"\0" + b"".join(struct.pack("<I", length << 4 | op) for length, op in ops) + bytes(packed) + qualities
    return struct.pack("<i", len(body)) + body


def bam_records(case):
    return b"".join(bam_record(case[0], record) for record in case[1])


def inflate_bgzf(data):
    """-> (payload, [(payload of the block, CRC-32 and ISIZE of its trailer)])"""
    at, payload, blocks = 0, [], []
    while at < len(data):
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04" and data[at + 12:at + 16] == b"BC\x02\x00"
        size = struct.unpack_from("<H", data, at + 16)[0] + 1
        piece = zlib.decompress(data[at + 18:at + size - 8], -15)
        blocks.append((piece, struct.unpack_from("<II", data, at + size - 8)))
        payload.append(piece)
        at += size
    return b"".join(payload), blocks


def file_records(data):
    """the records of a BAM file: [(offset of the record in the uncompressed stream, qname, flag)]"""
    stream = inflate_bgzf(data)[0]
    assert stream[:4] == b"BAM\x01"
    at = 8 + struct.unpack_from("<i", stream, 4)[0]
    n_ref = struct.unpack_from("<i", stream, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", stream, at)[0]
    records = []
    while at < len(stream):
        size = struct.unpack_from("<i", stream, at)[0]
        l_read_name = stream[at + 12]
        records.append((at, stream[at + 36:at + 36 + l_read_name - 1].decode(), struct.unpack_from("<H", stream, at + 18)[0]))
        at += 4 + size
    return records


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------------------------------

def _mapped(record):
    return not record["flag"] & 4 and record["rname"] != "*"


def _end_key(record, index_of):
    ops = [] if record["cigar"] == "*" else [(int(length), op) for length, op in re.findall(r"(\d+)([MIDNSHP=X])", record["cigar"])]
    pos = record["pos"] - 1
    if record["flag"] & 0x10:
        clipped = 0
        for length, op in reversed(ops):
            if op not in "SH":
                break
            clipped += length
        reference_length = sum(length for length, op in ops if op in "MDN=X") if ops else 1
        return (index_of[record["rname"]], pos + reference_length - 1 + clipped, 1)
    clipped = 0
    for length, op in ops:
        if op not in "SH":
            break
        clipped += length
    return (index_of[record["rname"]], pos - clipped, 0)


def _score(record):
    if record["qual"] == "*" or record["seq"] == "*":
        return 0
    return sum(ord(c) - 33 for c in record["qual"] if ord(c) - 33 >= 15) & 0xFFFFFFFF


def duplicate_names(case):
    """-> the set of the QNAMEs of the duplicate templates"""
    references, records = case
    index_of = {name: k for k, (name, _) in enumerate(references)}
    templates = {}
    for number, record in enumerate(records):
        template = templates.setdefault(record["qname"], {})
        if record["flag"] & 0x900 == 0:
            template.setdefault(1 if record["flag"] & 1 and record["flag"] & 0x80 else 0, number)
    pairs, fragments, pair_ends = {}, {}, set()
    for qname, ends in templates.items():
        mapped = [number for number in ends.values() if _mapped(records[number])]
        if not mapped:
            continue
        keys = sorted(_end_key(records[number], index_of) for number in mapped)
        order = (-(sum(_score(records[number]) for number in mapped) & 0xFFFFFFFF), min(ends.values()), qname)
        if len(mapped) == 2:
            pairs.setdefault(tuple(keys), []).append(order)
            pair_ends.update(keys)
        else:
            fragments.setdefault(keys[0], []).append(order)
    duplicates = set()
    for group in pairs.values():
        duplicates.update(qname for _, _, qname in sorted(group)[1:])
    for key, group in fragments.items():
        duplicates.update(qname for _, _, qname in sorted(group)[0 if key in pair_ends else 1:])
    return duplicates


def restate(case):
    """-> [0 or 1 per record]: whether it leaves with 0x400"""
    duplicates = duplicate_names(case)
    return [1 if record["qname"] in duplicates else 0 for record in case[1]]


def counts(case):
    """what agpu_markdup_stats reports, from the rule"""
    references, records = case
    marks = restate(case)
    names = set(record["qname"] for record in records)
    return {"templates": len(names), "records_flagged": sum(marks), "records_changed": sum(1 for mark, record in zip(marks, records) if mark != (1 if record["flag"] & DUPLICATE else 0))}


# ---- cases -------------------------------------------------------------------------------------------------------------------------------------------------------

def _record(qname, flag, rname, pos, cigar, qual=None, generator=None, mate=None):
    query = sum(int(length) for length, op in re.findall(r"(\d+)([MIS=X])", cigar)) if cigar != "*" else 10
    seq = "".join((generator or random).choice("ACGT") for _ in range(query))
    rnext, pnext = ("=", mate) if mate is not None else ("*", 0)
    return {"qname": qname, "flag": flag, "rname": rname, "pos": pos, "mapq": 30 if rname != "*" and not flag & 4 else 0, "cigar": cigar, "rnext": rnext, "pnext": pnext, "tlen": 0, "seq": seq,
            "qual": qual if qual is not None else "I" * query}


def random_case(seed, n_templates=120):
    """a few hundred records drawn from a handful of positions on two or three contigs, so that groups are large: pairs in all four orientations, fragments, unmapped mates,
    templates without a mapped record, clips on both sides, N and D, secondary and supplementary records, repeated primaries, input marks; the records shuffled"""
    g = random.Random(seed)
    references = [("m%d_%d" % (seed, k), g.randint(3000, 9000)) for k in range(g.randint(2, 3))]
    spots = [(g.randrange(len(references)), g.randint(20, 60) * 10) for _ in range(5)]
    records = []

    def aligned(qname, flag, spot, forward_u=None):
        """a record whose 5' coordinate is the spot's (mostly), whatever its clips"""
        t, u = spot
        u += g.choice((0, 0, 0, 0, 1))
        front, back = g.choice((0, 0, 2, 5)), g.choice((0, 0, 3))
        middle = g.choice(("20M", "8M30N12M", "10M2D10M", "10M2I8M", "20="))
        length = sum(int(n) for n, op in re.findall(r"(\d+)([MDN=X])", middle))
        cigar = ("%d%s" % (front, g.choice("SH")) if front else "") + middle + ("%d%s" % (back, g.choice("SH")) if back else "")
        if flag & 16:
            pos = u - back - length + 1  # 0-based: u = pos + length - 1 + back
        else:
            pos = u + front
        query = sum(int(n) for n, op in re.findall(r"(\d+)([MIS=X])", cigar))
        kind = g.random()
        qual = "*" if kind < 0.1 else "".join(chr(33 + g.choice((14, 15, 30, 40))) for _ in range(query)) if kind < 0.5 else chr(33 + g.choice((20, 30))) * query
        return _record(qname, flag | (DUPLICATE if g.random() < 0.15 else 0), references[t][0], pos + 1, cigar, qual, g, mate=1)

    for k in range(n_templates):
        qname, kind = "t%d_%d" % (seed, k), g.random()
        if kind < 0.45:  # a pair
            first_reverse, second_reverse = g.choice(((0, 16), (16, 0), (0, 0), (16, 16), (0, 16)))
            mine = [aligned(qname, 1 | 0x40 | first_reverse | (32 if second_reverse else 0), g.choice(spots)), aligned(qname, 1 | 0x80 | second_reverse | (32 if first_reverse else 0), g.choice(spots))]
        elif kind < 0.75:  # a single-end fragment
            mine = [aligned(qname, g.choice((0, 16)), g.choice(spots))]
        elif kind < 0.87:  # a read whose mate is unmapped
            end = aligned(qname, 1 | 8 | g.choice((0x40, 0x80)) | g.choice((0, 16)), g.choice(spots))
            mate = _record(qname, 1 | 4 | (0x40 if end["flag"] & 0x80 else 0x80) | (DUPLICATE if g.random() < 0.2 else 0), end["rname"], end["pos"], "*", None, g, mate=end["pos"])
            mine = [end, mate]
        else:  # nothing mapped
            mine = [_record(qname, 77 | (DUPLICATE if g.random() < 0.3 else 0), "*", 0, "*", None, g), _record(qname, 141, "*", 0, "*", None, g)]
        if g.random() < 0.15 and mine[0]["rname"] != "*":
            mine.append(aligned(qname, (mine[0]["flag"] & 0xC1) | g.choice((0x100, 0x800)) | g.choice((0, 16)), g.choice(spots)))
        if g.random() < 0.08 and mine[0]["rname"] != "*":
            mine.append(aligned(qname, mine[0]["flag"] & ~DUPLICATE & ~16 | g.choice((0, 16)), g.choice(spots)))  # a second primary of the slot
        records += mine
    g.shuffle(records)
    return references, records


def hot_case(n=70001):
    """n pairs at one key and n fragments on its forward end: exactly one template survives, the pair with the highest score"""
    references = [("hot1", 5000), ("hot2", 500)]
    g = random.Random(7)
    forward, reverse, single = _record("x", 99, "hot1", 1001, "20M", None, g, mate=1201), _record("x", 147, "hot1", 1201, "20M", None, g, mate=1001), _record("x", 0, "hot1", 1001, "20M", None, g)
    best = n // 3
    records = []
    for k in range(n):
        qual = "I" * 20 if k != best else "J" * 20
        records.append(dict(forward, qname="p%05d" % k, qual=qual))
        records.append(dict(reverse, qname="p%05d" % k, qual=qual))
    records += [dict(single, qname="f%05d" % k, qual="K" * 20) for k in range(n)]
    return (references, records), "p%05d" % best


def one_record_case():
    return [("o1", 1000)], [_record("only", 0, "o1", 11, "10M", None, random.Random(1))]


def unmapped_case():
    g = random.Random(2)
    return [("e1", 4000), ("e2", 90)], [_record("u1", 77, "*", 0, "*", None, g), _record("u1", 141 | DUPLICATE, "*", 0, "*", None, g), _record("u2", 4, "e1", 10, "*", None, g), _record("u3", 4 | DUPLICATE, "*", 0, "*", None, g)]


def straddle_case(flag_byte_at, n_records=400):
    """fragments at one end key with equal qualities -- every record but the first is a duplicate --, all of one size but the first, whose name is padded so that byte 19 of a
    later record lies at offset `flag_byte_at` of the sorted uncompressed stream (the input is in coordinate order already); returns (case, number of that record)"""
    references = [("s1", 100000)]
    fixed = _record("s0000", 0, "s1", 501, "100M", "I" * 100, random.Random(3))
    size = len(bam_record(references, fixed))
    pad = (flag_byte_at - 19 - size) % size
    assert 5 + pad < 255
    records = [dict(fixed, qname="s0000" + "x" * pad)] + [dict(fixed, qname="s%04d" % k) for k in range(1, n_records)]
    number = (flag_byte_at - 19 - (size + pad)) // size + 1
    assert 0 < number < n_records and (size + pad) + (number - 1) * size + 19 == flag_byte_at
    return (references, records), number
