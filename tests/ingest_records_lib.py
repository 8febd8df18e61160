"""Hand-dressed BAM records for the ingest (test tooling; `struct` and `hashlib` only).

tools/gen_synth writes records of one shape: the name `r%010d` (CIGAR and sequence always on a 4-byte boundary), the aux fields NH:C, HI:C and one fixed SA:Z in that order,
about 200 bytes per record.  redress() takes the uncompressed record stream of such a file and gives every record a new QNAME and a new aux block; fixed fields, CIGAR, sequence
and qualities stay.  All records of one old QNAME get the same new QNAME and an injective map of their HI values, so split reads, ITDs, read-throughs, multi-mappers and
duplicates stay what they were.  Every choice is a function of hashlib.sha256(old QNAME) (and of the flags of the records, to put the rare constructions on reads that end
up as chimeric fragments); nothing is drawn from `random`, the bytes are the same on every machine.

redress() returns the new stream and a table: class -> the new QNAMEs that carry it (plus "layout": record numbers of the constructions that are about sizes).
The classes are listed, with the code they aim at, in tests/test_ingest_records.py.
"""
import hashlib
import struct

ALPHABET = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789:_"   # (within [!-?A-~], no comma, no '#')
SPECIAL_LENGTHS = (2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 253, 254)                # (1 and 3 are "X" and "X,1")
DIFFERENCE_AT = (6, 7, 8, 9, 15, 16)                                           # index of the first byte that differs (7, 8, 9, 16 counted from 0 and from 1)
ARRAY_TYPES = "cCsSiIf"
ARRAY_WIDTH = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}
HI_CLASSES = ("C", "c", "c_negative", "s_negative", "S", "i", "I_above_2_31", "mixed_types", "A", "Z", "f", "i_negative", "s", "I", "mixed_types", "C")
PIECE_TARGETS = ("piece_16384", "piece_16385", "piece_16384_plus_misalignment")
PARSE_WINDOW = 16384    # agpu_ingest.hip
SEGMENT_BYTES = 8192    # ingest_core.hpp


def _digest_bytes(seed, n):
    out, counter = b"", 0
    while len(out) < n:
        out += hashlib.sha256(seed + b"/" + str(counter).encode()).digest()
        counter += 1
    return out[:n]


def _letters(seed, n):
    return "".join(ALPHABET[b & 63] for b in _digest_bytes(seed, n))


def first_record_offset(stream):
    assert stream[:4] == b"BAM\x01"
    at = 8 + struct.unpack_from("<I", stream, 4)[0]
    n_ref = struct.unpack_from("<I", stream, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 4 + struct.unpack_from("<I", stream, at)[0] + 4
    return at


def walk_aux(aux):
    """[(tag, type, value bytes)] of a well-formed aux block"""
    fields, at = [], 0
    while at < len(aux):
        tag, kind = aux[at:at + 2], chr(aux[at + 2])
        if kind in "AcC":
            size = 1
        elif kind in "sS":
            size = 2
        elif kind in "iIf":
            size = 4
        elif kind == "d":
            size = 8
        elif kind in "ZH":
            size = aux.index(b"\0", at + 3) - (at + 3) + 1
        elif kind == "B":
            size = 5 + ARRAY_WIDTH[chr(aux[at + 3])] * struct.unpack_from("<I", aux, at + 4)[0]
        else:
            raise ValueError("aux type %r" % kind)
        fields.append((tag, kind, aux[at + 3:at + 3 + size]))
        at += 3 + size
    assert at == len(aux)
    return fields


def parse_records(stream):
    """[dict] of the records of an uncompressed BAM stream, in stream order: offset, fixed (the 32 bytes), name (l_read_name bytes, NULs included), body (CIGAR, sequence,
    qualities), aux, flag, l_seq"""
    at, records = first_record_offset(stream), []
    while at < len(stream):
        block_size = struct.unpack_from("<I", stream, at)[0]
        fixed = stream[at + 4:at + 36]
        l_read_name, n_cigar, flag, l_seq = fixed[8], struct.unpack_from("<H", fixed, 12)[0], struct.unpack_from("<H", fixed, 14)[0], struct.unpack_from("<i", fixed, 16)[0]
        name_at = at + 36
        body_at = name_at + l_read_name
        aux_at = body_at + 4 * n_cigar + (l_seq + 1) // 2 + l_seq
        end = at + 4 + block_size
        assert aux_at <= end <= len(stream)
        records.append({"offset": at, "fixed": fixed, "name": stream[name_at:body_at], "body": stream[body_at:aux_at], "aux": stream[aux_at:end], "flag": flag, "l_seq": l_seq, "n_cigar": n_cigar})
        at = end
    return records


def qname_of(record):
    return record["name"].split(b"\0", 1)[0]


def encode_record(record):
    fixed = bytearray(record["fixed"])
    fixed[8] = len(record["name"])
    payload = bytes(fixed) + record["name"] + record["body"] + record["aux"]
    return struct.pack("<I", len(payload)) + payload


def _integer_field(tag, kind, value):
    return tag + kind.encode() + struct.pack({"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}[kind], value)


def _array_field(tag, kind, count, fill=None):
    width = ARRAY_WIDTH[kind]
    data = fill if fill is not None else bytes((17 * k + 3) & 0x7F for k in range(count * width))
    assert len(data) == count * width
    return tag + b"B" + kind.encode() + struct.pack("<I", count) + data


def padding_field(n):
    """an aux field of exactly n bytes (n >= 8)"""
    assert n >= 8
    return _array_field(b"XQ", "C", n - 8, b"\xAA" * (n - 8))


def _hit_index_field(hi_class, value, position):
    """(the HI field, the value bam_aux2i gives) of a record whose old HI was `value`; the map value -> new value is injective within a class"""
    if hi_class == "mixed_types":   # the same value on every record of the fragment, the type turns
        kind = "cCsSiI"[position % 6]
        return _integer_field(b"HI", kind, value), value
    if hi_class in ("A", "Z", "f"):  # (only dealt to names whose records all have HI 1) not an integer type: 0
        assert value == 1
        return {"A": b"HIA7", "Z": b"HIZ12\0", "f": b"HIf" + struct.pack("<f", 3.0)}[hi_class], 0
    kind, new = {"C": ("C", value), "c": ("c", value), "c_negative": ("c", -value), "s_negative": ("s", -(value + 200)), "S": ("S", value + 1000), "i": ("i", value + 100000),
                 "I_above_2_31": ("I", value + 3000000000), "i_negative": ("i", -(value + 70000)), "s": ("s", value + 300), "I": ("I", value + 5)}[hi_class]
    return _integer_field(b"HI", kind, new), new


def _extras(choice, seed):
    """aux fields that go in front of HI: (bytes, classes)"""
    d = _digest_bytes(seed + b"/extras", 8)
    if choice == 3:
        kind = ARRAY_TYPES[d[0] % 7]
        count = d[1] % 13
        return _array_field(b"XB", kind, count), ["hi_behind_B_" + kind] + (["hi_behind_B_count_0"] if count == 0 else [])
    if choice == 4:
        return b"XAA!" + b"Xff" + struct.pack("<f", 1.5) + b"Xdd" + struct.pack("<d", 2.5), ["hi_behind_A_f_d"]
    if choice == 5:   # the bytes of a HI:C:5 field and of the start of a SA:Z field inside a string
        return b"XZZ" + b"vHIC\x05wSAZx" + b"\0", ["decoy_in_Z"]
    if choice == 6:   # ... and inside an array, behind a hex string
        return b"XHH1AE3\0" + _array_field(b"XC", "C", 8, b"HIC\x05SAZ1"), ["decoy_in_B", "hi_behind_H"]
    if choice == 7:
        return b"XZZ" + _letters(seed + b"/z", 1 + d[2] % 9).encode() + b"\0", ["hi_behind_Z"]
    return b"", []


def redress(stream, salt=b""):
    header_end = first_record_offset(stream)
    records = parse_records(stream)
    table = {}

    def note(name, qname):
        table.setdefault(name, set()).add(qname)

    # ---- what the old stream says about every old QNAME
    reads, order = {}, []
    for index, record in enumerate(records):
        q = qname_of(record)
        if q not in reads:
            reads[q] = {"records": [], "digest": hashlib.sha256(salt + q).digest()}
            order.append(q)
        fields = {tag: (kind, value) for tag, kind, value in walk_aux(record["aux"])}
        record["hi"] = fields[b"HI"][1][0] if b"HI" in fields else None
        record["nh"] = fields[b"NH"][1] if b"NH" in fields else None
        record["sa"] = (b"SA" + fields[b"SA"][0].encode() + fields[b"SA"][1]) if b"SA" in fields else None
        reads[q]["records"].append(index)
    for q, read in reads.items():
        mine = [records[i] for i in read["records"]]
        read["split"] = any(r["sa"] is not None for r in mine)
        read["likely"] = read["split"] or any((r["flag"] & 1) and not (r["flag"] & 2) for r in mine)   # an SA field or a discordant mate: very likely a chimeric fragment
        read["all_hi_one"] = all(r["hi"] == 1 for r in mine)
        read["all_have_hi"] = all(r["hi"] is not None for r in mine)
    by_hash = sorted(order, key=lambda q: reads[q]["digest"])

    # ---- names
    new_name = {}   # old QNAME -> the l_read_name bytes of the new one
    singles = [q for q in by_hash if reads[q]["split"] and reads[q]["all_hi_one"] and len(reads[q]["records"]) == 3]   # (a whole split read of a unique hit)
    taken = iter(singles)

    def single(name_bytes, *classes, where=None):
        q = next(taken) if where is None else next(c for c in singles if c not in new_name and where(reads[c]["records"][0]))
        new_name[q] = name_bytes
        for c in classes:
            note(c, name_bytes.split(b"\0", 1)[0].decode())
        return q
    single(b"X\0", "length_1", "X_and_X,1")
    single(b"X,1\0", "length_3", "X_and_X,1", "comma")
    single(b"abc\0\0\0", "inner_nul")
    for length in SPECIAL_LENGTHS:
        single(("L%d_" % length + _letters(b"length%d" % length, 254))[:length].encode() + b"\0", "length_%d" % length)
    big20k = single(b"big20k_" + _letters(b"big20k", 6).encode() + b"\0", "record_20k")
    # (in the second half of the stream: a window of 1 MB of the stream lies in front of it)
    big100k = single(b"big100k" + _letters(b"big100k", 4).encode() + b"\0", "record_100k", where=lambda index: len(records) * 5 // 8 < index < len(records) * 7 // 8)
    used = set(new_name)
    pairs = {}
    for q in by_hash:
        read = reads[q]
        if q in used:
            continue
        d = read["digest"]
        u = d[0]
        length = (5 + d[1] % 14) if d[2] < 176 else (19 + d[1] % 50) if d[2] < 232 else (69 + (d[1] * 256 + d[3]) % 186)   # mostly short, a spread up to 254
        base = _letters(salt + q + b"/name", 254)
        if read["likely"] and u < 34:
            kind = "prefix" if u < 10 else "difference_at_%d" % DIFFERENCE_AT[(u - 10) // 4]
            waiting = pairs.pop(kind, None)
            if waiting is None:
                pairs[kind] = (q, base, length)
                continue
            other, other_base, other_length = waiting
            if kind == "prefix":
                shorter = "p" + other_base[:min(max(other_length, 4), 240)]
                names = (shorter, shorter + base[:1 + d[4] % 12])
            else:
                at = DIFFERENCE_AT[(u - 10) // 4]
                total = max(other_length, at + 1 + d[4] % 9)
                names = ("d" + other_base[:at - 1] + "a" + other_base[at:total - 1], "d" + other_base[:at - 1] + "b" + other_base[at:total - 1])
            for old, name in zip((other, q), names):
                new_name[old] = name.encode() + b"\0"
                note(kind, name)
            table.setdefault(kind + "_pairs", []).append(names)
            continue
        name = base[:length]
        if (read["likely"] and u < 50) or (not read["likely"] and u < 16):   # commas inside, at the end, two in a row
            at = d[4] % length
            name = (name[:at] + "," + name[at + 1:]) if d[5] % 3 else (name[:at] + ",," + name[at + 2:] + ",1")[:254]
            note("comma", name)
        new_name[q] = name.encode() + b"\0"
    for kind, (q, base, length) in pairs.items():   # (an odd one out)
        new_name[q] = base[:length].encode() + b"\0"
    plain = [bytes(n).split(b"\0", 1)[0] for n in new_name.values()]
    assert len(set(plain)) == len(plain) == len(reads), "two old names were dealt the same new name"
    assert all(0x21 <= b <= 0x7E and b != 0x40 for n in plain for b in n) and not any(n.startswith(b"#") for n in plain)

    # ---- aux blocks
    out = []
    for q in order:
        read = reads[q]
        d = read["digest"]
        hi_class = HI_CLASSES[d[6] % 16]
        if not read["all_have_hi"] and hi_class != "mixed_types":
            hi_class = "C"          # a record without HI counts as HI 1: the values stay
        if hi_class in ("A", "Z", "f") and not read["all_hi_one"]:
            hi_class = "mixed_types"  # (0 for every record would merge the hits of a multi-mapper)
        name = new_name[q]
        plain_name = name.split(b"\0", 1)[0].decode()
        note("hi_" + hi_class, plain_name)
        note("length_up_to_18" if len(plain_name) < 19 else "length_19_to_68" if len(plain_name) < 69 else "length_69_to_254", plain_name)
        for position, index in enumerate(read["records"]):
            record = records[index]
            seed = salt + q + b"/%d" % position
            e = _digest_bytes(seed, 8)
            nh = b"NHC" + record["nh"] if record["nh"] is not None else b""
            fields = []   # in front of HI
            if q == big20k and position == 0:
                fields.append(_array_field(b"XB", "S", 10240))
                note("hi_behind_B_S", plain_name)
            elif q == big100k and position == 1:
                fields.append(_array_field(b"XB", "I", 26000))
                note("hi_behind_B_I", plain_name)
            else:
                extra, classes = _extras(e[1] % 8, seed)
                fields.append(extra)
                if record["hi"] is not None:
                    for c in classes:
                        note(c, plain_name)
            hi = b""
            if record["hi"] is not None:
                hi, value = _hit_index_field(hi_class, record["hi"], position)
                hi = b"".join(fields) + hi
                if e[4] < 32:   # a second HI field: the first one counts
                    hi += b"HIC" + bytes([(value + 77) & 0xFF])
                    note("two_hi_fields", plain_name)
            else:
                hi = b"".join(fields)
                note("record_without_hi", plain_name)
                if record["flag"] & 256:
                    note("secondary_without_hi", plain_name)
            sa = record["sa"] or b""
            layout = e[0] % 4
            if layout == 1 and sa and record["hi"] is not None:
                note("hi_behind_SA", plain_name)
            aux = (nh + hi + sa, nh + sa + hi, sa + nh + hi, hi + nh + sa)[layout]
            body = bytearray(record["body"])
            if record["l_seq"] & 1 and e[5] >= 64:   # the unused low nibble of the last sequence byte
                body[4 * record["n_cigar"] + (record["l_seq"] + 1) // 2 - 1] |= 1 + e[5] % 15
                note("odd_length_nibble", plain_name)
            out.append({"fixed": record["fixed"], "name": name, "body": bytes(body), "aux": aux, "flag": record["flag"]})

    # ---- sizes: groups of 64 records (index a multiple of 64) whose piece, as record_parse_kernel computes it, has a chosen size
    layout = {}
    sizes = [len(encode_record(r)) for r in out]

    def offsets():
        result, at = [], header_end
        for size in sizes:
            result.append(at)
            at += size
        return result + [at]
    group, giants = 1, {i for i, s in enumerate(sizes) if s > 4096}
    for target in PIECE_TARGETS:
        while True:
            offset = offsets()
            base = 64 * group
            assert base + 64 < len(out), "no group of 64 records left for " + target
            misalignment = offset[base] & 15
            begin = offset[base] & ~15
            wanted = {"piece_16384": begin + PARSE_WINDOW, "piece_16385": begin + PARSE_WINDOW + 1, "piece_16384_plus_misalignment": offset[base] + PARSE_WINDOW}[target]
            missing = wanted - offset[base + 64]
            group += 1
            if missing >= 8 and not giants.intersection(range(base, base + 64)) and (misalignment != 0 or target == "piece_16384"):
                break
        out[base + 63]["aux"] += padding_field(missing)
        sizes[base + 63] += missing
        layout[target] = base
    # ---- the carrier of two false record starts: an unmapped record (no stage looks at it) whose array holds two well-formed headers exactly at the start of an 8 KB segment
    at = 64 * (group + 1)
    assert at < len(out)
    offset = offsets()[at]
    fake = struct.pack("<IiiBBHHHiiii", 40, 0, 5, 2, 0, 0, 0, 0, 0, -1, -1, 0) + b"y\0" + b"\0" * 6   # block_size 40: a complete, plausible record of 44 bytes
    carrier_head = 4 + 32 + 2 + 8
    pad = (header_end - offset - carrier_head) % SEGMENT_BYTES
    body = b"\xAA" * pad + fake + fake + b"\xFF" * 64
    assert (offset + carrier_head + pad - header_end) % SEGMENT_BYTES == 0
    carrier = {"fixed": struct.pack("<iiBBHHHiiii", -1, -1, 2, 0, 0, 0, 4, 0, -1, -1, 0), "name": b"x\0", "body": b"", "aux": b"ZZBC" + struct.pack("<I", len(body)) + body, "flag": 4}
    out.insert(at, carrier)
    layout["carrier"] = at
    table["layout"] = layout
    new_stream = stream[:header_end] + b"".join(encode_record(r) for r in out)
    return new_stream, {key: (sorted(value) if isinstance(value, set) else value) for key, value in table.items()}


def fragment_qname(fragment_name):
    """the QNAME of a fragment name of the reference ("QNAME,HI" or "QNAME,HIITD")"""
    return fragment_name.rsplit(",", 1)[0]


def piece_sizes(stream):
    """per group of 64 records: (piece size as record_parse_kernel computes it, misalignment of its first record)"""
    offsets = [r["offset"] for r in parse_records(stream)] + [len(stream)]
    return [(offsets[min(base + 64, len(offsets) - 1)] - (offsets[base] & ~15), offsets[base] & 15) for base in range(0, len(offsets) - 1, 64)]


# the base datasets (parameters of tools/gen_synth): one like toy3k; multi-mappers, a stranded library and ITD hotspots; an odd read length and secondaries without HI
DATASETS = {
    "plain3k": {"args": ["--seed", "11", "--fragments", "3000", "--contigs", "4", "--contig-len", "300000", "--junctions", "60"]},
    "multimappers3k": {"args": ["--seed", "23", "--fragments", "3000", "--normal-mult", "0.5", "--contigs", "4", "--contig-len", "300000", "--junctions", "60", "--multimap", "0.2", "--stranded", "--itd-hotspots", "2"]},
    "odd_length3k": {"args": ["--seed", "31", "--fragments", "3000", "--normal-mult", "0.5", "--contigs", "4", "--contig-len", "300000", "--junctions", "60", "--read-len", "75", "--multimap", "0.15", "--missing-hi", "0.5"]},
}


def write_dressed(base_prefix, prefix):
    """<base_prefix>.bam re-dressed into <prefix>.bam (a raw BAM stream; <prefix>.fa and .gtf are links to the base's); -> (prefix, table)"""
    import gzip
    import os
    stream, table = redress(gzip.open(base_prefix + ".bam", "rb").read())
    with open(prefix + ".bam", "wb") as out:
        out.write(stream)
    for suffix in (".fa", ".gtf"):
        if not os.path.exists(prefix + suffix):
            os.symlink(base_prefix + suffix, prefix + suffix)
    return prefix, table


def hit_index_of(record):
    """what bam_aux2i gives for the first HI field of a record, 1 without one"""
    for tag, kind, value in walk_aux(record["aux"]):
        if tag == b"HI":
            return struct.unpack({"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}[kind], value)[0] if kind in "cCsSiI" else 0
    return 1


def name_runs(stream):
    """fragment name ("QNAME,HI") -> (QNAME, the bytes of its records in stream order) of a re-dressed stream; the unmapped carrier is left out"""
    records = parse_records(stream)
    ends = [r["offset"] for r in records[1:]] + [len(stream)]
    runs = {}
    for record, end in zip(records, ends):
        if not record["flag"] & 4:
            q = qname_of(record)
            runs.setdefault(q + b"," + str(hit_index_of(record)).encode(), (q, []))[1].append(stream[record["offset"]:end])
    return runs


def in_name_order(stream, runs, without_commas=False, swap=None):
    """the records of a re-dressed stream (runs: name_runs(stream)) moved so that the fragment names ascend as std::string compares them; the records of a name keep their
    order.  without_commas: QNAMEs with a comma are left out.  swap=(a, b): two QNAMEs that are neighbours in that order change places (None if they are not).
    The reference's read table is a std::map: it does not depend on the order of the names in the file."""
    order = sorted(key for key in runs if not (without_commas and b"," in runs[key][0]))
    if swap is not None:
        a, b = ([i for i, key in enumerate(order) if runs[key][0] == q.encode()] for q in swap)
        if not (len(a) == len(b) == 1 and abs(a[0] - b[0]) == 1):
            return None
        order[a[0]], order[b[0]] = order[b[0]], order[a[0]]
    return stream[:first_record_offset(stream)] + b"".join(b"".join(runs[key][1]) for key in order)
