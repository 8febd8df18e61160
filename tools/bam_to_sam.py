#!/usr/bin/env python3
"""BAM -> SAM text in pure Python (gzip/zlib + struct), written from the SAM specification alone (SAMv1 sections 1.4-1.5 and 4):
an independent decoder for the tests of the SAM text input, and a tool for looking at a BAM file where samtools is not at hand.

    python tools/bam_to_sam.py in.bam > out.sam
    from bam_to_sam import bam_to_sam; text, reference_names = bam_to_sam(open("in.bam", "rb").read())

The container may be BGZF (a series of gzip members), plain gzip or the uncompressed BAM stream."""
import struct
import sys
import zlib

CIGAR_OPS = "MIDNSHP=X"
BASES = "=ACMGRSVTWYHKDBN"
ARRAY_TYPES = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}


def inflate_all(data):
    """the uncompressed stream: every gzip member of `data` inflated and joined (BGZF is a series of members); bytes that are no gzip are returned as they are"""
    if data[:2] != b"\x1f\x8b":
        return bytes(data)
    parts = []
    while data[:2] == b"\x1f\x8b":
        member = zlib.decompressobj(16 + zlib.MAX_WBITS)
        parts.append(member.decompress(data))
        parts.append(member.flush())
        data = member.unused_data
    return b"".join(parts)


def format_float(value):
    """shortest decimal text that reads back as the same 32-bit float"""
    for digits in range(1, 10):
        text = "%.*g" % (digits, value)
        if struct.unpack("<f", struct.pack("<f", float(text)))[0] == value:
            return text
    return repr(value)


def format_tags(aux):
    fields = []
    at = 0
    while at < len(aux):
        tag, kind = aux[at:at + 2].decode("ascii"), chr(aux[at + 2])
        at += 3
        if kind == "A":
            fields.append("%s:A:%s" % (tag, chr(aux[at])))
            at += 1
        elif kind in "cCsSiI":
            code = ARRAY_TYPES[kind]
            fields.append("%s:i:%d" % (tag, struct.unpack_from("<" + code, aux, at)[0]))
            at += struct.calcsize(code)
        elif kind == "f":
            fields.append("%s:f:%s" % (tag, format_float(struct.unpack_from("<f", aux, at)[0])))
            at += 4
        elif kind in "ZH":
            end = aux.index(b"\0", at)
            fields.append("%s:%s:%s" % (tag, kind, aux[at:end].decode("latin-1")))
            at = end + 1
        elif kind == "B":
            subtype = chr(aux[at])
            count = struct.unpack_from("<I", aux, at + 1)[0]
            code = ARRAY_TYPES[subtype]
            values = struct.unpack_from("<%d%s" % (count, code), aux, at + 5)
            fields.append("%s:B:%s%s" % (tag, subtype, "".join("," + (format_float(v) if subtype == "f" else str(v)) for v in values)))
            at += 5 + count * struct.calcsize(code)
        else:
            raise ValueError("unknown type %r of optional field %s" % (kind, tag))
    return fields


def parse_header(stream):
    """(header text, [reference names], [reference lengths], offset of the first record) of an uncompressed BAM stream"""
    if stream[:4] != b"BAM\x01":
        raise ValueError("not a BAM file")
    l_text = struct.unpack_from("<i", stream, 4)[0]
    header_text = stream[8:8 + l_text].split(b"\0")[0]
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", stream, at)[0]
    at += 4
    names, lengths = [], []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", stream, at)[0]
        names.append(stream[at + 4:at + 4 + l_name - 1].decode("latin-1"))
        lengths.append(struct.unpack_from("<i", stream, at + 4 + l_name)[0])
        at += 8 + l_name
    return header_text, names, lengths, at


def record_lines(stream, at, end, names):
    """the alignment lines of the records stream[at:end]"""
    lines = []
    while at < end:
        at = _record_line(stream, at, names, lines)
    return lines


def bam_to_sam(data, with_header=True):
    """(text of the SAM file as bytes, [reference names]) of a BAM file given as bytes"""
    stream = inflate_all(data)
    header_text, names, lengths, at = parse_header(stream)
    lines = []
    if with_header:
        if header_text:
            lines.extend(line for line in header_text.decode("latin-1").split("\n") if line)
        if not any(line.startswith("@SQ") for line in lines):  # a BAM header may carry its references in the binary table only
            lines.extend("@SQ\tSN:%s\tLN:%d" % (name, length) for name, length in zip(names, lengths))
    lines.extend(record_lines(stream, at, len(stream), names))
    return ("\n".join(lines) + "\n").encode("latin-1"), names


def _record_line(stream, at, names, lines):
    """appends the line of the record at stream[at]; returns where the next record begins"""
    block_size = struct.unpack_from("<i", stream, at)[0]
    ref, pos, l_read_name, mapq, _bin, n_cigar, flag, l_seq, next_ref, next_pos, tlen = struct.unpack_from("<iiBBHHHiiii", stream, at + 4)
    record_end = at + 4 + block_size
    at += 36
    qname = stream[at:at + l_read_name - 1].decode("latin-1")
    at += l_read_name
    cigar = struct.unpack_from("<%dI" % n_cigar, stream, at)
    at += 4 * n_cigar
    packed = stream[at:at + (l_seq + 1) // 2]
    at += (l_seq + 1) // 2
    qual = stream[at:at + l_seq]
    at += l_seq
    aux = stream[at:record_end]
    at = record_end
    rname = names[ref] if ref >= 0 else "*"
    rnext = "*" if next_ref < 0 else ("=" if next_ref == ref else names[next_ref])
    sequence = "".join(BASES[packed[i >> 1] >> 4 if i % 2 == 0 else packed[i >> 1] & 15] for i in range(l_seq)) if l_seq else "*"
    quality = "*" if l_seq == 0 or qual[0] == 0xFF else bytes(q + 33 for q in qual).decode("latin-1")
    fields = [qname, str(flag), rname, str(pos + 1), str(mapq), "".join("%d%s" % (op >> 4, CIGAR_OPS[op & 15]) for op in cigar) or "*", rnext, str(next_pos + 1), str(tlen), sequence, quality]
    lines.append("\t".join(fields + format_tags(aux)))
    return at


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    with open(sys.argv[1], "rb") as handle:
        text, _ = bam_to_sam(handle.read())
    sys.stdout.buffer.write(text)


if __name__ == "__main__":
    main()
