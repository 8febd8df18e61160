#!/usr/bin/env python3
"""Splits a BAM file of STAR --chimOutType WithinBAM into what STAR --chimOutType SeparateSAMold would have written: the chimeric alignments in a file of
their own (the input of -c) and the main alignments (the input of -x).  Pure Python (zlib + struct), written from the SAM specification alone, as
tools/bam_to_sam.py is; for the tests of -c and for trying -c on data that was aligned the other way.

    python tools/split_chimeric.py in.bam chimeric.bam main.bam [--variant clean|full] [--keep-multimappers]

chimeric.bam gets every read-name group (records of one QNAME and one HI) that has a supplementary record or an SA tag -- the supplementary record re-flagged
0x800 -> 0x100, which is how Chimeric.out.sam marks it -- and every discordant pair (paired, not a proper pair).  main.bam gets, with --variant clean (the
default), everything that was not moved; with --variant full, the file as it was (the main alignments then hold the chimeric ones a second time, as the
main BAM file of a WithinBAM run passed with -x beside -c would).  Groups with HI > 1 stay where they are unless --keep-multimappers is given: the separate
file knows no hit index, several hits of one read collapse into one name there and are dropped as malformed.

Both outputs are uncompressed BAM streams wrapped in stored BGZF blocks."""
import struct
import sys
import zlib

sys.path.insert(0, __import__("os").path.dirname(__import__("os").path.abspath(__file__)))
from bam_to_sam import inflate_all, parse_header  # noqa: E402

FLAG_PAIRED, FLAG_PROPER_PAIR, FLAG_UNMAPPED, FLAG_MATE_UNMAPPED, FLAG_SECONDARY, FLAG_SUPPLEMENTARY = 1, 2, 4, 8, 0x100, 0x800


def records_of(stream, at):
    """(offset, end) of every record of the uncompressed stream from `at` on"""
    while at < len(stream):
        block_size = struct.unpack_from("<i", stream, at)[0]
        yield at, at + 4 + block_size
        at += 4 + block_size


def aux_tags(stream, at, end):
    """{tag: value or None} of the optional fields stream[at:end]; only integer values are decoded (HI), the others are None"""
    sizes = {"A": 1, "c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4, "d": 8}
    formats = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}
    tags = {}
    while at + 3 <= end:
        tag, kind = stream[at:at + 2].decode("latin-1"), chr(stream[at + 2])
        at += 3
        if kind in sizes:
            tags.setdefault(tag, struct.unpack_from(formats[kind], stream, at)[0] if kind in formats else None)
            at += sizes[kind]
        elif kind in "ZH":
            close = stream.index(b"\0", at)
            tags.setdefault(tag, None)
            at = close + 1
        elif kind == "B":
            element, count = chr(stream[at]), struct.unpack_from("<i", stream, at + 1)[0]
            tags.setdefault(tag, None)
            at += 5 + count * sizes[element]
        else:
            raise ValueError("unknown type of an optional field: %r" % kind)
    return tags


def describe(stream, at, end):
    """(QNAME, flag, HI or 1, has SA) of the record stream[at:end]"""
    l_read_name = stream[at + 12]
    n_cigar, flag = struct.unpack_from("<HH", stream, at + 16)
    l_seq = struct.unpack_from("<i", stream, at + 20)[0]
    name = bytes(stream[at + 36:at + 36 + l_read_name]).split(b"\0")[0]
    tags = aux_tags(stream, at + 36 + l_read_name + 4 * n_cigar + (l_seq + 1) // 2 + l_seq, end)
    hit_index = tags.get("HI")
    return name, flag, 1 if hit_index is None else hit_index, "SA" in tags


def bgzf_stored(stream):
    """the bytes as a BGZF file of stored blocks with the end-of-file marker"""
    out = []
    for begin in range(0, len(stream), 0xFF00):
        payload = bytes(stream[begin:begin + 0xFF00])
        deflated = b"\x01" + struct.pack("<HH", len(payload), len(payload) ^ 0xFFFF) + payload
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(deflated) + 25) + deflated + struct.pack("<II", zlib.crc32(payload), len(payload)))
    out.append(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    return b"".join(out)


def split(data, variant="clean", keep_multimappers=False):
    """(bytes of the chimeric file, bytes of the main file, number of records moved) of a WithinBAM file given as bytes"""
    if variant not in ("clean", "full"):
        raise ValueError("variant: clean or full")
    stream = inflate_all(data)
    first_record = parse_header(stream)[3]
    records = [(at, end) + describe(stream, at, end) for at, end in records_of(stream, first_record)]
    chimeric_groups = set()
    for at, end, name, flag, hit_index, has_sa in records:
        if flag & (FLAG_UNMAPPED | FLAG_SECONDARY) and not flag & FLAG_SUPPLEMENTARY:
            continue  # (neither kind starts a chimeric group; a secondary record of a moved group moves with it)
        discordant = flag & FLAG_PAIRED and not flag & FLAG_PROPER_PAIR and not flag & FLAG_MATE_UNMAPPED
        if (flag & FLAG_SUPPLEMENTARY or has_sa or discordant) and (hit_index == 1 or keep_multimappers):
            chimeric_groups.add((name, hit_index))
    header = bytes(stream[:first_record])
    chimeric, main, moved = [header], [header], 0
    for at, end, name, flag, hit_index, has_sa in records:
        record = bytes(stream[at:end])
        if (name, hit_index) in chimeric_groups:
            moved += 1
            if flag & FLAG_SUPPLEMENTARY:
                record = record[:18] + struct.pack("<H", (flag & ~FLAG_SUPPLEMENTARY) | FLAG_SECONDARY) + record[20:]
            chimeric.append(record)
            if variant == "full":
                main.append(bytes(stream[at:end]))
        else:
            main.append(record)
    return bgzf_stored(b"".join(chimeric)), bgzf_stored(b"".join(main)), moved


def main():
    arguments = [a for a in sys.argv[1:] if not a.startswith("--")]
    variant = "clean"
    if "--variant" in sys.argv:
        variant = sys.argv[sys.argv.index("--variant") + 1]
        arguments.remove(variant)
    if len(arguments) != 3:
        sys.exit(__doc__)
    chimeric, main_file, moved = split(open(arguments[0], "rb").read(), variant, "--keep-multimappers" in sys.argv)
    open(arguments[1], "wb").write(chimeric)
    open(arguments[2], "wb").write(main_file)
    print("%d records moved to %s" % (moved, arguments[1]), file=sys.stderr)


if __name__ == "__main__":
    main()
