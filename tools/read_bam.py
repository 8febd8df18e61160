"""tools/read_bam.py -- a BAM reader and a BAI reader with a region query, in plain Python (zlib + struct), written from the SAM specification (SAMv1 sections 4.1, 4.2,
5.1.1, 5.2, 5.3).  The independent side of tests/test_sorted_bam.py: it walks the BGZF blocks itself and checks BSIZE, CRC-32, ISIZE and the end-of-file block of every file.

    python tools/read_bam.py FILE.bam [REF:BEGIN-END]     summary, or the records of a region through FILE.bam.bai (0-based, half open)
"""
import struct
import sys
import zlib

EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
CONSUMES_REFERENCE = (0, 2, 3, 7, 8)  # M D N = X


class BamError(ValueError):
    pass


def bgzf_blocks(raw):
    """[(file offset, payload)] of every block; checks the gzip member, the BC subfield, BSIZE, CRC-32, ISIZE, and that the file ends with the EOF block"""
    blocks, at = [], 0
    while at < len(raw):
        if len(raw) - at < 18:
            raise BamError("truncated block header at %d" % at)
        id1, id2, cm, flg, _, _, _, xlen = struct.unpack_from("<BBBBIBBH", raw, at)
        if (id1, id2, cm) != (31, 139, 8) or not flg & 4:
            raise BamError("no BGZF block at %d" % at)
        extra, bsize = raw[at + 12:at + 12 + xlen], None
        field = 0
        while field + 4 <= len(extra):
            si1, si2, slen = struct.unpack_from("<BBH", extra, field)
            if (si1, si2) == (66, 67):
                if slen != 2:
                    raise BamError("BC subfield of %d bytes at %d" % (slen, at))
                bsize = struct.unpack_from("<H", extra, field + 4)[0]
            field += 4 + slen
        if bsize is None:
            raise BamError("no BC subfield at %d" % at)
        size = bsize + 1
        if at + size > len(raw):
            raise BamError("BSIZE runs past the end of the file at %d" % at)
        deflated = raw[at + 12 + xlen:at + size - 8]
        crc, isize = struct.unpack_from("<II", raw, at + size - 8)
        inflater = zlib.decompressobj(-15)
        payload = inflater.decompress(deflated) + inflater.flush()
        if not inflater.eof or inflater.unused_data:
            raise BamError("BSIZE does not end with the deflate stream at %d" % at)
        if len(payload) != isize:
            raise BamError("ISIZE %d, payload %d at %d" % (isize, len(payload), at))
        if zlib.crc32(payload) != crc:
            raise BamError("CRC-32 mismatch at %d" % at)
        blocks.append((at, payload))
        at += size
    if not blocks or raw[blocks[-1][0]:] != EOF_BLOCK:
        raise BamError("no end-of-file block")
    return blocks


def is_stored(raw, offset):
    """the block at `offset` is one stored deflate block (0x01, LEN, ~LEN)"""
    xlen = struct.unpack_from("<H", raw, offset + 10)[0]
    at = offset + 12 + xlen
    length, inverse = struct.unpack_from("<HH", raw, at + 1)
    return raw[at] == 1 and length ^ inverse == 0xFFFF


class Record(object):
    __slots__ = ("bytes", "start", "ref", "pos", "flag", "end", "name")

    def __init__(self, data, start):
        block_size = struct.unpack_from("<i", data, start)[0]
        if block_size < 32 or start + 4 + block_size > len(data):
            raise BamError("bad block_size at uncompressed offset %d" % start)
        self.start = start
        self.bytes = bytes(data[start:start + 4 + block_size])
        self.ref, self.pos, l_read_name, _, _, n_cigar, self.flag = struct.unpack_from("<iiBBHHH", self.bytes, 4)
        self.name = self.bytes[36:36 + l_read_name - 1]
        length = 0
        if not self.flag & 4:
            for op in struct.unpack_from("<%dI" % n_cigar, self.bytes, 36 + l_read_name):
                if op & 15 in CONSUMES_REFERENCE:
                    length += op >> 4
        self.end = self.pos + (length if length > 0 else 1)  # (an unmapped record or an empty CIGAR covers one base, as for htslib's indexer)


class BamFile(object):
    def __init__(self, path):
        self.raw = open(path, "rb").read()
        self.blocks = bgzf_blocks(self.raw)
        self.data = b"".join(payload for _, payload in self.blocks)
        self.block_start = {}  # file offset of a block -> uncompressed offset of its payload
        at = 0
        for offset, payload in self.blocks:
            self.block_start[offset] = at
            at += len(payload)
        self.block_start[len(self.raw)] = at
        data = self.data
        if data[:4] != b"BAM\x01":
            raise BamError("no BAM magic")
        l_text = struct.unpack_from("<i", data, 4)[0]
        self.text = data[8:8 + l_text]
        n_ref = struct.unpack_from("<i", data, 8 + l_text)[0]
        at = 12 + l_text
        self.references = []
        for _ in range(n_ref):
            l_name = struct.unpack_from("<i", data, at)[0]
            name = data[at + 4:at + 4 + l_name]
            if not name.endswith(b"\0"):
                raise BamError("reference name without NUL")
            self.references.append((name[:-1].decode(), struct.unpack_from("<i", data, at + 4 + l_name)[0]))
            at += 8 + l_name
        self.header_size = at
        self.records = []
        while at < len(data):
            record = Record(data, at)
            self.records.append(record)
            at += len(record.bytes)

    def uncompressed_offset(self, virtual_offset):
        return self.block_start[virtual_offset >> 16] + (virtual_offset & 0xFFFF)

    def records_between(self, begin, end):
        """the records from virtual offset `begin` up to (not including) the one at `end`"""
        at, stop = self.uncompressed_offset(begin), self.uncompressed_offset(end)
        while at < stop:
            record = Record(self.data, at)
            yield record
            at += len(record.bytes)


class BaiFile(object):
    """references: [{"bins": {bin: [(begin, end)]}, "linear": [offsets], "pseudo": (begin, end, mapped, unmapped) or None}]; n_no_coor (None if the file ends before it)"""

    def __init__(self, path):
        raw = open(path, "rb").read()
        if raw[:4] != b"BAI\x01":
            raise BamError("no BAI magic")
        n_ref = struct.unpack_from("<i", raw, 4)[0]
        at = 8
        self.references = []
        for _ in range(n_ref):
            n_bin = struct.unpack_from("<i", raw, at)[0]
            at += 4
            bins, pseudo = {}, None
            for _ in range(n_bin):
                number, n_chunk = struct.unpack_from("<Ii", raw, at)
                at += 8
                chunks = [struct.unpack_from("<QQ", raw, at + 16 * k) for k in range(n_chunk)]
                at += 16 * n_chunk
                if number == 37450:
                    if n_chunk != 2:
                        raise BamError("pseudo-bin with %d chunks" % n_chunk)
                    pseudo = chunks[0] + chunks[1]
                else:
                    if number > 37449 or number in bins:
                        raise BamError("bad or repeated bin %d" % number)
                    bins[number] = chunks
            n_intv = struct.unpack_from("<i", raw, at)[0]
            at += 4
            linear = list(struct.unpack_from("<%dQ" % n_intv, raw, at))
            at += 8 * n_intv
            self.references.append({"bins": bins, "linear": linear, "pseudo": pseudo})
        self.n_no_coor = struct.unpack_from("<Q", raw, at)[0] if at + 8 <= len(raw) else None
        if at + (8 if self.n_no_coor is not None else 0) != len(raw):
            raise BamError("bytes behind the index")


def reg2bin(begin, end):
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if begin >> shift == end >> shift:
            return base + (begin >> shift)
    return 0


def reg2bins(begin, end):
    end -= 1
    bins = [0]
    for shift, base in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        bins.extend(range(base + (begin >> shift), base + (end >> shift) + 1))
    return bins


def query(bam, bai, reference, begin, end):
    """the records that overlap [begin, end) of reference number `reference`, found through the index: the chunks of the bins of the region whose end lies above the linear-index
    offset of the region's first window, read from their virtual offsets, filtered by overlap; in file order, every record once"""
    if begin >= end:
        return []
    index = bai.references[reference]
    window = begin >> 14
    minimum = index["linear"][window] if window < len(index["linear"]) else 0
    found = {}
    for number in reg2bins(begin, end):
        for chunk_begin, chunk_end in index["bins"].get(number, ()):
            if chunk_end <= minimum:
                continue
            for record in bam.records_between(chunk_begin, chunk_end):
                if record.ref == reference and record.pos < end and record.end > begin:
                    found[record.start] = record
    return [found[start] for start in sorted(found)]


def brute_force(bam, reference, begin, end):
    if begin >= end:
        return []
    return [record for record in bam.records if record.ref == reference and record.pos < end and record.end > begin]


def main(arguments):
    bam = BamFile(arguments[0])
    if len(arguments) == 1:
        print("%d blocks, %d references, %d records, %d bytes uncompressed" % (len(bam.blocks), len(bam.references), len(bam.records), len(bam.data)))
        return 0
    bai = BaiFile(arguments[0] + ".bai")
    name, _, span = arguments[1].rpartition(":")
    begin, end = (int(v) for v in span.split("-"))
    for record in query(bam, bai, [n for n, _ in bam.references].index(name), begin, end):
        print("%s\t%d\t%s\t%d\t%d" % (record.name.decode(), record.flag, name, record.pos, record.end))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
