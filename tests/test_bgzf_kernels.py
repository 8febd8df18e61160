"""The container kernels of the device ingest (arriba_amd/csrc/device/agpu_ingest.hip: bgzf_unwrap_kernel, bgzf_inflate_tokens_kernel<16|20|24>, bgzf_inflate_resolve_kernel,
bgzf_inflate_kernel, bgzf_crc_kernel<false|true>) on the GPU against Python's zlib, through agpu_bgzf_unpack -- the launch code of agpu_ingest_push_bgzf over a caller's blocks.

Every expectation is zlib's: a block is made with zlib.compressobj(level, DEFLATED, -15, 8, strategy), a stream is valid if and only if zlib.decompressobj(-15) reaches its end,
a CRC-32 is zlib.crc32.  Nothing here comes from the project's own decoders; tests/emu/inflate_check.cpp (the same cores stepped on the host) is only asked which blocks of
this corpus pass 1 hands back, so that `handed_back >= 1` on the device is a condition that is known to be met."""
import collections
import ctypes
import functools
import gzip
import os
import random
import struct
import subprocess
import zlib

import numpy as np
import pytest

import conftest

KINDS = ("random bytes", "ACGT text", "one run", "period 251", "matches from 33 000 back", "skewed", "16-value hash", "chains of short matches")
SIZES = (0, 1, 2, 100, 4097, 20000, 65280, 65536)
LEVELS = (0, 1, 6, 9)
STRATEGIES = (("default", zlib.Z_DEFAULT_STRATEGY), ("fixed", zlib.Z_FIXED), ("huffman_only", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE), ("filtered", zlib.Z_FILTERED))
WAYS = (0, 16, 24, -1)
GUARD, FILL = 64, 0xCD
INFLATE_MATCH_CAPACITY = 8192  # inflate_fast_core.hpp: a block with more matches goes back to the one-wavefront-per-block decoder
BLOCK_DTYPE = np.dtype([("raw_offset", "<u8"), ("payload_offset", "<u4"), ("payload_size", "<u4"), ("stream_offset", "<u8"), ("crc32", "<u4"), ("isize", "<u4"), ("skip", "<u4"), ("keep", "<u4")])

# payload: the DEFLATE stream (stored path: the data); isize: what the table says it inflates to; data: what the stream must hold afterwards, None = nothing is known of it
Entry = collections.namedtuple("Entry", "label payload isize data")


# ---- the corpus ---------------------------------------------------------------------------------------------------------------------------------------------

def _deflate(data, level, strategy):
    compressor = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return compressor.compress(data) + compressor.flush()


def _zlib_inflate(payload, limit=70000):
    """the bytes if zlib.decompressobj(-15) reaches the end of the stream, else None"""
    stream = zlib.decompressobj(-15)
    try:
        data = stream.decompress(payload, limit)
    except zlib.error:
        return None
    return data if stream.eof else None


@functools.lru_cache(maxsize=None)
def _kind_data(kind):
    """65 536 bytes of one kind (the eight kinds of tests/emu/inflate_check.cpp, restated); the data of a size are its first bytes"""
    n = 65536
    rng = np.random.RandomState(1000 + kind)
    i = np.arange(n, dtype=np.int64)
    if kind == 0:
        data = rng.randint(0, 256, n)
    elif kind == 1:
        data = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.randint(0, 4, n)]
    elif kind == 2:
        data = np.full(n, ord("A"))
    elif kind == 3:
        data = i % 251
    elif kind == 4:  # matches from far back (beyond the 8 KB ring of the wave decoder): every source lies in the random part
        data = rng.randint(0, 256, n)
        data[40000:] = data[i[40000:] - 33000 + i[40000:] % 7]
    elif kind == 5:  # long and short codes
        data = np.where(rng.randint(0, 100, n) < 97, ord("x"), rng.randint(0, 256, n))
    elif kind == 6:
        data = ((i * 2654435761) & 0xFFFFFFFF) >> 24 & 15
    else:  # chains of short matches that read each other's output (many rounds in pass 2), periods below 8
        fresh, literal, back = rng.randint(0, 256, n), rng.randint(0, 5, n) == 0, rng.randint(0, 1 << 30, n)
        data = [0] * n
        for k in range(n):
            data[k] = fresh[k] if k < 64 or literal[k] else data[k - 1 - back[k] % 12]
        data = np.array(data)
    return data.astype(np.uint8).tobytes()


def _short_matches_block():
    """more matches than pass 1 can note, by construction: three bytes that occurred 4 bytes before, then a byte that breaks the match -- 16 384 matches of length 3 in 64 KB"""
    rng = np.random.RandomState(77)
    data = bytearray(rng.randint(0, 256, 65536).astype(np.uint8).tobytes())
    for k in range(4, 65536):
        if k % 4 != 3:
            data[k] = data[k - 4]
        elif data[k] == data[k - 4]:
            data[k] ^= 0x55
    return bytes(data)


@functools.lru_cache(maxsize=None)
def _corpus():
    """8 kinds x 8 sizes x 4 levels x 5 strategies, one data set per (kind, size); + one block built to be handed back"""
    entries = []
    for kind in range(len(KINDS)):
        for size in SIZES:
            data = _kind_data(kind)[:size]
            for level in LEVELS:
                for name, strategy in STRATEGIES:
                    entries.append(Entry("%s, %d bytes, level %d, %s" % (KINDS[kind], size, level, name), _deflate(data, level, strategy), size, data))
    data = _short_matches_block()
    entries.append(Entry("3-byte matches alternating with a literal, 65536 bytes, level 6, default", _deflate(data, 6, zlib.Z_DEFAULT_STRATEGY), len(data), data))
    return tuple(entries)


def _entry(label):
    return next(entry for entry in _corpus() if entry.label == label)


ACGT_HANDED_BACK = "ACGT text, 65536 bytes, level 6, default"


@functools.lru_cache(maxsize=None)
def _damaged():
    """every corpus block of more than 100 bytes with one bit of its DEFLATE stream flipped"""
    rng = random.Random(11)
    entries, verdicts = [], []
    for entry in _corpus():
        if entry.isize <= 100:
            continue
        payload = bytearray(entry.payload)
        payload[rng.randrange(len(payload))] ^= 1 << rng.randrange(8)
        theirs = _zlib_inflate(bytes(payload))
        entries.append(Entry("damaged: " + entry.label, bytes(payload), entry.isize, theirs if theirs is not None and len(theirs) == entry.isize else None))
        verdicts.append(theirs)
    return tuple(entries), tuple(verdicts)


# ---- dynamic headers written by hand (tests/emu/inflate_check.cpp: handmade_block / canonical) ------------------------------------------------------------------------

class _Bits(object):
    def __init__(self):
        self.value, self.n = 0, 0

    def put(self, value, n):  # (lowest bit first)
        self.value |= (value & ((1 << n) - 1)) << self.n
        self.n += n

    def put_code(self, code, length):  # (a Huffman code: its first bit first)
        for k in range(length - 1, -1, -1):
            self.put((code >> k) & 1, 1)

    def bytes(self):
        return self.value.to_bytes((self.n + 7) // 8, "little")


def _canonical(lengths):
    count = [0] * 16
    for length in lengths:
        count[length] += 1
    count[0] = 0
    following, code = [0] * 16, 0
    for length in range(1, 16):
        code = (code + count[length - 1]) << 1
        following[length] = code
    codes = [0] * len(lengths)
    for symbol, length in enumerate(lengths):
        if length:
            codes[symbol] = following[length]
            following[length] += 1
    return codes


def _handmade_block(litlen, distance, tokens):
    """A dynamic block whose code-length code gives every length 0..15 a 4-bit code (complete), so that any set of lengths can be written down, also those a compressor never
    makes.  tokens: (literal, -1) or (length symbol, distance symbol), symbols without extra bits.  Returns (stream, bytes the tokens stand for)."""
    w = _Bits()
    w.put(1, 1); w.put(2, 2); w.put(len(litlen) - 257, 5); w.put(len(distance) - 1, 5); w.put(19 - 4, 4)
    for symbol in (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15):
        w.put(4 if symbol < 16 else 0, 3)
    for length in list(litlen) + list(distance):
        w.put_code(length, 4)  # (lengths 0..15 all have 4 bits: the canonical code of the length value v is v)
    litlen_codes, distance_codes = _canonical(litlen), _canonical(distance)
    produced = 0
    for symbol, far in tokens:
        w.put_code(litlen_codes[symbol], litlen[symbol])
        if far >= 0:
            w.put_code(distance_codes[far], distance[far])
        produced += 1 if far < 0 else 3 + (symbol - 257)
    w.put_code(litlen_codes[256], litlen[256])
    return w.bytes(), produced


def _named_headers():
    a, b = ord("a"), ord("b")
    cases = []
    litlen, distance = [0] * 257, [0]

    def add(what, tokens):
        cases.append((what, list(litlen), list(distance), tokens))
    litlen[256] = 1; add("a single end-of-block code of one bit, no distance code", [])
    litlen[a] = 1; add("two codes of one bit, no distance code", [(a, -1), (a, -1)])
    litlen[a] = 2; litlen[256] = 2; add("incomplete literal / length code", [(a, -1)])
    litlen[b] = 2; litlen[ord("c")] = 2; litlen[ord("d")] = 2; add("over-subscribed literal / length code", [(a, -1)])
    litlen = [0] * 258
    litlen[a] = 2; litlen[b] = 2; litlen[256] = 2; litlen[257] = 2  # (257: length 3)
    distance = [0, 0]
    distance[0] = 1; add("a single distance code of one bit", [(a, -1), (257, 0)])
    distance[0] = 2; add("a single distance code of two bits (incomplete)", [(a, -1), (257, 0)])
    distance[1] = 2; add("two distance codes of two bits (incomplete)", [(a, -1), (257, 0)])
    distance[0] = 1; distance[1] = 1; add("two distance codes of one bit", [(a, -1), (b, -1), (257, 1), (257, 0)])
    distance = [0]
    add("a match without any distance code", [(a, -1), (257, 0)])
    add("no distance code, literals only", [(a, -1), (b, -1)])
    return cases


def _random_headers(trials):
    """random sets of code lengths, a quarter of them neither complete nor checked for anything; literals and matches with codes of up to 15 bits"""
    rng = random.Random(7)

    def random_code(n, complete, must_have):
        lengths = [0] * n
        if not complete:
            for s in range(n):
                lengths[s] = 0 if rng.randrange(3) else 1 + rng.randrange(15)
            if must_have >= 0 and lengths[must_have] == 0:
                lengths[must_have] = 1 + rng.randrange(15)
            return lengths
        if n < 2:
            lengths[0] = rng.randrange(2)
            return lengths
        leaves, wanted = [0], 2 + rng.randrange(n - 1)  # a complete code: leaves of a binary tree split at random until there are enough
        while len(leaves) < wanted:
            k = rng.randrange(len(leaves))
            if leaves[k] >= 15:
                if all(leaf >= 15 for leaf in leaves):
                    break
                continue
            leaves[k] += 1
            leaves.append(leaves[k])
        symbols = list(range(n))
        rng.shuffle(symbols)
        if must_have >= 0:
            k = symbols.index(must_have)
            symbols[0], symbols[k] = symbols[k], symbols[0]
        for k, leaf in enumerate(leaves):
            lengths[symbols[k]] = leaf
        return lengths
    cases = []
    for trial in range(trials):
        n_litlen, n_distance = 257 + rng.randrange(30), 1 + rng.randrange(30)
        complete = rng.randrange(4) != 0
        litlen, distance = random_code(n_litlen, complete, 256), random_code(n_distance, complete or rng.randrange(2) == 1, -1)
        tokens, produced = [], 0
        for _ in range(200):
            symbol = rng.randrange(n_litlen)
            if litlen[symbol] == 0 or symbol == 256:
                continue
            if symbol < 256:
                tokens.append((symbol, -1)); produced += 1
                continue
            if symbol > 264 or produced == 0:  # (length and distance codes without extra bits)
                continue
            far = rng.randrange(4)
            if far >= n_distance or distance[far] == 0 or far + 1 > produced:
                continue
            tokens.append((symbol, far)); produced += 3 + (symbol - 257)
        cases.append(("random code %d" % trial, litlen, distance, tokens))
    return cases


@functools.lru_cache(maxsize=None)
def _handmade():
    """(entries, zlib's verdicts): a refused stream is given the size its tokens stand for -- a decoder that took the header would find nothing else wrong with it"""
    entries, verdicts = [], []
    for what, litlen, distance, tokens in _named_headers() + _random_headers(1200):
        payload, produced = _handmade_block(litlen, distance, tokens)
        theirs = _zlib_inflate(payload)
        entries.append(Entry("hand-made header: " + what, payload, produced if theirs is None else len(theirs), theirs))
        verdicts.append(theirs)
    return tuple(entries), tuple(verdicts)


# ---- CPU tier: the generator checks itself ------------------------------------------------------------------------------------------------------------------------

def test_corpus_blocks_are_what_they_are_meant_to_be():
    """every block inflates with zlib to its data; Z_FIXED gives fixed-Huffman blocks (BTYPE 01 in the first byte of the stream) and level 0 stored ones (BTYPE 00)"""
    corpus = _corpus()
    assert len(corpus) == len(KINDS) * len(SIZES) * len(LEVELS) * len(STRATEGIES) + 1
    fixed = []
    for entry in corpus:
        assert _zlib_inflate(entry.payload) == entry.data and len(entry.data) == entry.isize, entry.label
        block_type = entry.payload[0] >> 1 & 3
        if ", level 0," in entry.label:
            assert block_type == 0, entry.label
        elif entry.label.endswith(", fixed"):  # (zlib stores a block that the fixed code would make longer than it is, whatever the strategy: trees.c, _tr_flush_block)
            assert block_type == 1 or (block_type == 0 and len(entry.payload) > len(entry.data)), entry.label
            fixed.append(block_type)


    assert len(fixed) == len(KINDS) * len(SIZES) * 3 and 4 * fixed.count(1) >= 3 * len(fixed), fixed.count(1)


def test_hand_made_headers_are_two_sided():
    """zlib accepts at least a third of the hand-made headers and refuses at least a fifth (the C++ corpus: 2 971 of 4 010 accepted); of the ten named cases both kinds"""
    entries, verdicts = _handmade()
    accepted = sum(1 for theirs in verdicts if theirs is not None)
    assert len(entries) >= 1010
    assert 3 * accepted >= len(entries) and 5 * (len(entries) - accepted) >= len(entries), (accepted, len(entries))
    named = verdicts[:10]
    assert any(theirs is None for theirs in named) and any(theirs is not None for theirs in named)
    for entry, theirs in zip(entries, verdicts):
        if theirs is not None:
            assert len(theirs) == entry.isize, entry.label


def test_damaged_streams_are_two_sided():
    """of the streams with one bit flipped zlib refuses some, inflates some to another size and most -- a changed literal or stored byte -- to the same size: every branch of the
    GPU test is walked"""
    entries, verdicts = _damaged()
    refused = sum(1 for theirs in verdicts if theirs is None)
    same_size = sum(1 for entry, theirs in zip(entries, verdicts) if theirs is not None and len(theirs) == entry.isize)
    assert len(entries) == (len(_corpus()) - 1) // 2 + 1 and refused >= 30 and same_size >= 30 and len(entries) - refused - same_size >= 30, (len(entries), refused, same_size)


def test_pass_one_hands_blocks_of_the_corpus_back(built, tmp_path):
    """`handed_back >= 1` of the GPU tests is a condition, not a measurement: inflate_tokens (inflate_fast_core.hpp) stepped on the host over this corpus returns INFLATE_RETRY
    for the block that is built to hold 16 384 matches and for the 64 KB of ACGT text the partial-block test uses"""
    directory = os.path.join(conftest.ROOT, "tests", "emu")
    subprocess.run(["make", "-s", "-C", directory, "inflate_check"], check=True)
    corpus = _corpus()
    with open(str(tmp_path / "corpus.bin"), "wb") as out:
        out.write(struct.pack("<I", len(corpus)))
        for entry in corpus:
            out.write(struct.pack("<II", len(entry.payload), entry.isize) + entry.payload)
    result = subprocess.run([os.path.join(directory, "inflate_check"), "--handed-back", str(tmp_path / "corpus.bin")], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    assert result.returncode == 0 and result.stdout.startswith("handed back:"), result.stdout[-2000:]
    handed_back = set(corpus[int(index)].label for index in result.stdout.split(":")[1].split())
    assert corpus[-1].label in handed_back and ACGT_HANDED_BACK in handed_back, sorted(handed_back)


# ---- GPU tier -----------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def device(built):
    """(api, context) of the device library; one context for the module"""
    from arriba_amd import _capi
    api = _capi.bind_device_api(_capi.device_library())
    params = _capi.Params()
    api.default_params(ctypes.byref(params))
    context = api.create(0, ctypes.byref(params))
    assert context, api.last_error()
    assert BLOCK_DTYPE.itemsize == ctypes.sizeof(_capi.BgzfBlock)
    yield api, context
    api.destroy(context)


Unpacked = collections.namedtuple("Unpacked", "entries out expected offsets written status handed_back crc_mismatches")


def _unpack(device, entries, way, stored=False, partial=None, crcs=None):
    """One call of agpu_bgzf_unpack.  The blocks lie in `raw` as in a BGZF file (18-byte header, DEFLATE stream, trailer), the way the feeder hands them on; block k goes to a
    stream offset that is k mod 4 and has 64 bytes of 0xCD in front of the next block.  partial: {index: (skip, keep)}; crcs: {index: the CRC-32 for the table}."""
    from arriba_amd import _capi
    api, context = device
    partial, crcs = partial or {}, crcs or {}
    table = np.zeros(len(entries), dtype=BLOCK_DTYPE)
    raw, offsets, written, at = bytearray(), [], [], 0
    for k, entry in enumerate(entries):
        skip, keep = partial.get(k, (0, entry.isize))
        payload = entry.payload
        table[k]["raw_offset"], table[k]["payload_offset"], table[k]["payload_size"] = len(raw), 18 + (5 if stored else 0), len(payload)
        if stored:
            payload = b"\x01" + struct.pack("<HH", len(payload), len(payload) ^ 0xFFFF) + payload
        crc = crcs.get(k, 0 if k in partial else zlib.crc32(entry.data if entry.data is not None else b"") & 0xFFFFFFFF)
        raw += struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, ord("B"), ord("C"), 2, (len(payload) + 25) & 0xFFFF) + payload + struct.pack("<II", crc, entry.isize)
        at += (k - at) % 4
        offsets.append(at); written.append(keep)
        table[k]["stream_offset"], table[k]["crc32"] = at, crc
        if not stored:
            table[k]["isize"], table[k]["skip"], table[k]["keep"] = entry.isize, skip, keep
        at += keep + GUARD
    assert set(offset % 4 for offset in offsets[:4]) == set(range(min(4, len(entries))))
    out = np.full(at, FILL, dtype=np.uint8)
    expected = out.copy()
    for k, entry in enumerate(entries):
        if entry.data is not None:
            skip = partial.get(k, (0, 0))[0]
            expected[offsets[k]:offsets[k] + written[k]] = np.frombuffer(entry.data[skip:skip + written[k]], dtype=np.uint8)
    status = np.full(len(entries), -1, dtype=np.int32)
    handed_back, crc_mismatches = ctypes.c_uint32(12345), ctypes.c_uint32(12345)
    rc = api.bgzf_unpack(context, bytes(raw), len(raw), table.ctypes.data_as(ctypes.POINTER(_capi.BgzfBlock)), len(entries), way,
                         out.ctypes.data, len(out), status.ctypes.data, ctypes.byref(handed_back), ctypes.byref(crc_mismatches))
    assert rc == 0, api.last_error()
    return Unpacked(entries, out, expected, offsets, written, status, handed_back.value, crc_mismatches.value)


def _wrong(result, refused=()):
    """labels of the blocks whose bytes or status are not the expected ones (blocks in `refused` must have a status, their bytes are their own affair), and of the blocks with a
    damaged guard behind them"""
    wrong = []
    for k, entry in enumerate(result.entries):
        at, n = result.offsets[k], result.written[k]
        if k in refused or entry.data is None:
            if k in refused and result.status[k] == 0:
                wrong.append("accepted: " + entry.label)
        elif result.status[k] != 0 or not np.array_equal(result.out[at:at + n], result.expected[at:at + n]):
            wrong.append("status %d: %s" % (result.status[k], entry.label))
        end = result.offsets[k + 1] if k + 1 < len(result.entries) else len(result.out)
        if not (result.out[at + n:end] == FILL).all():
            wrong.append("guard behind: " + entry.label)
    if not (result.out[:result.offsets[0]] == FILL).all():
        wrong.append("bytes in front of the first block")
    return wrong


@pytest.mark.gpu
@pytest.mark.parametrize("way", WAYS)
def test_every_kind_of_block_inflates_to_what_zlib_gives(way, device):
    """the whole corpus in one call: stored sub-blocks, fixed and dynamic codes, Huffman-only, distance-1 runs, matches from 32 KB back, chains of short matches, blocks that
    pass 1 hands back; with 16, 20 and 24 blocks per wavefront in pass 1 and with the one-wavefront-per-block decoder alone"""
    result = _unpack(device, _corpus(), way)
    wrong = _wrong(result)
    assert not wrong, (way, len(wrong), wrong[:10])
    assert np.array_equal(result.out, result.expected)
    assert result.crc_mismatches == 0
    if way == -1:
        assert result.handed_back == 0
    else:
        assert 1 <= result.handed_back < len(result.entries) // 4, result.handed_back  # (test_pass_one_hands_blocks_of_the_corpus_back: at least two)


@pytest.mark.gpu
def test_block_counts_around_the_launch_shapes(device):
    """the last workgroup of pass 1 (16, 20, 24 blocks each) partly filled, full, and one block over; the same for the four wavefronts of a workgroup of pass 2 and of the CRC"""
    pool = [entry for entry in _corpus() if entry.isize in (100, 4097, 20000) and (", level 6," in entry.label or ", level 0, default" in entry.label)]
    assert len(pool) >= 85
    for way, count in [(0, n) for n in (1, 19, 20, 21, 24, 25, 41, 85)] + [(16, 15), (16, 16), (16, 17), (24, 23), (24, 24), (24, 25), (-1, 1), (-1, 5)]:
        entries = [pool[(7 * k + count) % len(pool)] for k in range(count)]
        result = _unpack(device, entries, way)
        wrong = _wrong(result)
        assert not wrong and result.crc_mismatches == 0, (way, count, wrong[:10])


@pytest.mark.gpu
@pytest.mark.parametrize("way", [0, -1])
def test_first_and_last_block_of_a_part_of_a_file(way, device):
    """skip / keep: the first and the last block go through the spill buffer and only their share reaches the stream -- ordinary blocks, and 64 KB of ACGT text that pass 1 hands
    back (there the other decoder copies the share); their CRC field is 0, not checked, as the feeder sets it"""
    ordinary = [_entry("skewed, 20000 bytes, level 6, default"), _entry("period 251, 4097 bytes, level 9, default"), _entry("chains of short matches, 65536 bytes, level 1, default"),
                _entry("matches from 33 000 back, 65536 bytes, level 6, default")]
    acgt = _entry(ACGT_HANDED_BACK)
    for entries, first, last in ((ordinary, (19000, 1000), (0, 12345)), (ordinary[:3], (1, 19999), (65000, 535)), ([acgt, ordinary[1], ordinary[0], acgt], (4097, 61439), (3, 60001)),
                                 ([acgt, ordinary[1], acgt], (65535, 1), (0, 1))):
        assert first[0] > 0 and first[0] + first[1] == entries[0].isize and last[1] < entries[-1].isize - last[0]
        result = _unpack(device, entries, way, partial={0: first, len(entries) - 1: last})
        wrong = _wrong(result)
        assert not wrong and result.crc_mismatches == 0, (way, [entry.label for entry in entries], wrong)
        assert np.array_equal(result.out, result.expected)
        if entries[0] is acgt:
            assert result.handed_back == (2 if way == 0 else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("way", [0, -1])
def test_damaged_streams_are_refused_or_decoded_as_zlib_does(way, device):
    """one bit flipped in every block of more than 100 bytes: what zlib refuses is refused, what zlib inflates to another size is refused, what zlib inflates to the same size
    is refused or gives zlib's bytes; never a byte outside the block's place"""
    entries, verdicts = _damaged()
    result = _unpack(device, entries, way)
    must_refuse = set(k for k, theirs in enumerate(verdicts) if theirs is None or len(theirs) != entries[k].isize)
    wrong = _wrong(result, refused=must_refuse)
    for k, theirs in enumerate(verdicts):
        at = result.offsets[k]
        if k not in must_refuse and result.status[k] == 0 and result.out[at:at + entries[k].isize].tobytes() != theirs:
            wrong.append("decoded differently: " + entries[k].label)
    wrong = [line for line in wrong if not line.startswith("status ")]  # (a stream zlib takes may still be refused here)
    assert not wrong, (way, len(wrong), wrong[:10])


@pytest.mark.gpu
@pytest.mark.parametrize("way", [0, -1])
def test_hand_made_dynamic_headers_get_the_verdict_of_zlib(way, device):
    """incomplete, over-subscribed, single-symbol and empty codes, codes of up to 15 bits (second-level tables; the blocks whose tables a lane has no room for are handed back):
    accepted if and only if zlib accepts, and then zlib's bytes"""
    entries, verdicts = _handmade()
    result = _unpack(device, entries, way)
    wrong = _wrong(result, refused=set(k for k, theirs in enumerate(verdicts) if theirs is None))
    assert not wrong, (way, len(wrong), wrong[:10])


def _btype_3(entry):
    """the block with the reserved block type in its first header: refused before a byte is written"""
    return Entry("block type 3: " + entry.label, bytes([entry.payload[0] | 6]) + entry.payload[1:], entry.isize, None)


@pytest.mark.gpu
def test_crc_of_inflated_blocks_on_the_device(device):
    """a wrong CRC-32 in the table of every seventh block is counted, and nothing else; a refused block among the blocks leaves the count of the others as it was (its place holds
    no byte of the block, so it is counted too)"""
    corpus = list(_corpus())
    wrong_crcs = {}
    for k in range(3, len(corpus), 7):
        crc = (zlib.crc32(corpus[k].data) ^ 0x5A5A5A5A) & 0xFFFFFFFF
        wrong_crcs[k] = crc if crc != 0 else 1  # (0 in the table: not to be checked)
    result = _unpack(device, corpus, 0, crcs=wrong_crcs)
    assert not _wrong(result) and result.crc_mismatches == len(wrong_crcs)
    bad = next(k for k, entry in enumerate(corpus) if k not in wrong_crcs and entry.label == "16-value hash, 20000 bytes, level 6, default")
    true_crc = zlib.crc32(corpus[bad].data) & 0xFFFFFFFF
    assert _zlib_inflate(_btype_3(corpus[bad]).payload) is None and zlib.crc32(bytes([FILL]) * 20000) & 0xFFFFFFFF != true_crc and true_crc != 0
    corpus[bad] = _btype_3(corpus[bad])
    wrong_crcs[bad] = true_crc
    result = _unpack(device, corpus, 0, crcs=wrong_crcs)
    assert not _wrong(result, refused={bad}) and result.status[bad] != 0
    assert (result.out[result.offsets[bad]:result.offsets[bad] + 20000] == FILL).all()
    assert result.crc_mismatches == len(wrong_crcs)


@pytest.mark.gpu
def test_stored_blocks_are_moved_and_checked(device):
    """bgzf_unwrap_kernel with payloads shorter than its head / word / tail split and at the ends of its loops, from an unaligned source (blocks back to back behind 18-byte
    headers + 5 bytes) to stream offsets of every alignment; bgzf_crc_kernel<false> on the same payloads: no mismatch, then exactly the blocks with a changed byte"""
    rng = np.random.RandomState(5)
    sizes = list(range(0, 301)) + list(range(4093, 4101)) + [65279, 65280, 65535]
    entries = []
    for size in sizes:
        data = rng.randint(0, 256, size).astype(np.uint8).tobytes()
        entries.append(Entry("stored, %d bytes" % size, data, size, data))
    result = _unpack(device, entries, 0, stored=True)
    wrong = _wrong(result)
    assert not wrong and result.crc_mismatches == 0 and result.handed_back == 0, wrong[:10]
    assert np.array_equal(result.out, result.expected) and set(offset % 4 for offset in result.offsets) == {0, 1, 2, 3}
    changed, crcs = list(entries), {}
    for k in range(1, len(entries), 9):  # (sizes 1, 10, 19, ...: the first is a payload of one byte)
        data = bytearray(entries[k].data)
        data[(k * 7919) % len(data)] ^= 1 << (k % 8)
        changed[k] = Entry(entries[k].label + ", one byte changed", bytes(data), entries[k].isize, bytes(data))
        crcs[k] = zlib.crc32(entries[k].data) & 0xFFFFFFFF
        assert crcs[k] != 0
    result = _unpack(device, changed, 0, stored=True, crcs=crcs)
    assert not _wrong(result) and result.crc_mismatches == len(crcs) >= 30


def _bgzf_member(chunk, level, strategy):
    data = _deflate(chunk, level, strategy)
    if len(data) + 26 > 65536:  # (BSIZE has 16 bits)
        return None
    return struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, ord("B"), ord("C"), 2, len(data) + 25) + data + struct.pack("<II", zlib.crc32(chunk) & 0xFFFFFFFF, len(chunk))


def _mixed_file(stream):
    """the stream as BGZF members of 1, 997, 0xff00 and 65 536 bytes in turn, every (level, strategy) in turn -- level 0 first: the file begins with stored blocks and goes
    on with deflated ones --, three empty members in the middle.  A member holds at most 64 KB: a chunk that does not pack that small is halved.  Returns the members."""
    pairs = [(level, strategy) for level in LEVELS for _, strategy in STRATEGIES]
    members, at, k = [], 0, 0
    while at < len(stream):
        if at >= len(stream) // 2 and not any(member["size"] == 0 for member in members):
            members += [{"bytes": _bgzf_member(b"", 6, zlib.Z_DEFAULT_STRATEGY), "size": 0, "level": 6} for _ in range(3)]
        size, (level, strategy) = (1, 997, 0xff00, 65536)[k % 4], pairs[k % len(pairs)]
        member = _bgzf_member(stream[at:at + size], level, strategy)
        while member is None:
            size //= 2
            member = _bgzf_member(stream[at:at + size], level, strategy)
        members.append({"bytes": member, "size": min(size, len(stream) - at), "level": level})
        at += size
        k += 1
    members.append({"bytes": _bgzf_member(b"", 6, zlib.Z_DEFAULT_STRATEGY), "size": 0, "level": 6})  # (the end-of-file marker)
    return members


@pytest.mark.gpu
def test_a_file_of_every_kind_of_member_through_the_ingest(built, dataset_files, tmp_path, monkeypatch):
    """the product path (DevicePipeline: the feeder's tables, agpu_ingest_push_bgzf in pieces of 1 MB) over a file that begins with stored members, goes on with members of every
    level and strategy and of 1 byte to 64 KB, and has empty members in the middle: the batch of the host ingest of the original file.  One bit of a DEFLATE stream flipped so
    that zlib refuses it, or a changed CRC-32: the ingest fails; the latter is taken with ARRIBA_VERIFY_CRC=0"""
    import test_gpu_parity
    import test_host_and_device_logic as cpu_tier
    from arriba_amd.pipeline import ArribaError, DevicePipeline, HostSession
    monkeypatch.delenv("ARRIBA_VERIFY_CRC", raising=False)
    prefix = dataset_files("toy3k")
    host, expected, session, pipeline, columns = test_gpu_parity._batch_columns_of_both(prefix, piece_bytes=1 << 20)
    assert [key for key in expected if expected[key] != columns[key]] == []
    stream = gzip.open(prefix + ".bam", "rb").read()
    members = _mixed_file(stream)
    assert len(members) >= 44 and sum(member["size"] for member in members) == len(stream) and sum(1 for member in members if member["size"] == 0) == 4
    assert members[0]["level"] == 0 and set(member["level"] for member in members) == set(LEVELS)

    def ingest(name, changed=None):
        with open(str(tmp_path / name), "wb") as out:
            for k, member in enumerate(members):
                out.write(changed[1] if changed is not None and changed[0] == k else member["bytes"])
        other = HostSession(prefix + ".fa", prefix + ".gtf")
        return cpu_tier._device_batch_columns(other, DevicePipeline(other, bam=str(tmp_path / name), piece_bytes=1 << 20))
    rows = ingest("mixed.bam")
    assert [key for key in expected if expected[key] != rows[key]] == []
    # a deflated member of 64 KB in the second half of the file
    victim = max(k for k, member in enumerate(members) if member["level"] == 6 and member["size"] >= 0xff00)
    member = members[victim]["bytes"]
    rng = random.Random(3)
    while True:
        at, bit = rng.randrange(18, len(member) - 8), rng.randrange(8)
        damaged = member[:at] + bytes([member[at] ^ 1 << bit]) + member[at + 1:]
        if _zlib_inflate(damaged[18:-8]) is None:
            break
    with pytest.raises(ArribaError, match="failed to load alignments"):
        ingest("damaged.bam", (victim, damaged))
    other_crc = member[:-8] + struct.pack("<I", struct.unpack("<I", member[-8:-4])[0] ^ 0x10) + member[-4:]
    with pytest.raises(ArribaError, match="failed to load alignments"):
        ingest("crc.bam", (victim, other_crc))
    monkeypatch.setenv("ARRIBA_VERIFY_CRC", "0")
    rows = ingest("crc.bam", (victim, other_crc))
    assert [key for key in expected if expected[key] != rows[key]] == []
