// sorted_bam_core.hpp -- the records of -x in coordinate order as a BAM file of stored BGZF blocks, with its BAI index (SAMv1 sections 4.1, 4.2, 5.2): what the
// reference's workflow script gets from `samtools sort` + `samtools index` behind the call of arriba (run_arriba.sh:47-51).  Everything that decides a byte of the two files
// is here and is shared by the kernels of agpu_sorted_bam.hip and the host stepping of arriba_amd/csrc/host/sorted_bam.cpp:
//   sbam_parse        the sort key of a record (refID as unsigned, pos + 1, the reverse-strand flag), its size, and its end coordinate from the CIGAR of the record
//   sbam_voffset      the virtual offset of a byte of the sorted uncompressed stream: blocks of exactly SBAM_PAYLOAD bytes, so block positions are arithmetic (stored
//                     blocks) or come from a table of block file offsets (compressed blocks: deflate_out_core.hpp)
//   sbam_head_byte / sbam_tail_byte   the 23 bytes in front of the payload of a stored block and the 8 behind it
//   sbam_reg2bin, sbam_indexed, sbam_window_range   the bin and the 16 kb windows of a record
// Records are moved byte for byte; the `bin` field of a record is never read (generators write constants there).
#ifndef AGPU_SORTED_BAM_CORE_HPP
#define AGPU_SORTED_BAM_CORE_HPP 1

#include "views.hpp"

namespace agpu {

const uint32_t SBAM_PAYLOAD = 0xff00;                  // payload bytes of every record block but the last
const uint32_t SBAM_HEAD = 23, SBAM_TAIL = 8;          // gzip header with the BC subfield (18) + stored-deflate header (5); CRC-32 + ISIZE
const uint32_t SBAM_BLOCK = SBAM_PAYLOAD + SBAM_HEAD + SBAM_TAIL;
const uint32_t SBAM_EOF_BYTES = 28;
const uint32_t SBAM_LINEAR_SHIFT = 14;                 // 16 kb windows of the linear index
const int32_t SBAM_MAX_REFERENCE = 1 << 29;            // what the bins of a BAI index can address
const uint32_t SBAM_PSEUDO_BIN = 37450;
const uint64_t SBAM_NO_OFFSET = ~0ull;

// 32 / 16 bits, little endian, at any alignment.  On the device: aligned words and shifts (a word is only touched if one of the wanted bytes lies in it).
AGPU_HD uint32_t sbam_load32(const uint8_t* bytes, uint64_t at) {
#if defined(__HIP_DEVICE_COMPILE__)
	const uint64_t address = (uint64_t) (bytes + at);
	const uint32_t* word = (const uint32_t*) (address & ~3ull);
	const uint32_t shift = (uint32_t) (address & 3u) * 8;
	const uint32_t low = word[0];
	if (shift == 0) return low;
	return (low >> shift) | (word[1] << (32 - shift));
#else
	uint32_t v; __builtin_memcpy(&v, bytes + at, 4); return v;
#endif
}
AGPU_HD uint32_t sbam_load16(const uint8_t* bytes, uint64_t at) { return (uint32_t) bytes[at] | (uint32_t) bytes[at + 1] << 8; }

struct SbamRecord {
	uint64_t key;      // ascending: refID as unsigned (-1 last), pos + 1, reverse strand
	uint32_t size;     // block_size + 4
	int32_t ref, pos, end; // end: pos + reference length of the CIGAR; pos + 1 if that is 0 or the record is unmapped
	uint32_t flag;
};

AGPU_HD uint64_t sbam_key(int32_t ref, int32_t pos, uint32_t flag) {
	// pos is -1 .. 2^31 - 2 (SAMv1 4.2), so pos + 1 has 31 bits
	return (uint64_t) (uint32_t) ref << 32 | (uint64_t) (((uint32_t) pos + 1u) & 0x7FFFFFFFu) << 1 | ((flag >> 4) & 1u);
}

// the record whose block_size word is at stream[at]; nothing outside stream[0 .. stream_size) is read (the device rounds the ends of its reads to whole words that hold a byte of the record)
AGPU_HD SbamRecord sbam_parse(const uint8_t* stream, uint64_t at, uint64_t stream_size) {
	SbamRecord r;
	if (at + 36 > stream_size) { r.ref = -1; r.pos = -1; r.end = 0; r.flag = 4; r.size = (uint32_t) (stream_size - at); r.key = sbam_key(-1, -1, 4); return r; }
	uint64_t size = (uint64_t) sbam_load32(stream, at) + 4;
	if (size > stream_size - at) size = stream_size - at;
	r.size = (uint32_t) size;
	r.ref = (int32_t) sbam_load32(stream, at + 4); r.pos = (int32_t) sbam_load32(stream, at + 8);
	const uint32_t l_read_name = stream[at + 12];
	uint32_t n_cigar = sbam_load16(stream, at + 16);
	r.flag = sbam_load16(stream, at + 18);
	r.key = sbam_key(r.ref, r.pos, r.flag);
	if (36ull + l_read_name + 4ull * n_cigar > size) n_cigar = 0;
	int64_t length = 0;
	if (!(r.flag & 4u)) {
		const uint64_t cigar = at + 36 + l_read_name;
		for (uint32_t k = 0; k < n_cigar; ++k) {
			const uint32_t op = sbam_load32(stream, cigar + 4ull * k);
			if ((0x18Du >> (op & 15u)) & 1u) length += op >> 4; // M, D, N, =, X
		}
	}
	int64_t end = (int64_t) r.pos + (length > 0 ? length : 1);
	if (end > SBAM_MAX_REFERENCE) end = SBAM_MAX_REFERENCE;
	r.end = (int32_t) end;
	return r;
}

// a record goes into the bins and the linear index if it has a coordinate the index can address
AGPU_HD bool sbam_indexed(int32_t ref, int32_t pos, uint32_t n_ref) { return ref >= 0 && (uint32_t) ref < n_ref && pos >= 0 && pos < SBAM_MAX_REFERENCE; }
AGPU_HD uint32_t sbam_reg2bin(int32_t begin, int32_t end) { // SAMv1 5.3
	--end;
	if (begin >> 14 == end >> 14) return ((1u << 15) - 1) / 7 + (begin >> 14);
	if (begin >> 17 == end >> 17) return ((1u << 12) - 1) / 7 + (begin >> 17);
	if (begin >> 20 == end >> 20) return ((1u << 9) - 1) / 7 + (begin >> 20);
	if (begin >> 23 == end >> 23) return ((1u << 6) - 1) / 7 + (begin >> 23);
	if (begin >> 26 == end >> 26) return ((1u << 3) - 1) / 7 + (begin >> 26);
	return 0;
}
AGPU_HD uint64_t sbam_windows_of(uint32_t reference_length) { return ((uint64_t) reference_length + (1u << SBAM_LINEAR_SHIFT) - 1) >> SBAM_LINEAR_SHIFT; }
// the windows [first, last] of its reference a record overlaps, cut to the windows the reference has; false: none
AGPU_HD bool sbam_window_range(int32_t pos, int32_t end, uint64_t windows, uint64_t& first, uint64_t& last) {
	if (windows == 0) return false;
	first = (uint64_t) pos >> SBAM_LINEAR_SHIFT; last = (uint64_t) (end - 1) >> SBAM_LINEAR_SHIFT;
	if (first >= windows) first = windows - 1;
	if (last >= windows) last = windows - 1;
	return true;
}

AGPU_HD uint64_t sbam_block_count(uint64_t uncompressed) { return (uncompressed + SBAM_PAYLOAD - 1) / SBAM_PAYLOAD; }
AGPU_HD uint64_t sbam_voffset(uint64_t first_block_file_offset, uint64_t uncompressed_offset) {
	return (first_block_file_offset + uncompressed_offset / SBAM_PAYLOAD * SBAM_BLOCK) << 16 | uncompressed_offset % SBAM_PAYLOAD;
}

// ... of a file whose blocks have sizes of their own (--sorted-bam-compression): block_file_offset[b] is where block b begins in the file, one entry more for the end
AGPU_HD uint64_t sbam_voffset(const uint64_t* block_file_offset, uint64_t uncompressed_offset) {
	return block_file_offset[uncompressed_offset / SBAM_PAYLOAD] << 16 | uncompressed_offset % SBAM_PAYLOAD;
}

// byte i < SBAM_HEAD in front of a payload of n bytes
AGPU_HD uint8_t sbam_head_byte(uint32_t i, uint32_t n) {
	const uint32_t bsize = n + SBAM_HEAD + SBAM_TAIL - 1;
	switch (i) {
		case 0: return 0x1f; case 1: return 0x8b; case 2: return 8; case 3: return 4; case 9: return 0xff; case 10: return 6; case 12: return 'B'; case 13: return 'C'; case 14: return 2;
		case 16: return (uint8_t) bsize; case 17: return (uint8_t) (bsize >> 8);
		case 18: return 1; case 19: return (uint8_t) n; case 20: return (uint8_t) (n >> 8); case 21: return (uint8_t) ~n; case 22: return (uint8_t) (~n >> 8);
		default: return 0;
	}
}
// byte i < SBAM_TAIL behind it
AGPU_HD uint8_t sbam_tail_byte(uint32_t i, uint32_t crc, uint32_t n) { return (uint8_t) ((i < 4 ? crc : n) >> (8 * (i & 3u))); }
// byte i < SBAM_EOF_BYTES of the end-of-file block (SAMv1 4.1.2): an empty block whose payload is the two bytes of an empty final deflate block
AGPU_HD uint8_t sbam_eof_byte(uint32_t i) { return i < 16 ? sbam_head_byte(i, 0) : i == 16 ? 0x1b : i == 18 ? 3 : 0; }

// the key a chunk of the index is grouped by
AGPU_HD uint64_t sbam_chunk_key(int32_t ref, uint32_t bin) { return (uint64_t) (uint32_t) ref << 32 | bin; }

}

#endif
