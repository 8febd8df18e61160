// markdup_core.hpp -- --mark-duplicates: which templates of the -x input are duplicates (DESIGN.md 4.14 has the rule in full: Picard's for one library, without optical
// duplicates and UMIs).  What decides the bit 0x400 of a record of the sorted file is here and is shared by the kernels of agpu_markdup.hip and the host stepping of
// arriba_amd/csrc/host/markdup.cpp:
//   mdup_primary / mdup_slot / mdup_mapped   which records may be an end of their template, and of which slot
//   mdup_name_insert   read names -> template ids: the open-addressing table of supporting_core.hpp (hash tag << 32 | record + 1, 64-bit compare-and-swap, a hit confirmed by
//                      the bytes), over the QNAMEs of the records of the stream themselves: the id of a template is the record that got its name into the table first
//   mdup_end           the end of a slot: its key (refID, the unclipped 5' coordinate u, strand) in one 64-bit word, and its score (the base qualities >= 15, summed)
//   mdup_tie           the order inside a group: score descending, then file rank ascending, as one ascending 64-bit word
// Records are as sbam_parse reads them; byte 19 of a record is the high byte of its flag, 0x04 in it is BAM_FDUP.
#ifndef AGPU_MARKDUP_CORE_HPP
#define AGPU_MARKDUP_CORE_HPP 1

#include "supporting_core.hpp"

namespace agpu {

const uint32_t MDUP_NONE = 0xFFFFFFFFu;               // no record: an empty slot, a record without a name
const uint64_t MDUP_NO_END = ~0ull;                   // the key of a slot whose end is missing or unmapped (no mapped end has it: it would lie on reference 2^31 - 1, and a header holds fewer)
const uint32_t MDUP_MIN_QUALITY = 15;
const uint32_t MDUP_FLAG_BYTE = 19, MDUP_FLAG_MASK = 0x04; // byte of a record (counted from its block_size word) and bit in it that carry 0x400

AGPU_HD bool mdup_primary(uint32_t flag) { return (flag & 0x900u) == 0; }
AGPU_HD uint32_t mdup_slot(uint32_t flag) { return (flag & 1u) && (flag & 0x80u) ? 1u : 0u; }
AGPU_HD bool mdup_mapped(uint32_t flag, int32_t ref) { return !(flag & 4u) && ref >= 0; }

// (refID, u, strand), ascending as one word: refID in 31 bits, u + 2^31 in 32 (u is held to the range of a signed 32-bit number), the strand bit
AGPU_HD uint64_t mdup_end_key(int32_t ref, int64_t u, uint32_t reverse) {
	if (u < -2147483648ll) u = -2147483648ll;
	if (u > 2147483647ll) u = 2147483647ll;
	return (uint64_t) (uint32_t) ref << 33 | (uint64_t) (uint32_t) (u + 2147483648ll) << 1 | (reverse & 1u);
}
AGPU_HD uint64_t mdup_tie(uint32_t score, uint32_t rank) { return (uint64_t) ~score << 32 | rank; }

// the QNAME of record r of the stream (offset[r]: where its block_size word lies); false: the record is too short to hold one
AGPU_HD bool mdup_name_of(const uint8_t* stream, uint64_t stream_size, const uint64_t* offset, uint32_t r, const uint8_t*& name, uint32_t& length) {
	const uint64_t at = offset[r];
	if (at + 36 > stream_size) return false;
	uint64_t size = (uint64_t) sbam_load32(stream, at) + 4;
	if (size > stream_size - at) size = stream_size - at;
	return support_qname(stream, at, (uint32_t) size, name, length);
}

// Record r goes into the table; returns the id of its template: r, or the record with the same QNAME that got there first (whichever of them that is: ids only join records).
// The table has support_table_slots(records) slots, so it is never more than half full and a probe run ends.
AGPU_HD uint32_t mdup_name_insert(unsigned long long* table, uint64_t slots, const uint8_t* stream, uint64_t stream_size, const uint64_t* offset, uint32_t r, uint32_t hash_bits) {
	const uint8_t* mine; uint32_t length;
	if (!mdup_name_of(stream, stream_size, offset, r, mine, length)) return MDUP_NONE;
	const uint64_t h = support_hash(mine, length, hash_bits);
	const unsigned long long entry = (h >> 32) << 32 | (unsigned long long) (r + 1u);
	for (uint64_t slot = h & (slots - 1); ; slot = (slot + 1) & (slots - 1)) {
#if defined(__HIP_DEVICE_COMPILE__)
		const unsigned long long there = atomicCAS(&table[slot], 0ull, entry);
#else
		const unsigned long long there = table[slot];
		if (there == 0) table[slot] = entry;
#endif
		if (there == 0) return r;
		if (there >> 32 != entry >> 32) continue;
		const uint32_t other = (uint32_t) there - 1u;
		const uint8_t* theirs; uint32_t their_length;
		if (mdup_name_of(stream, stream_size, offset, other, theirs, their_length) && their_length == length && support_same_bytes(mine, theirs, length)) return other;
	}
}

struct MdupEnd { uint64_t key; uint32_t score; };

// the end that the record at stream[at] is: MDUP_NO_END and score 0 if it is not mapped.  Nothing outside the record is read.
AGPU_HD MdupEnd mdup_end(const uint8_t* stream, uint64_t at, uint64_t stream_size) {
	MdupEnd e; e.key = MDUP_NO_END; e.score = 0;
	if (at + 36 > stream_size) return e;
	uint64_t size = (uint64_t) sbam_load32(stream, at) + 4;
	if (size > stream_size - at) size = stream_size - at;
	const int32_t ref = (int32_t) sbam_load32(stream, at + 4), pos = (int32_t) sbam_load32(stream, at + 8);
	const uint32_t l_read_name = stream[at + 12], flag = sbam_load16(stream, at + 18);
	if (!mdup_mapped(flag, ref)) return e;
	uint32_t n_cigar = sbam_load16(stream, at + 16);
	if (36ull + l_read_name + 4ull * n_cigar > size) n_cigar = 0;
	const uint64_t cigar = at + 36 + l_read_name;
	// the clips in front (S, H: 4, 5), the reference length, the clips behind
	int64_t leading = 0, trailing = 0, length = 0;
	bool in_front = true;
	for (uint32_t k = 0; k < n_cigar; ++k) {
		const uint32_t word = sbam_load32(stream, cigar + 4ull * k), op = word & 15u;
		const bool clip = op == 4 || op == 5;
		if (clip) { if (in_front) leading += word >> 4; trailing += word >> 4; }
		else { in_front = false; trailing = 0; if ((0x18Du >> op) & 1u) length += word >> 4; }
	}
	if (n_cigar == 0) length = 1;
	const uint32_t reverse = (flag >> 4) & 1u;
	e.key = mdup_end_key(ref, reverse ? (int64_t) pos + length - 1 + trailing : (int64_t) pos - leading, reverse);
	// the qualities: l_seq bytes behind the packed bases, as far as they lie inside the record
	const uint64_t l_seq = sbam_load32(stream, at + 20);
	const uint64_t qualities = 36ull + l_read_name + 4ull * n_cigar + (l_seq + 1) / 2;
	if (qualities >= size) return e;
	const uint64_t count = l_seq < size - qualities ? l_seq : size - qualities;
	if (count == 0 || stream[at + qualities] == 0xFFu) return e;
	uint32_t score = 0;
	for (uint64_t k = 0; k < count; ++k) { const uint32_t q = stream[at + qualities + k]; if (q >= MDUP_MIN_QUALITY) score += q; }
	e.score = score;
	return e;
}

}

#endif
