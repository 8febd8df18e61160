// supporting_core.hpp -- --supporting-alignments: one small sorted, indexed BAM file per row of fusions.tsv with the alignments of the row's read_identifiers that lie near
// its breakpoints (what scripts/extract_fusion-supporting_alignments.sh of the reference gets from samtools view / sort / index).  What decides which record goes into which
// file is here and is shared by the kernels of agpu_supporting.hip and the host stepping of arriba_amd/csrc/host/supporting.cpp:
//   support_hash, support_insert, support_lookup   read names -> name ids: an open-addressing table of 64-bit slots (hash tag << 32 | name + 1), a hit confirmed by the bytes
//   support_listed_length                          a name of the batch is "QNAME,HI[ITD]": the listed name ends in front of its last ','
//   support_overlaps                               the window of the script around a breakpoint (SEARCH_WINDOW) against pos / end of sbam_parse
// The container of a file is that of --sorted-bam (sorted_bam_core.hpp).
#ifndef AGPU_SUPPORTING_CORE_HPP
#define AGPU_SUPPORTING_CORE_HPP 1

#include "sorted_bam_core.hpp"

namespace agpu {

const uint32_t SUPPORT_NONE = 0xFFFFFFFFu;             // a record (or a listed name) that belongs to no name of the table
const int64_t SUPPORT_DEFAULT_WINDOW = 1000000;        // SEARCH_WINDOW of the script
const uint64_t SUPPORT_MAX_NAMES = 0x7FFFFFF0ull;

// FNV-1a over the bytes, finalised (murmur3 fmix64); `bits` < 64 (ARRIBA_SUPPORT_HASH_BITS, a test knob) keeps the low bits only: collisions and long probe runs on purpose
AGPU_HD uint64_t support_hash(const uint8_t* name, uint32_t length, uint32_t bits) {
	uint64_t h = 0xCBF29CE484222325ull;
	for (uint32_t k = 0; k < length; ++k) { h ^= name[k]; h *= 0x100000001B3ull; }
	h ^= h >> 33; h *= 0xFF51AFD7ED558CCDull; h ^= h >> 33; h *= 0xC4CEB9FE1A85EC53ull; h ^= h >> 33;
	return bits >= 64 ? h : h & ((1ull << bits) - 1);
}
AGPU_HD bool support_same_bytes(const uint8_t* a, const uint8_t* b, uint32_t length) { for (uint32_t k = 0; k < length; ++k) if (a[k] != b[k]) return false; return true; }
// slots of a table for n names: a power of two, at most half full
AGPU_HD uint64_t support_table_slots(uint64_t n_names) { uint64_t slots = 16; while (slots < 2 * n_names) slots *= 2; return slots; }

// names[name_offset[i] .. name_offset[i + 1]): the listed name of entry i is all of it, or (strip_hit_index) what lies in front of its last ','
AGPU_HD uint32_t support_listed_length(const uint8_t* names, uint64_t begin, uint64_t end, bool strip_hit_index) {
	if (strip_hit_index) for (uint64_t k = end; k > begin; --k) if (names[k - 1] == ',') return (uint32_t) (k - 1 - begin);
	return (uint32_t) (end - begin);
}

struct SupportNames { const uint8_t* bytes; const uint64_t* offset; uint64_t n; bool strip_hit_index; };
AGPU_HD uint32_t support_name_of(const SupportNames& names, uint64_t i, const uint8_t*& bytes) { bytes = names.bytes + names.offset[i]; return support_listed_length(names.bytes, names.offset[i], names.offset[i + 1], names.strip_hit_index); }

// Entry i of the names goes into the table; returns its name id: i, or the entry with the same bytes that got there first (whichever of them that is: ids only join records
// to rows).  The table is never more than half full, so a probe run ends.  On the device the slot is taken with a 64-bit compare-and-swap.
AGPU_HD uint32_t support_insert(unsigned long long* table, uint64_t slots, const SupportNames& names, uint32_t i, uint32_t hash_bits) {
	const uint8_t* mine; const uint32_t length = support_name_of(names, i, mine);
	const uint64_t h = support_hash(mine, length, hash_bits);
	const unsigned long long entry = (h >> 32) << 32 | (unsigned long long) (i + 1u);
	for (uint64_t slot = h & (slots - 1); ; slot = (slot + 1) & (slots - 1)) {
#if defined(__HIP_DEVICE_COMPILE__)
		unsigned long long there = atomicCAS(&table[slot], 0ull, entry);
#else
		unsigned long long there = table[slot];
		if (there == 0) table[slot] = entry;
#endif
		if (there == 0) return i;
		if (there >> 32 != entry >> 32) continue;
		const uint32_t other = (uint32_t) there - 1u;
		const uint8_t* theirs; const uint32_t their_length = support_name_of(names, other, theirs);
		if (their_length == length && support_same_bytes(mine, theirs, length)) return other;
	}
}
// the name id of name[0 .. length), SUPPORT_NONE if the table does not hold it
AGPU_HD uint32_t support_lookup(const unsigned long long* table, uint64_t slots, const SupportNames& names, const uint8_t* name, uint32_t length, uint32_t hash_bits) {
	const uint64_t h = support_hash(name, length, hash_bits);
	for (uint64_t slot = h & (slots - 1); ; slot = (slot + 1) & (slots - 1)) {
		const unsigned long long there = table[slot];
		if (there == 0) return SUPPORT_NONE;
		if (there >> 32 != h >> 32) continue;
		const uint32_t other = (uint32_t) there - 1u;
		const uint8_t* theirs; const uint32_t their_length = support_name_of(names, other, theirs);
		if (their_length == length && support_same_bytes(name, theirs, length)) return other;
	}
}

// the QNAME of the record at stream[at] whose size (sbam_parse) is `size`: false if the record is too short to hold it
AGPU_HD bool support_qname(const uint8_t* stream, uint64_t at, uint32_t size, const uint8_t*& name, uint32_t& length) {
	if (size < 36) return false;
	const uint32_t l_read_name = stream[at + 12];
	if (36u + l_read_name > size) return false;
	name = stream + at + 36; length = l_read_name > 0 ? l_read_name - 1 : 0; // (l_read_name counts the NUL)
	return true;
}

// The script asks samtools for CONTIG:max(P,W)-W .. max(P,W)+W (1-based, closed) around the printed position P = breakpoint + 1.  A record with 0-based pos and exclusive end
// overlaps that region when pos < P' + W and end > max(P' - W - 1, 0).  Records without a reference, and breakpoints on a contig the BAM header does not have (ref < 0), never match.
AGPU_HD bool support_overlaps(int32_t record_ref, int32_t pos, int32_t end, int32_t window_ref, int32_t breakpoint, int64_t window) {
	if (record_ref < 0 || record_ref != window_ref) return false;
	const int64_t printed = (int64_t) breakpoint + 1, centre = printed > window ? printed : window;
	const int64_t low = centre - window - 1;
	return (int64_t) pos < centre + window && (int64_t) end > (low > 0 ? low : 0);
}

// 64-bit keys of the two sorts of the join: (name id, row) groups the rows by name; (row, pool rank) is the order of the files
AGPU_HD uint64_t support_pair_key(uint32_t name_id, uint32_t row) { return (uint64_t) name_id << 32 | row; }

}

#endif
