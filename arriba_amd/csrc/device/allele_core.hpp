// allele_core.hpp -- --allele-counts: the bases the records of -x show at a list of known positions (DESIGN.md 4.17 has the rule in full).  What decides a number of the file is here
// and is shared by the kernels of agpu_alleles.hip and the host stepping of arriba_amd/csrc/host/allele_counts.cpp:
//   allele_record        whether a record counts (mpileup's flag filter, a reference of the header, MAPQ, a CIGAR, SEQ and QUAL that lie inside the record, a CIGAR whose read length
//                        is l_seq) and where its CIGAR, SEQ and QUAL lie: depth_parse and the per-base fields behind it
//   allele_nibble / allele_quality / allele_column   base i of the 4-bit SEQ packing, quality byte i, and the column a base under M, = or X adds to
//   allele_key           a site as one ascending 64-bit word, (reference << 32) | 0-based position; allele_lower_bound searches the sorted keys
//   allele_window / allele_windows_hold   one bit per 64-base window of the concatenated references that holds a site: the rejection test of an aligned block
//   AlleleWalk / allele_walk_next   the walk of a CIGAR from POS and read index 0 as a resumable iterator: every call gives the next (site slot, column) the record adds one to,
//                        in the order of the sorted keys, or false at the end of the CIGAR.  It is an iterator, not a visitor, because the lanes of a wavefront merge their adds
//                        between two steps (agpu_alleles.hip), which needs all of them at the same place
//   allele_ref_base      the upper-case base of the assembly under a site
// Records are as sbam_parse reads them.  Nothing outside a record is read: the read index of every base lies below l_seq, which is what the check of the CIGAR is for.
#ifndef AGPU_ALLELE_CORE_HPP
#define AGPU_ALLELE_CORE_HPP 1

#include "depth_core.hpp"

namespace agpu {

enum { ALLELE_A = 0, ALLELE_C = 1, ALLELE_G = 2, ALLELE_T = 3, ALLELE_N = 4, ALLELE_DEL = 5, ALLELE_SKIP = 6, ALLELE_LOWQ = 7, ALLELE_COLUMNS = 8 };
const uint32_t ALLELE_UNPLACED = 0xFFFFFFFFu;                    // agpu_allele_site.ref of a site without a reference
const uint32_t ALLELE_EXCLUDED_FLAGS = 0x4u | 0x100u | 0x200u | 0x400u; // unmapped, secondary, QC fail, duplicate: mpileup's default
const uint32_t ALLELE_WINDOW_SHIFT = 6;                          // 64 bases per bit of the window bitmap
const uint64_t ALLELE_MAX_SITES = (1ull << 29) - 1;              // (slot << 3 | column) is one 32-bit word
const uint64_t ALLELE_PROBE_WINDOWS = 2048;                      // a block over more windows (an N of 128 kb) is searched without the probe

struct AlleleRecord { uint32_t ref; int32_t pos; uint32_t n_cigar, l_seq; uint64_t cigar_at, seq_at, qual_at; };

// The record whose block_size word is at stream[at]: false if it contributes nothing.
AGPU_HD bool allele_record(const uint8_t* stream, uint64_t at, uint64_t stream_size, uint32_t n_ref, uint32_t min_mapq, AlleleRecord& out) {
	const DepthRecord head = depth_parse(stream, at, stream_size, n_ref); // (36 bytes of head, flag 0x4, the reference, a CIGAR that is not empty and lies inside the record)
	if (!head.counts) return false;
	const uint32_t flag = sbam_load16(stream, at + 18), mapq = stream[at + 13], l_read_name = stream[at + 12];
	if ((flag & ALLELE_EXCLUDED_FLAGS) != 0 || mapq < min_mapq) return false;
	const uint64_t l_seq = sbam_load32(stream, at + 20);
	if (l_seq == 0) return false;
	uint64_t size = (uint64_t) sbam_load32(stream, at) + 4;
	if (size > stream_size - at) size = stream_size - at;
	const uint64_t seq = 36ull + l_read_name + 4ull * head.n_cigar;
	if (seq + (l_seq + 1) / 2 + l_seq > size) return false; // (a negative l_seq is a large one here)
	uint64_t read_bases = 0;
	for (uint32_t k = 0; k < head.n_cigar; ++k) {
		const uint32_t word = sbam_load32(stream, head.cigar_at + 4ull * k);
		if ((0x193u >> (word & 15u)) & 1u) read_bases += word >> 4; // M (0), I (1), S (4), = (7), X (8)
	}
	if (read_bases != l_seq) return false;
	out.ref = (uint32_t) head.ref; out.pos = head.pos; out.n_cigar = head.n_cigar; out.l_seq = (uint32_t) l_seq;
	out.cigar_at = head.cigar_at; out.seq_at = at + seq; out.qual_at = at + seq + (l_seq + 1) / 2;
	return true;
}

// base i: the high nibble of SEQ byte i / 2 when i is even, the low nibble when it is odd
AGPU_HD uint32_t allele_nibble(const uint8_t* stream, uint64_t seq_at, uint64_t i) { return (stream[seq_at + (i >> 1)] >> ((i & 1u) ? 0 : 4)) & 15u; }
AGPU_HD uint32_t allele_quality(const uint8_t* stream, uint64_t qual_at, uint64_t i) { return stream[qual_at + i]; } // (an unsigned byte: 0xFF, no quality, passes every threshold)
AGPU_HD uint32_t allele_column_of(uint32_t nibble) { return nibble == 1 ? ALLELE_A : nibble == 2 ? ALLELE_C : nibble == 4 ? ALLELE_G : nibble == 8 ? ALLELE_T : ALLELE_N; }
AGPU_HD uint32_t allele_column(const uint8_t* stream, const AlleleRecord& record, uint64_t i, uint32_t min_baseq) {
	if (allele_quality(stream, record.qual_at, i) < min_baseq) return ALLELE_LOWQ;
	return allele_column_of(allele_nibble(stream, record.seq_at, i));
}

AGPU_HD uint64_t allele_key(uint32_t ref, uint32_t pos) { return (uint64_t) ref << 32 | pos; }
// the first of n ascending keys that is not below `key`
AGPU_HD uint64_t allele_lower_bound(const uint64_t* keys, uint64_t n, uint64_t key) {
	uint64_t begin = 0, end = n;
	while (begin < end) { const uint64_t middle = begin + (end - begin) / 2; if (keys[middle] < key) begin = middle + 1; else end = middle; }
	return begin;
}

// keys: the placed sites, ascending (equal keys -- duplicate lines -- are neighbours); window_offset[t]: the first window of reference t, (LN + 63) / 64 windows each; bitmap: 32
// windows per word, null = no rejection test
struct AlleleSites { const uint64_t* keys; uint64_t n; const uint32_t* bitmap; const uint64_t* window_offset; };
AGPU_HD uint64_t allele_windows_of(uint32_t length) { return ((uint64_t) length + (1u << ALLELE_WINDOW_SHIFT) - 1) >> ALLELE_WINDOW_SHIFT; }
AGPU_HD uint64_t allele_window(const uint64_t* window_offset, uint32_t ref, uint32_t pos) { return window_offset[ref] + (pos >> ALLELE_WINDOW_SHIFT); }
// whether a window that [lo, hi) of reference ref touches holds a site; 0 <= lo < hi <= LN
AGPU_HD bool allele_windows_hold(const AlleleSites& sites, uint32_t ref, uint32_t lo, uint32_t hi) {
	if (sites.bitmap == nullptr) return true;
	const uint64_t first = allele_window(sites.window_offset, ref, lo), last = allele_window(sites.window_offset, ref, hi - 1);
	if (last - first >= ALLELE_PROBE_WINDOWS) return true;
	for (uint64_t word = first >> 5; word <= last >> 5; ++word) {
		uint32_t mask = 0xFFFFFFFFu;
		if (word == first >> 5) mask &= 0xFFFFFFFFu << (first & 31u);
		if (word == last >> 5) mask &= 0xFFFFFFFFu >> (31u - (uint32_t) (last & 31u));
		if (sites.bitmap[word] & mask) return true;
	}
	return false;
}

// The walk of a record over a reference of `length` bases.  Between two calls of allele_walk_next a block may be open: an operation that spans reference positions (M, =, X: kind 1;
// D: 2; N: 3), cut to [0, length), with `cursor` at the next sorted site inside it.
struct AlleleWalk {
	AlleleRecord record; uint32_t length;
	uint32_t k;            // the next CIGAR operation
	int64_t at;            // the reference position at its start
	uint64_t read_index;   // the read index at its start
	uint32_t kind;         // of the open block; 0: none
	uint64_t cursor, end_key; int64_t block_at; uint64_t block_read;
};
AGPU_HD void allele_walk_begin(AlleleWalk& walk, const AlleleRecord& record, uint32_t length) {
	walk.record = record; walk.length = length; walk.k = 0; walk.at = record.pos; walk.read_index = 0; walk.kind = 0; walk.cursor = 0; walk.end_key = 0; walk.block_at = 0; walk.block_read = 0;
}
// the next (slot, column) the record adds one to: slot is an index into sites.keys.  A CIGAR only moves forward on the reference, so no slot comes twice.
AGPU_HD bool allele_walk_next(AlleleWalk& walk, const uint8_t* stream, const AlleleSites& sites, uint32_t min_baseq, uint32_t& slot, uint32_t& column) {
	for (;;) {
		if (walk.kind != 0) {
			if (walk.cursor < sites.n) {
				const uint64_t key = sites.keys[walk.cursor];
				if (key < walk.end_key) {
					slot = (uint32_t) walk.cursor++;
					if (walk.kind == 1) column = allele_column(stream, walk.record, walk.block_read + (uint64_t) ((int64_t) (uint32_t) key - walk.block_at), min_baseq);
					else column = walk.kind == 2 ? ALLELE_DEL : ALLELE_SKIP;
					return true;
				}
			}
			walk.kind = 0;
		}
		if (walk.k >= walk.record.n_cigar) return false;
		const uint32_t word = sbam_load32(stream, walk.record.cigar_at + 4ull * walk.k), op = word & 15u;
		const int64_t span = word >> 4;
		++walk.k;
		if ((0x18Du >> op) & 1u) { // M (0), D (2), N (3), = (7), X (8): the operations that span reference positions
			const int64_t lo = walk.at < 0 ? 0 : walk.at, hi = walk.at + span < (int64_t) walk.length ? walk.at + span : (int64_t) walk.length;
			const bool bases = op != 2 && op != 3;
			if (lo < hi && allele_windows_hold(sites, walk.record.ref, (uint32_t) lo, (uint32_t) hi)) {
				walk.cursor = allele_lower_bound(sites.keys, sites.n, allele_key(walk.record.ref, (uint32_t) lo));
				walk.end_key = allele_key(walk.record.ref, 0) + (uint64_t) hi; // (hi <= LN < 2^32: no carry into the next reference that a site could sit on)
				walk.block_at = walk.at; walk.block_read = walk.read_index;
				walk.kind = bases ? 1u : op == 2 ? 2u : 3u;
			}
			walk.at += span;
			if (bases) walk.read_index += (uint64_t) span;
		} else if (op == 1 || op == 4) walk.read_index += (uint64_t) span; // I, S: the read index only; H, P and the unassigned codes: nothing
	}
}

// contig: of the session (any value if the session has none for the reference); 'N' where the session holds no sequence there
AGPU_HD uint8_t allele_ref_base(const GenomeView& genome, uint32_t contig, uint32_t pos) {
	if (contig >= genome.n_contigs) return (uint8_t) 'N';
	const uint64_t begin = genome.contig_offset[contig], bases = genome.contig_offset[contig + 1] - begin;
	if ((uint64_t) pos >= bases) return (uint8_t) 'N';
	const uint8_t base = (uint8_t) genome.bases[begin + pos];
	return base >= (uint8_t) 'a' && base <= (uint8_t) 'z' ? (uint8_t) (base - 32) : base;
}

}

#endif
