// indel_core.hpp -- --indel-sites: the short insertions and deletions the records of -x carry in their CIGARs, left-normalised against the assembly (DESIGN.md 4.22 has the rule in
// full).  What decides a number of the file is here and is shared by the kernels of agpu_indels.hip and the host stepping of arriba_amd/csrc/host/indel_sites.cpp:
//   indel_last_aligned   the last operation M, = or X of a CIGAR with a span: an I or D counts only between the first such operation and the last one
//   indel_pack           an insertion from the SEQ nibbles (allele_nibble; it may start at an even or an odd read index): 2 bits a base, false if a nibble is not A, C, G or T
//   indel_shift_deletion / indel_shift_insertion   the two normalisation loops: to the left while the assembly (allele_ref_base) allows it, INDEL_MAX_SHIFT steps at the most
//   indel_shape          the second word of an event: type, length, and the bases of an insertion; the first word is the allele_key of the anchor
//   indel_walk           the CIGAR of a counting record: tallies its indel operations and, if asked, normalises each event and hands it to a sink
//   indel_reported       the percent test of a (support, depth) pair
// Which records count and where their CIGAR and SEQ lie is allele_core.hpp's (allele_record with --indel-min-mapq); base qualities are not consulted.
#ifndef AGPU_INDEL_CORE_HPP
#define AGPU_INDEL_CORE_HPP 1

#include "allele_core.hpp"

namespace agpu {

const uint32_t INDEL_MAX_INSERTION = 28;        // bases of a keyable insertion: 56 bits of the shape word
const uint32_t INDEL_MAX_SHIFT = 4096;          // steps to the left of one event (ARRIBA_INDEL_MAX_SHIFT lowers it)
const uint64_t INDEL_MAX_EVENTS = 1ull << 31;   // of one call (ARRIBA_INDEL_MAX_EVENTS lowers it): 32 GB of events, twice
const uint64_t INDEL_INSERTION = 1ull << 63;    // of a shape word
const uint32_t INDEL_TEXT_DELETION = 64;        // the deleted bases are printed up to this length
enum { INDEL_DEL = 0, INDEL_INS = 1 };

// an event: two ascending words.  Equal events are neighbours behind a sort by (site, shape); the events of a site are neighbours; sites come in the order of the file
struct IndelEvent { uint64_t site, shape; };
AGPU_HD bool operator==(const IndelEvent& a, const IndelEvent& b) { return a.site == b.site && a.shape == b.shape; }
AGPU_HD bool operator!=(const IndelEvent& a, const IndelEvent& b) { return !(a == b); }
struct IndelEventLess { AGPU_HD bool operator()(const IndelEvent& a, const IndelEvent& b) const { return a.site < b.site || (a.site == b.site && a.shape < b.shape); } };

struct IndelTally { uint32_t operations, events, unkeyed, capped; }; // of one record: indel operations (rule 2), events among them, insertions without a key, events stopped at the cap

AGPU_HD bool indel_is_base(uint8_t base) { return base == 'A' || base == 'C' || base == 'G' || base == 'T'; }
AGPU_HD uint32_t indel_code(uint8_t base) { return base == 'A' ? 0u : base == 'C' ? 1u : base == 'G' ? 2u : 3u; }

// the index of the last operation M, = or X with a span of at least 1, n_cigar if there is none
AGPU_HD uint32_t indel_last_aligned(const uint8_t* stream, const AlleleRecord& record) {
	uint32_t last = record.n_cigar;
	for (uint32_t k = 0; k < record.n_cigar; ++k) {
		const uint32_t word = sbam_load32(stream, record.cigar_at + 4ull * k), op = word & 15u;
		if ((op == 0 || op == 7 || op == 8) && (word >> 4) != 0) last = k;
	}
	return last;
}

// the bases [read_index, read_index + length) of SEQ, length <= INDEL_MAX_INSERTION, as 2 bits each with the first base on top of 2 * length bits; false if one is not A, C, G or T
AGPU_HD bool indel_pack(const uint8_t* stream, const AlleleRecord& record, uint64_t read_index, uint32_t length, uint64_t& bases) {
	bases = 0;
	for (uint32_t j = 0; j < length; ++j) {
		const uint32_t column = allele_column_of(allele_nibble(stream, record.seq_at, read_index + j));
		if (column > ALLELE_T) return false;
		bases = bases << 2 | column;
	}
	return true;
}

// Deletion of [a + 1, a + length] of a reference (a + length < LN): to the left while the base that leaves on the right equals the one that enters on the left.  capped: another step
// was due when max_shift were done.
AGPU_HD uint32_t indel_shift_deletion(const GenomeView& genome, uint32_t contig, uint32_t a, uint32_t length, uint32_t max_shift, bool& capped) {
	capped = false;
	for (uint32_t steps = 0; a >= 1; ++steps) {
		const uint8_t base = allele_ref_base(genome, contig, a);
		if (!indel_is_base(base) || base != allele_ref_base(genome, contig, a + length)) break;
		if (steps == max_shift) { capped = true; break; }
		--a;
	}
	return a;
}
// Insertion of `bases` (indel_pack) behind a: to the left while the last inserted base equals the anchor; the bases rotate to the right by one with every step
AGPU_HD uint32_t indel_shift_insertion(const GenomeView& genome, uint32_t contig, uint32_t a, uint32_t length, uint32_t max_shift, uint64_t& bases, bool& capped) {
	capped = false;
	for (uint32_t steps = 0; a >= 1; ++steps) {
		const uint8_t base = allele_ref_base(genome, contig, a);
		if (!indel_is_base(base) || indel_code(base) != (uint32_t) (bases & 3u)) break;
		if (steps == max_shift) { capped = true; break; }
		bases = bases >> 2 | (bases & 3u) << (2 * (length - 1));
		--a;
	}
	return a;
}

// deletions before insertions, by length, insertions of one length by their bases (A < C < G < T, left-justified in 56 bits)
AGPU_HD uint64_t indel_shape_deletion(uint32_t length) { return length; } // (a CIGAR span: below 2^28)
AGPU_HD uint64_t indel_shape_insertion(uint32_t length, uint64_t bases) { return INDEL_INSERTION | (uint64_t) length << 56 | bases << (56 - 2 * length); } // 1 <= length <= 28
AGPU_HD uint32_t indel_shape_type(uint64_t shape) { return shape & INDEL_INSERTION ? INDEL_INS : INDEL_DEL; }
AGPU_HD uint32_t indel_shape_length(uint64_t shape) { return shape & INDEL_INSERTION ? (uint32_t) (shape >> 56) & 127u : (uint32_t) shape; }
AGPU_HD uint64_t indel_shape_bases(uint64_t shape) { return shape & INDEL_INSERTION ? shape & ((1ull << 56) - 1) : 0; } // base j of an insertion: bits 55 - 2 j and 54 - 2 j

// The CIGAR of a counting record over a reference of `length` bases that is `contig` of the session.  Adds to `tally`.  resolve false: operations, events and unkeyed only (the
// head, the CIGAR and the nibbles of the insertions are read).  resolve true: every event is normalised as well, `capped` is counted and sink(site, shape) gets it, in CIGAR order.
template <class Sink> AGPU_HD void indel_walk(const uint8_t* stream, const AlleleRecord& record, const GenomeView& genome, uint32_t contig, uint32_t length, uint32_t max_shift, bool resolve, IndelTally& tally, Sink& sink) {
	const uint32_t last = indel_last_aligned(stream, record);
	if (last == record.n_cigar) return;
	int64_t at = record.pos; uint64_t read_index = 0;
	bool aligned_before = false;
	for (uint32_t k = 0; k < last; ++k) { // (an operation behind the last aligned one is no indel operation)
		const uint32_t word = sbam_load32(stream, record.cigar_at + 4ull * k), op = word & 15u, span = word >> 4;
		if (op == 0 || op == 7 || op == 8) { if (span != 0) aligned_before = true; at += span; read_index += span; }
		else if (op == 3) at += span;          // N
		else if (op == 4) read_index += span;  // S
		else if (op == 1 || op == 2) {         // I, D
			const bool deletion = op == 2;
			const int64_t anchor = at - 1;
			if (span >= 1 && aligned_before && anchor >= 0 && anchor < (int64_t) length && (!deletion || at + (int64_t) span <= (int64_t) length)) {
				++tally.operations;
				uint64_t bases = 0;
				if (!deletion && (span > INDEL_MAX_INSERTION || !indel_pack(stream, record, read_index, span, bases))) ++tally.unkeyed;
				else {
					++tally.events;
					if (resolve) {
						bool capped;
						const uint32_t a = deletion ? indel_shift_deletion(genome, contig, (uint32_t) anchor, span, max_shift, capped) : indel_shift_insertion(genome, contig, (uint32_t) anchor, span, max_shift, bases, capped);
						if (capped) ++tally.capped;
						sink(allele_key(record.ref, a), deletion ? indel_shape_deletion(span) : indel_shape_insertion(span, bases));
					}
				}
			}
			if (deletion) at += span; else read_index += span;
		}
	}
}
struct IndelNoSink { AGPU_HD void operator()(uint64_t, uint64_t) {} };

// 64-bit arithmetic: support < 2^32, depth < 2^32
AGPU_HD bool indel_reported(uint64_t support, uint64_t depth, uint32_t min_alt, uint32_t min_percent) { return support >= min_alt && support * 100 >= (uint64_t) min_percent * depth; }

}

#endif
