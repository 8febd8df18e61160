// variant_core.hpp -- --variant-sites: the positions at which the records of -x show a base that differs from the assembly (DESIGN.md 4.21 has the rule in full).  What decides a
// number of the file is here and is shared by the kernels of agpu_variants.hip and the host stepping of arriba_amd/csrc/host/variant_sites.cpp:
//   variant_event        the event test: a base under M, = or X whose column (allele_column) is one of A/C/G/T over a REF (allele_ref_base) that is one of A/C/G/T and another one
//   variant_base_event   that test for base j of an aligned block: the position inside [0, LN), the column of read index block_read + j, REF under block_at + j
//   variant_key          an event as one ascending 64-bit word, ((reference << 32 | position) << 2) | alt: equal events are neighbours behind a sort, the (up to three) alts of a
//                        site are neighbours, sites come in the order of the file
//   variant_reported     the percent test of a (support, depth) pair
// Which records count, where their SEQ and QUAL lie and the eight counters of a site are allele_core.hpp's: the row of a candidate site is the row --allele-counts gives there.
#ifndef AGPU_VARIANT_CORE_HPP
#define AGPU_VARIANT_CORE_HPP 1

#include "allele_core.hpp"

namespace agpu {

const uint32_t VARIANT_NO_EVENT = 4;         // what the event tests give for a base that is no mismatch event; an event is its alt, ALLELE_A .. ALLELE_T
const uint32_t VARIANT_MAX_REFERENCES = 1u << 30; // the reference of a key has 30 bits
const uint64_t VARIANT_MAX_EVENTS = 1ull << 31;   // of one call (ARRIBA_VARIANT_MAX_EVENTS lowers it): 16 GB of keys, twice

AGPU_HD uint32_t variant_ref_column(uint8_t ref_base) { return ref_base == 'A' ? ALLELE_A : ref_base == 'C' ? ALLELE_C : ref_base == 'G' ? ALLELE_G : ref_base == 'T' ? ALLELE_T : VARIANT_NO_EVENT; }
// column: of the base (allele_column); ref_base: upper case (allele_ref_base)
AGPU_HD uint32_t variant_event(uint32_t column, uint8_t ref_base) {
	const uint32_t ref_column = variant_ref_column(ref_base);
	return column <= ALLELE_T && ref_column != VARIANT_NO_EVENT && column != ref_column ? column : VARIANT_NO_EVENT;
}
// base j of a block of M, = or X that begins at reference position block_at with read index block_read, over a reference of `length` bases that is `contig` of the session
AGPU_HD uint32_t variant_base_event(const uint8_t* stream, const AlleleRecord& record, const GenomeView& genome, uint32_t contig, uint32_t length, int64_t block_at, uint64_t block_read, uint64_t j, uint32_t min_baseq) {
	const int64_t p = block_at + (int64_t) j;
	if (p < 0 || p >= (int64_t) length) return VARIANT_NO_EVENT;
	const uint32_t column = allele_column(stream, record, block_read + j, min_baseq);
	if (column > ALLELE_T) return VARIANT_NO_EVENT; // (before REF is read: LOWQ and N are no events whatever lies under them)
	return variant_event(column, allele_ref_base(genome, contig, (uint32_t) p));
}

AGPU_HD uint64_t variant_key(uint32_t ref, uint32_t pos, uint32_t alt) { return allele_key(ref, pos) << 2 | alt; } // ref < 2^30
AGPU_HD uint64_t variant_key_site(uint64_t key) { return key >> 2; }  // the allele_key of its site
AGPU_HD uint32_t variant_key_alt(uint64_t key) { return (uint32_t) (key & 3u); }

// depth = A + C + G + T of the row; 64-bit arithmetic: support < 2^32, depth < 2^34
AGPU_HD bool variant_reported(uint64_t support, uint64_t depth, uint32_t min_alt, uint32_t min_percent) { return support >= min_alt && support * 100 >= (uint64_t) min_percent * depth; }

// The rule of a row: counts: the eight counters of the site; support[alt]: the events of the site by alt (0 where none).  Gives the mask of the reported
// alts (bit ALLELE_A .. ALLELE_T); consistent: whether every support equals its counter -- the events of a site are the bases its counters count
AGPU_HD uint32_t variant_row_mask(const uint32_t* counts, const uint32_t* support, uint8_t ref_base, uint32_t min_alt, uint32_t min_percent, bool& consistent) {
	const uint64_t depth = (uint64_t) counts[ALLELE_A] + counts[ALLELE_C] + counts[ALLELE_G] + counts[ALLELE_T];
	const uint32_t ref_column = variant_ref_column(ref_base);
	uint32_t mask = 0;
	consistent = true;
	for (uint32_t alt = ALLELE_A; alt <= ALLELE_T; ++alt) {
		if (alt == ref_column || ref_column == VARIANT_NO_EVENT) { if (support[alt] != 0) consistent = false; continue; }
		if (support[alt] != counts[alt]) consistent = false;
		if (variant_reported(support[alt], depth, min_alt, min_percent)) mask |= 1u << alt;
	}
	return mask;
}

}

#endif
