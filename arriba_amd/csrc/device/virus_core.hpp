// virus_core.hpp -- --virus-expression: what decides a number of the table that the reference's workflow gets from scripts/quantify_virus_expression.sh (default parameters),
// shared by the kernels of agpu_virus.hip and the host stepping of arriba_amd/csrc/host/virus.cpp (DESIGN.md 4.11 has the rule in full):
//   virus_parse        flag, refID, POS and where CIGAR and SEQ of a record lie; nothing outside the record is ever read, a record whose fields do not fit it is no candidate
//   virus_flag_ok / virus_cigar_ok   mapped, proper pair or single-end; a CIGAR that is not empty and holds M, N and X only
//   virus_tandem       eight copies of one ACGT dinucleotide with at most one character between consecutive copies
//   virus_kmer_count / virus_kmer_key   the 12-mers that start at the 1-based positions 1 .. l_seq - 12 as 48 bits of nibbles above 16 bits of virus slot
//   virus_cover        the reference positions M and X mark, as masks of 32-bit words of a bitmap, cut to the contig
#ifndef AGPU_VIRUS_CORE_HPP
#define AGPU_VIRUS_CORE_HPP 1

#include "sorted_bam_core.hpp"

namespace agpu {

const uint32_t VIRUS_KMER = 12;              // KMER_LENGTH of the script
const uint32_t VIRUS_TANDEM_COPIES = 8;
const uint32_t VIRUS_MAX_SLOTS = 65535;      // viral contigs a key can name
const uint32_t VIRUS_NO_SLOT = 0xFFFFFFFFu;
const uint32_t VIRUS_SHARED_PCT = 10, VIRUS_MIN_COVERED_PCT = 5, VIRUS_MIN_COVERED_BASES = 100;

struct VirusRecord {
	uint32_t flag, l_seq, n_cigar;
	int32_t ref, pos;
	uint64_t cigar_at, seq_at;  // offsets in the stream
	bool whole;                 // CIGAR and SEQ lie inside the record
};

AGPU_HD VirusRecord virus_parse(const uint8_t* stream, uint64_t at, uint64_t stream_size) {
	VirusRecord r;
	r.flag = 4; r.l_seq = 0; r.n_cigar = 0; r.ref = -1; r.pos = -1; r.cigar_at = at; r.seq_at = at; r.whole = false;
	if (at + 36 > stream_size) return r;
	uint64_t size = (uint64_t) sbam_load32(stream, at) + 4;
	if (size > stream_size - at) size = stream_size - at;
	r.ref = (int32_t) sbam_load32(stream, at + 4); r.pos = (int32_t) sbam_load32(stream, at + 8);
	const uint32_t l_read_name = stream[at + 12];
	r.n_cigar = sbam_load16(stream, at + 16); r.flag = sbam_load16(stream, at + 18);
	r.l_seq = sbam_load32(stream, at + 20);
	r.cigar_at = at + 36 + l_read_name; r.seq_at = r.cigar_at + 4ull * r.n_cigar;
	r.whole = r.l_seq <= 0x7FFFFFFFu && 36ull + l_read_name + 4ull * r.n_cigar + ((uint64_t) r.l_seq + 1) / 2 <= size;
	return r;
}

AGPU_HD bool virus_mapped(uint32_t flag) { return (flag & 4u) == 0; }
AGPU_HD bool virus_flag_ok(uint32_t flag) { return (flag & 4u) == 0 && ((flag & 2u) != 0 || (flag & 1u) == 0); }
AGPU_HD bool virus_cigar_ok(const uint8_t* stream, uint64_t cigar_at, uint32_t n_cigar) {
	if (n_cigar == 0) return false;
	for (uint32_t k = 0; k < n_cigar; ++k) {
		const uint32_t op = sbam_load32(stream, cigar_at + 4ull * k) & 15u;
		if (!((0x109u >> op) & 1u)) return false; // M (0), N (3), X (8)
	}
	return true;
}

// base p of a packed sequence as its 4-bit code ("=ACMGRSVTWYHKDBN"): the high nibble of a byte comes first
AGPU_HD uint32_t virus_nibble(const uint8_t* seq, uint32_t p) { return ((uint32_t) seq[p >> 1] >> ((~p & 1u) << 2)) & 15u; }
AGPU_HD bool virus_acgt(uint32_t code) { return code == 1 || code == 2 || code == 4 || code == 8; }

// f[p] = 1 + max(f[p-2], f[p-3]) over the earlier positions with the same dinucleotide; a match iff some f[p] >= 8.  Three positions of history, in registers.
AGPU_HD bool virus_tandem(const uint8_t* seq, uint32_t l_seq) {
	if (l_seq < 2 * VIRUS_TANDEM_COPIES) return false;
	uint32_t d1 = 256, d2 = 256, d3 = 256, f1 = 0, f2 = 0, f3 = 0; // dinucleotide and f of p-1, p-2, p-3 (256: none)
	uint32_t byte = seq[0];
	uint32_t first = byte >> 4;
	for (uint32_t p = 0; p + 1 < l_seq; ++p) {
		uint32_t second;
		if (p & 1u) { byte = seq[(p + 1) >> 1]; second = byte >> 4; } else second = byte & 15u;
		uint32_t d = 256, f = 0;
		if (virus_acgt(first) && virus_acgt(second)) {
			d = first << 4 | second;
			f = 1;
			if (d2 == d && f2 + 1 > f) f = f2 + 1;
			if (d3 == d && f3 + 1 > f) f = f3 + 1;
			if (f >= VIRUS_TANDEM_COPIES) return true;
		}
		d3 = d2; f3 = f2; d2 = d1; f2 = f1; d1 = d; f1 = f;
		first = second;
	}
	return false;
}

// the script's loop is `i + 12 <= length`: the last 12-mer of a read is never taken
AGPU_HD uint32_t virus_kmer_count(uint32_t l_seq) { return l_seq > VIRUS_KMER ? l_seq - VIRUS_KMER : 0; }
// the 12-mer that begins at base i (0-based, i + 12 < l_seq), first base in the highest nibble, above the slot of its virus: keys sort by k-mer, then virus
AGPU_HD uint64_t virus_kmer_key(const uint8_t* seq, uint32_t i, uint32_t slot) {
	uint64_t bits = 0;
	const uint32_t first_byte = i >> 1;
	for (uint32_t b = 0; b < 7; ++b) bits = bits << 8 | seq[first_byte + b]; // 14 nibbles; base i + 12 exists, and it lies in byte first_byte + 6
	bits = ((i & 1u) ? bits >> 4 : bits >> 8) & 0xFFFFFFFFFFFFull;           // nibbles 1 .. 12 or 0 .. 11 of them
	return bits << 16 | (slot & 0xFFFFu);
}

// The positions M and X of the record mark on a contig of `length` bases, as masks of the words of its bitmap (word w holds positions 32 w .. 32 w + 31): mark(word, mask).
// What lies in front of position 0 or behind the contig is not marked.
template <class Mark> AGPU_HD void virus_cover(const uint8_t* stream, uint64_t cigar_at, uint32_t n_cigar, int32_t pos, uint32_t length, Mark mark) {
	int64_t at = pos;
	for (uint32_t k = 0; k < n_cigar; ++k) {
		const uint32_t word = sbam_load32(stream, cigar_at + 4ull * k), op = word & 15u;
		const int64_t span = word >> 4;
		if (op == 0 || op == 8) {
			int64_t begin = at < 0 ? 0 : at, end = at + span < (int64_t) length ? at + span : (int64_t) length;
			while (begin < end) {
				const uint32_t w = (uint32_t) (begin >> 5), low = (uint32_t) begin & 31u;
				const int64_t word_end = ((int64_t) w + 1) << 5;
				const uint32_t count = (uint32_t) ((end < word_end ? end : word_end) - begin);
				const uint32_t mask = (count == 32 ? 0xFFFFFFFFu : ((1u << count) - 1u)) << low;
				mark(w, mask);
				begin += count;
			}
		}
		at += span; // M, X and N advance (nothing else is in a CIGAR that passed virus_cigar_ok)
	}
}

AGPU_HD uint64_t virus_bitmap_words(uint32_t length) { return ((uint64_t) length + 31) >> 5; }

}

#endif
