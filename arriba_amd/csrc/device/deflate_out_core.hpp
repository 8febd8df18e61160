// deflate_out_core.hpp -- --sorted-bam-compression 1: the payload of a BGZF block as ONE deflate block with BFINAL = 1 (RFC 1951).  Everything that decides a byte of a compressed
// block is here, a pure function of the payload bytes, and is shared by the compressing gather of agpu_sorted_bam.hip and the host stepping of arriba_amd/csrc/host/sorted_bam.cpp
// (DESIGN.md 4.10).  The steps, each written so that lanes may run it side by side without the result depending on their order:
//   tokens     the payload is cut into segments of DFO_SEGMENT bytes; a segment is walked in rounds of DFO_ROUND positions.  Every position of a round looks its 4-byte hash up in
//              the table of its segment (position + 1 of the last earlier occurrence IN AN EARLIER ROUND), then all of them enter their own position with a maximum (an LDS
//              atomicMax on the device): all loads of a round come before its stores.  dfo_find: the candidate is checked and extended, distance 1 is probed on its own.  Matches
//              stay inside their segment (its table knows nothing else, and the next segment starts on its first byte), distance 1 may look one byte back across its front.
//              The greedy parse is a walk over the round: a match at p of length L makes p + L the next token start.
//   histogram  literal/length and distance symbols counted (sums: no order), the extra bits summed
//   codes      dfo_rank sorts the used symbols by (count, symbol); dfo_code_lengths (one lane) gives the Huffman code lengths, limited to 15 (7 for the code-length code) by
//              repairing the Kraft sum; dfo_plan (one lane) the header fields and the exact bit counts of the three encodings: the smallest wins, ties go to stored, then fixed
//   bits       dfo_token_bits / dfo_put_token: the bits of a token at a bit position that is a prefix sum of the sizes in front of it; bits are OR-ed into a zeroed image
#ifndef AGPU_DEFLATE_OUT_CORE_HPP
#define AGPU_DEFLATE_OUT_CORE_HPP 1

#include "views.hpp"

namespace agpu {

const uint32_t DFO_SEGMENT = 4096, DFO_ROUND = 64;       // (a segment is a whole number of rounds)
const uint32_t DFO_MAX_SEGMENTS = 16;                    // of a payload of up to 0xff00 bytes
const uint32_t DFO_HASH_BITS = 10, DFO_HASH_SLOTS = 1u << DFO_HASH_BITS;
const uint32_t DFO_MIN_MATCH = 4, DFO_MAX_MATCH = 258, DFO_MAX_DISTANCE = 32768;
const uint32_t DFO_LL = 286, DFO_D = 30, DFO_CL = 19, DFO_END = 256;
const uint32_t DFO_STORED = 0, DFO_FIXED = 1, DFO_DYNAMIC = 2; // BTYPE
const uint32_t DFO_TOKEN_LITERAL = 0x40000000u, DFO_TOKEN_MATCH = 0x80000000u; // a token word: the literal byte; (length - 3) << 16 | distance - 1.  0: the position starts no token

AGPU_HD uint32_t dfo_load32(const uint8_t* bytes, uint32_t at) { return (uint32_t) bytes[at] | (uint32_t) bytes[at + 1] << 8 | (uint32_t) bytes[at + 2] << 16 | (uint32_t) bytes[at + 3] << 24; }
AGPU_HD uint32_t dfo_hash(uint32_t value) { return (value * 0x9E3779B1u) >> (32 - DFO_HASH_BITS); }
AGPU_HD uint32_t dfo_segment_end(uint32_t segment_begin, uint32_t n) { return segment_begin + DFO_SEGMENT < n ? segment_begin + DFO_SEGMENT : n; }
AGPU_HD bool dfo_hashable(uint32_t p, uint32_t segment_end) { return p + DFO_MIN_MATCH <= segment_end; }

// the token a position would start: a match word, or the literal.  candidate: what the table of the segment held for the hash of `value` before this round (0: nothing)
AGPU_HD uint32_t dfo_find(const uint8_t* payload, uint32_t p, uint32_t segment_end, uint32_t candidate, uint32_t value) {
	const uint32_t limit = segment_end - p < DFO_MAX_MATCH ? segment_end - p : DFO_MAX_MATCH;
	uint32_t best = 0, distance = 0;
	if (limit >= DFO_MIN_MATCH) {
		if (candidate != 0) {
			const uint32_t c = candidate - 1;
			if (c < p && p - c <= DFO_MAX_DISTANCE && dfo_load32(payload, c) == value) {
				uint32_t length = DFO_MIN_MATCH;
				while (length < limit && payload[c + length] == payload[p + length]) ++length; // (c + length may pass p: a match may overlap itself)
				best = length; distance = p - c;
			}
		}
		if (p >= 1) {
			uint32_t length = 0;
			while (length < limit && payload[p - 1 + length] == payload[p + length]) ++length;
			if (length >= DFO_MIN_MATCH && length >= best) { best = length; distance = 1; }
		}
	}
	if (best == 0) return DFO_TOKEN_LITERAL | payload[p];
	return DFO_TOKEN_MATCH | (best - 3) << 16 | (distance - 1);
}
AGPU_HD uint32_t dfo_token_span(uint32_t token) { return (token & DFO_TOKEN_MATCH) ? ((token >> 16) & 0xFFu) + 3 : 1; } // payload bytes of the token

AGPU_HD uint32_t dfo_log2(uint32_t v) { return 31u - (uint32_t) __builtin_clz(v); } // v > 0
// length 3 .. 258 -> symbol 257 .. 285, the number of extra bits and their value (RFC 1951 3.2.5)
AGPU_HD void dfo_length_code(uint32_t length, uint32_t& symbol, uint32_t& extra_bits, uint32_t& extra_value) {
	const uint32_t l = length - 3;
	if (length == 258) { symbol = 285; extra_bits = 0; extra_value = 0; return; }
	if (l < 8) { symbol = 257 + l; extra_bits = 0; extra_value = 0; return; }
	const uint32_t e = dfo_log2(l) - 2;
	symbol = 261 + 4 * e + ((l >> e) & 3u); extra_bits = e; extra_value = l & ((1u << e) - 1);
}
// distance 1 .. 32768 -> symbol 0 .. 29
AGPU_HD void dfo_distance_code(uint32_t distance, uint32_t& symbol, uint32_t& extra_bits, uint32_t& extra_value) {
	const uint32_t d = distance - 1;
	if (d < 4) { symbol = d; extra_bits = 0; extra_value = 0; return; }
	const uint32_t e = dfo_log2(d) - 1;
	symbol = 2 * e + 2 + ((d >> e) & 1u); extra_bits = e; extra_value = d & ((1u << e) - 1);
}
AGPU_HD uint32_t dfo_fixed_length(uint32_t symbol) { return symbol < 144 ? 8 : symbol < 256 ? 9 : symbol < 280 ? 7 : 8; }
AGPU_HD uint32_t dfo_fixed_code(uint32_t symbol) { return symbol < 144 ? 0x30 + symbol : symbol < 256 ? 0x190 + (symbol - 144) : symbol < 280 ? symbol - 256 : 0xC0 + (symbol - 280); }
AGPU_HD uint32_t dfo_reverse(uint32_t code, uint32_t length) { uint32_t out = 0; for (uint32_t k = 0; k < length; ++k) { out = out << 1 | (code & 1u); code >>= 1; } return out; } // Huffman codes go out most significant bit first

// the tables of one block: in LDS on the device
struct DfoState {
	uint32_t ll_count[DFO_LL + 2], d_count[DFO_D + 2], cl_count[DFO_CL + 1]; // histograms
	uint32_t extra_bits;                       // of all tokens
	uint32_t ll_used, d_used, cl_used;         // symbols with a count
	uint16_t ll_sorted[DFO_LL + 2], d_sorted[DFO_D + 2], cl_sorted[DFO_CL + 1]; // the used symbols by (count, symbol), ascending
	uint32_t work[DFO_LL + 2], work_d[DFO_D + 2]; // dfo_code_lengths
	uint32_t per_length[2][34];                // codes per length; then the first code of every length
	uint8_t ll_length[DFO_LL + 2], d_length[DFO_D + 2], cl_length[DFO_CL + 1];
	uint16_t ll_code[DFO_LL + 2], d_code[DFO_D + 2], cl_code[DFO_CL + 1]; // already reversed: ready to be OR-ed in
	uint32_t ll_first[16], d_first[16], cl_first[16]; // canonical codes: the first code of every length
	uint32_t hlit, hdist, hclen;               // the counts themselves (257 .., 1 .., 4 ..)
	uint32_t btype, header_bits, total_bits;   // the encoding that won; the bits in front of the first token; all bits of the deflate data (stored: 8 * (n + 5))
};

// where symbol t comes among the used symbols sorted by (count, symbol); count[t] > 0
AGPU_HD uint32_t dfo_rank(const uint32_t* count, uint32_t n, uint32_t t) {
	uint32_t rank = 0; const uint32_t mine = count[t];
	for (uint32_t u = 0; u < n; ++u) { const uint32_t theirs = count[u]; if (theirs != 0 && (theirs < mine || (theirs == mine && u < t))) ++rank; }
	return rank;
}

// One lane.  sorted[0 .. used): symbols by ascending (count, symbol) -> length[symbol] (the others keep what they hold: zero them first), a complete prefix code of at most
// `limit` bits when used >= 2.  The tree is built in place over the sorted counts (two queues: the leaves and the inner nodes made so far, both ascending); lengths beyond the
// limit are repaired on the count of codes per length: the Kraft sum is brought down to 1 one unit at a time, then the most frequent symbols take the shortest lengths.
AGPU_HD void dfo_code_lengths(const uint32_t* count, const uint16_t* sorted, uint32_t used, uint32_t limit, uint32_t* work, uint32_t* per_length /* [34] */, uint8_t* length) {
	if (used == 0) return;
	if (used == 1) { length[sorted[0]] = 1; return; }
	const int n = (int) used;
	for (int i = 0; i < n; ++i) work[i] = count[sorted[i]];
	// pass 1: work[i] becomes the parent of inner node i
	work[0] += work[1];
	int root = 0, leaf = 2;
	for (int next = 1; next < n - 1; ++next) {
		if (leaf >= n || work[root] < work[leaf]) { work[next] = work[root]; work[root++] = (uint32_t) next; } else work[next] = work[leaf++];
		if (leaf >= n || (root < next && work[root] < work[leaf])) { work[next] += work[root]; work[root++] = (uint32_t) next; } else work[next] += work[leaf++];
	}
	// pass 2: depths of the inner nodes
	work[n - 2] = 0;
	for (int next = n - 3; next >= 0; --next) work[next] = work[work[next]] + 1;
	// pass 3: depths of the leaves, the deepest first
	int available = 1, inner = 0, depth = 0, next = n - 1;
	root = n - 2;
	while (available > 0) {
		while (root >= 0 && (int) work[root] == depth) { ++inner; --root; }
		while (available > inner) { work[next--] = (uint32_t) depth; --available; }
		available = 2 * inner; ++depth; inner = 0;
	}
	for (uint32_t k = 0; k < 34; ++k) per_length[k] = 0;
	for (int i = 0; i < n; ++i) ++per_length[work[i] < limit ? work[i] : limit];
	uint32_t kraft = 0;
	for (uint32_t k = 1; k <= limit; ++k) kraft += per_length[k] << (limit - k);
	while (kraft > (1u << limit)) {
		--per_length[limit];
		for (uint32_t k = limit - 1; k >= 1; --k) if (per_length[k] != 0) { --per_length[k]; per_length[k + 1] += 2; break; }
		--kraft;
	}
	uint32_t j = used;
	for (uint32_t k = 1; k <= limit; ++k) for (uint32_t c = per_length[k]; c > 0; --c) length[sorted[--j]] = (uint8_t) k;
}

// the first canonical code of every length (RFC 1951 3.2.2) from the lengths of n symbols
AGPU_HD void dfo_first_codes(const uint8_t* length, uint32_t n, uint32_t* per_length /* [34] */, uint32_t* first /* [16] */) {
	for (uint32_t k = 0; k < 16; ++k) per_length[k] = 0;
	for (uint32_t s = 0; s < n; ++s) ++per_length[length[s]];
	uint32_t code = 0; per_length[0] = 0; first[0] = 0;
	for (uint32_t k = 1; k < 16; ++k) { code = (code + per_length[k - 1]) << 1; first[k] = code; }
}
// the code of symbol s, reversed; any lane
AGPU_HD uint32_t dfo_code_of(const uint8_t* length, const uint32_t* first, uint32_t s) {
	const uint32_t mine = length[s];
	if (mine == 0) return 0;
	uint32_t before = 0;
	for (uint32_t u = 0; u < s; ++u) if (length[u] == mine) ++before;
	return dfo_reverse(first[mine] + before, mine);
}

// One lane, behind the histograms and dfo_rank of the two alphabets: the code lengths of both, the code-length code, the header fields, the bit counts, the encoding
AGPU_HD void dfo_plan_lengths(DfoState& s) {
	for (uint32_t k = 0; k < DFO_LL + 2; ++k) s.ll_length[k] = 0;
	for (uint32_t k = 0; k < DFO_D + 2; ++k) s.d_length[k] = 0;
	dfo_code_lengths(s.ll_count, s.ll_sorted, s.ll_used, 15, s.work, s.per_length[0], s.ll_length); // (the end-of-block symbol and a literal at least: two symbols or more)
	// distances: none used -> one code of zero bits; one used -> one code of one bit (RFC 1951 3.2.7)
	dfo_code_lengths(s.d_count, s.d_sorted, s.d_used, 15, s.work_d, s.per_length[1], s.d_length);
	uint32_t hlit = 257, hdist = 1;
	for (uint32_t k = 257; k < DFO_LL; ++k) if (s.ll_length[k] != 0) hlit = k + 1;
	for (uint32_t k = 1; k < DFO_D; ++k) if (s.d_length[k] != 0) hdist = k + 1;
	s.hlit = hlit; s.hdist = hdist;
	for (uint32_t k = 0; k <= DFO_CL; ++k) s.cl_count[k] = 0;
	for (uint32_t k = 0; k < hlit; ++k) ++s.cl_count[s.ll_length[k]];
	for (uint32_t k = 0; k < hdist; ++k) ++s.cl_count[s.d_length[k]];
}
// where the code-length symbols go in the header (RFC 1951 3.2.7)
AGPU_HD uint32_t dfo_code_length_order(uint32_t k) {
	switch (k) { case 0: return 16; case 1: return 17; case 2: return 18; case 3: return 0; case 4: return 8; case 5: return 7; case 6: return 9; case 7: return 6; case 8: return 10; case 9: return 5;
		case 10: return 11; case 11: return 4; case 12: return 12; case 13: return 3; case 14: return 13; case 15: return 2; case 16: return 14; case 17: return 1; default: return 15; }
}
// One lane, behind dfo_plan_lengths and dfo_rank of the code-length alphabet; n: payload bytes
AGPU_HD void dfo_plan(DfoState& s, uint32_t n) {
	for (uint32_t k = 0; k <= DFO_CL; ++k) s.cl_length[k] = 0;
	dfo_code_lengths(s.cl_count, s.cl_sorted, s.cl_used, 7, s.work, s.per_length[0], s.cl_length);
	if (s.cl_used == 1) s.cl_length[s.cl_sorted[0] == 0 ? 1 : 0] = 1; // (a complete code needs a second symbol)
	uint32_t hclen = 4;
	for (uint32_t k = 4; k < DFO_CL; ++k) if (s.cl_length[dfo_code_length_order(k)] != 0) hclen = k + 1;
	s.hclen = hclen;
	dfo_first_codes(s.ll_length, DFO_LL, s.per_length[0], s.ll_first);
	dfo_first_codes(s.d_length, DFO_D, s.per_length[0], s.d_first);
	dfo_first_codes(s.cl_length, DFO_CL, s.per_length[0], s.cl_first);
	uint32_t dynamic_header = 3 + 5 + 5 + 4 + 3 * hclen, dynamic_body = s.extra_bits, fixed_body = s.extra_bits;
	for (uint32_t k = 0; k < DFO_CL; ++k) dynamic_header += s.cl_count[k] * s.cl_length[k];
	for (uint32_t k = 0; k < DFO_LL; ++k) { dynamic_body += s.ll_count[k] * s.ll_length[k]; fixed_body += s.ll_count[k] * dfo_fixed_length(k); }
	for (uint32_t k = 0; k < DFO_D; ++k) { dynamic_body += s.d_count[k] * s.d_length[k]; fixed_body += s.d_count[k] * 5; }
	const uint32_t stored = 8 * (n + 5), fixed = 3 + fixed_body, dynamic = dynamic_header + dynamic_body;
	s.btype = DFO_STORED; s.header_bits = 0; s.total_bits = stored;
	if (fixed < s.total_bits) { s.btype = DFO_FIXED; s.header_bits = 3; s.total_bits = fixed; }
	if (dynamic < s.total_bits) { s.btype = DFO_DYNAMIC; s.header_bits = dynamic_header; s.total_bits = dynamic; }
}

// the symbols of a token for the histograms: literal/length symbol, distance symbol (DFO_D: none), extra bits of both
AGPU_HD void dfo_token_symbols(uint32_t token, uint32_t& ll, uint32_t& d, uint32_t& extra_bits) {
	if (!(token & DFO_TOKEN_MATCH)) { ll = token & 0xFFu; d = DFO_D; extra_bits = 0; return; }
	uint32_t bits_l, value_l, bits_d, value_d;
	dfo_length_code(((token >> 16) & 0xFFu) + 3, ll, bits_l, value_l);
	dfo_distance_code((token & 0xFFFFu) + 1, d, bits_d, value_d);
	extra_bits = bits_l + bits_d;
}
// the bits of a token in the encoding that won: up to four pieces (code, extra, code, extra) of at most 15 bits each, as value[k] / bits[k]; returns their sum
AGPU_HD uint32_t dfo_token_pieces(const DfoState& s, uint32_t token, uint32_t value[4], uint32_t bits[4]) {
	const bool fixed = s.btype == DFO_FIXED;
	if (!(token & DFO_TOKEN_MATCH)) {
		const uint32_t ll = token & 0xFFu;
		bits[0] = fixed ? dfo_fixed_length(ll) : s.ll_length[ll]; value[0] = fixed ? dfo_reverse(dfo_fixed_code(ll), bits[0]) : s.ll_code[ll];
		bits[1] = bits[2] = bits[3] = 0; value[1] = value[2] = value[3] = 0;
		return bits[0];
	}
	uint32_t ll, d;
	dfo_length_code(((token >> 16) & 0xFFu) + 3, ll, bits[1], value[1]);
	dfo_distance_code((token & 0xFFFFu) + 1, d, bits[3], value[3]);
	bits[0] = fixed ? dfo_fixed_length(ll) : s.ll_length[ll]; value[0] = fixed ? dfo_reverse(dfo_fixed_code(ll), bits[0]) : s.ll_code[ll];
	bits[2] = fixed ? 5 : s.d_length[d]; value[2] = fixed ? dfo_reverse(d, 5) : s.d_code[d];
	return bits[0] + bits[1] + bits[2] + bits[3];
}
AGPU_HD uint32_t dfo_token_bits(const DfoState& s, uint32_t token) {
	if (token == 0) return 0;
	uint32_t ll, d, extra;
	dfo_token_symbols(token, ll, d, extra);
	if (s.btype == DFO_FIXED) return dfo_fixed_length(ll) + (d < DFO_D ? 5 : 0) + extra;
	return s.ll_length[ll] + (d < DFO_D ? s.d_length[d] : 0) + extra;
}

// `bits` <= 16 bits of `value` at bit position `at` of a zeroed image of 32-bit little-endian words.  Or: (word index, bits to OR in)
template <class Or> AGPU_HD void dfo_put(uint32_t at, uint32_t value, uint32_t bits, Or or_word) {
	if (bits == 0) return;
	const uint32_t shift = (uint32_t) (at & 31u);
	or_word((uint32_t) (at >> 5), value << shift);
	if (shift + bits > 32) or_word((uint32_t) (at >> 5) + 1, value >> (32 - shift));
}
template <class Or> AGPU_HD void dfo_put_token(const DfoState& s, uint32_t at, uint32_t token, Or or_word) {
	uint32_t value[4], bits[4];
	dfo_token_pieces(s, token, value, bits);
	dfo_put(at, value[0], bits[0], or_word); at += bits[0];
	dfo_put(at, value[1], bits[1], or_word); at += bits[1];
	dfo_put(at, value[2], bits[2], or_word); at += bits[2];
	dfo_put(at, value[3], bits[3], or_word);
}
// One lane: BFINAL, BTYPE and, for a dynamic block, the code lengths (each one sent by itself: the run-length symbols 16 to 18 are not used); s.header_bits bits from `at` on
template <class Or> AGPU_HD void dfo_put_header(const DfoState& s, uint32_t at, Or or_word) {
	dfo_put(at, 1u | s.btype << 1, 3, or_word); at += 3;
	if (s.btype != DFO_DYNAMIC) return;
	dfo_put(at, s.hlit - 257, 5, or_word); at += 5;
	dfo_put(at, s.hdist - 1, 5, or_word); at += 5;
	dfo_put(at, s.hclen - 4, 4, or_word); at += 4;
	for (uint32_t k = 0; k < s.hclen; ++k) { dfo_put(at, s.cl_length[dfo_code_length_order(k)], 3, or_word); at += 3; }
	for (uint32_t k = 0; k < s.hlit; ++k) { const uint32_t l = s.ll_length[k]; dfo_put(at, s.cl_code[l], s.cl_length[l], or_word); at += s.cl_length[l]; }
	for (uint32_t k = 0; k < s.hdist; ++k) { const uint32_t l = s.d_length[k]; dfo_put(at, s.cl_code[l], s.cl_length[l], or_word); at += s.cl_length[l]; }
}
// the end-of-block symbol: (value, bits)
AGPU_HD uint32_t dfo_end_bits(const DfoState& s) { return s.btype == DFO_FIXED ? 7 : s.ll_length[DFO_END]; }
AGPU_HD uint32_t dfo_end_value(const DfoState& s) { return s.btype == DFO_FIXED ? 0 : s.ll_code[DFO_END]; }

// bytes of the block around deflate data of `total_bits` bits: the 18 bytes of the gzip header with the BC subfield, the data, CRC-32 and ISIZE
AGPU_HD uint32_t dfo_block_bytes(uint32_t total_bits) { return 18 + (total_bits + 7) / 8 + 8; }

}

#endif
