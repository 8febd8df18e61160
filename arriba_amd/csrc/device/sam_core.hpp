// arriba_amd/csrc/device/sam_core.hpp -- one line of SAM text -> the BAM record `samtools view -b` writes for it (SAMv1 section 4.2; the reference opens -x with
// sam_open, which reads both: source/read_chimeric_alignments.cpp:563).  Compiled for the device (agpu_sam.hip: sam_size_kernel / sam_emit_kernel) and for the host
// (arriba_amd/csrc/host: ahost_sam_transcode, the host ingest), like the other *_core.hpp: the host steps the very code the kernels run.
//
// sam_line<false> validates a line and returns the size of its record (0: the line is malformed, `reason` says why); sam_line<true> runs the same walk again and
// writes the bytes.  Both read line[0 .. n) only -- every loop is bounded by n, whatever the line holds -- and keep no array that is indexed at run time: the
// cursor walks the fields in order, the 4-bit base codes come out of two 64-bit constants.
#ifndef AGPU_SAM_CORE_HPP
#define AGPU_SAM_CORE_HPP 1

#include <stdint.h>
#include "views.hpp"

namespace agpu {

enum SamReason { SAM_OK = 0, SAM_FEW_FIELDS = 1, SAM_EMPTY_LINE = 2, SAM_HEADER_LINE = 3, SAM_BAD_NUMBER = 4, SAM_UNKNOWN_REFERENCE = 5, SAM_BAD_CIGAR = 6, SAM_QUAL_LENGTH = 7,
                 SAM_BAD_TAG = 8, SAM_BAD_NAME = 9, SAM_REASONS = 10 };
inline const char* sam_reason_text(uint32_t reason) {
	switch (reason) {
		case SAM_FEW_FIELDS: return "fewer than 11 fields";
		case SAM_EMPTY_LINE: return "empty line";
		case SAM_HEADER_LINE: return "header line behind the first alignment";
		case SAM_BAD_NUMBER: return "malformed number in a mandatory field";
		case SAM_UNKNOWN_REFERENCE: return "reference name that no @SQ line declares";
		case SAM_BAD_CIGAR: return "malformed CIGAR";
		case SAM_QUAL_LENGTH: return "SEQ and QUAL are of different length";
		case SAM_BAD_TAG: return "malformed optional field";
		case SAM_BAD_NAME: return "read name empty or longer than 254 characters";
		default: return "malformed line";
	}
}

// the @SQ names in tid order (names[name_offset[t] .. name_offset[t + 1])) and an open-addressing table over them: slot = tid + 1, 0 = free; at most half full
struct SamTargets { const char* names; const uint32_t* name_offset; const uint32_t* table; uint32_t mask; uint32_t n; };

template <class Bytes> AGPU_HD uint32_t sam_name_hash(Bytes s, uint32_t begin, uint32_t end) { // FNV-1a
	uint32_t h = 2166136261u;
	for (uint32_t i = begin; i < end; ++i) h = (h ^ (uint8_t) s[i]) * 16777619u;
	return h;
}
inline uint32_t sam_table_slots(uint32_t n_targets) { uint32_t slots = 4; while (slots < 2 * (uint64_t) n_targets + 2) slots *= 2; return slots; }
// fills table[sam_table_slots(n)] (host side, once per ingest); of two equal names the first keeps the name
inline void sam_build_table(const char* names, const uint32_t* name_offset, uint32_t n, uint32_t* table) {
	const uint32_t slots = sam_table_slots(n), mask = slots - 1;
	for (uint32_t k = 0; k < slots; ++k) table[k] = 0;
	for (uint32_t t = 0; t < n; ++t) {
		uint32_t h = sam_name_hash(names, name_offset[t], name_offset[t + 1]) & mask;
		while (table[h] != 0) h = (h + 1) & mask;
		table[h] = t + 1;
	}
}
// RNAME / RNEXT -> refID: by hash, then verified by comparing the strings; -2 = no such name
AGPU_HD int32_t sam_lookup(const SamTargets& t, const uint8_t* s, uint32_t begin, uint32_t end) {
	if (t.n == 0) return -2;
	uint32_t h = sam_name_hash(s, begin, end) & t.mask;
	for (uint32_t probes = 0; probes <= t.mask; ++probes) {
		const uint32_t slot = t.table[h];
		if (slot == 0) return -2;
		const uint32_t from = t.name_offset[slot - 1], length = t.name_offset[slot] - from;
		if (length == end - begin) {
			uint32_t k = 0;
			while (k < length && (uint8_t) t.names[from + k] == s[begin + k]) ++k;
			if (k == length) return (int32_t) (slot - 1);
		}
		h = (h + 1) & t.mask;
	}
	return -2;
}

AGPU_HD uint32_t sam_field_end(const uint8_t* s, uint32_t p, uint32_t n) { while (p < n && s[p] != '\t') ++p; return p; }
// decimal digits s[begin .. end), nothing else, at most `limit`
AGPU_HD bool sam_unsigned(const uint8_t* s, uint32_t begin, uint32_t end, uint64_t limit, uint64_t& value) {
	value = 0;
	if (begin >= end || end - begin > 18) return false;
	for (uint32_t i = begin; i < end; ++i) {
		const uint32_t digit = (uint32_t) s[i] - '0';
		if (digit > 9) return false;
		value = value * 10 + digit;
	}
	return value <= limit;
}
AGPU_HD bool sam_signed(const uint8_t* s, uint32_t begin, uint32_t end, int64_t lowest, int64_t highest, int64_t& value) {
	value = 0;
	if (begin >= end) return false;
	const bool negative = s[begin] == '-';
	if (negative || s[begin] == '+') ++begin;
	uint64_t magnitude;
	if (!sam_unsigned(s, begin, end, (uint64_t) 1 << 40, magnitude)) return false;
	value = negative ? -(int64_t) magnitude : (int64_t) magnitude;
	return value >= lowest && value <= highest;
}
// [+-]digits[.digits][e[+-]digits]: the mantissa exactly in 64 bits (digits behind the 18th only move the exponent), ONE multiplication or division by a power of ten
// that is exact up to 10^22, then the rounding to float -- multiplications and divisions only, so host and device give the same bits
AGPU_HD bool sam_float(const uint8_t* s, uint32_t begin, uint32_t end, float& value) {
	value = 0;
	if (begin >= end) return false;
	const bool negative = s[begin] == '-';
	if (negative || s[begin] == '+') ++begin;
	uint64_t mantissa = 0; int exponent = 0; bool any = false, point = false;
	uint32_t p = begin;
	for (; p < end; ++p) {
		if (s[p] == '.') { if (point) return false; point = true; continue; }
		const uint32_t digit = (uint32_t) s[p] - '0';
		if (digit > 9) break;
		any = true;
		if (mantissa < 100000000000000000ull) { mantissa = mantissa * 10 + digit; if (point) --exponent; }
		else if (!point) ++exponent;
	}
	if (!any) return false;
	if (p < end) {
		if ((s[p] | 32) != 'e') return false;
		++p;
		bool exponent_negative = false;
		if (p < end && (s[p] == '-' || s[p] == '+')) { exponent_negative = s[p] == '-'; ++p; }
		if (p >= end) return false;
		int x = 0;
		for (; p < end; ++p) { const uint32_t digit = (uint32_t) s[p] - '0'; if (digit > 9) return false; if (x < 10000) x = x * 10 + (int) digit; }
		exponent += exponent_negative ? -x : x;
	}
	double power = 1.0;
	int steps = exponent < 0 ? -exponent : exponent;
	if (steps > 400) steps = 400;
	for (int k = 0; k < steps; ++k) power *= 10.0;
	const double result = exponent < 0 ? (double) mantissa / power : (double) mantissa * power;
	value = (float) (negative ? -result : result);
	return true;
}

// "=ACMGRSVTWYHKDBN" in either case -> 0..15, anything else -> 15 (N), as htslib's seq_nt16_table has it: nibble (c & 31) of two constants
AGPU_HD uint32_t sam_base_code(uint32_t c) {
	if (c == '=') return 0;
	const uint32_t letter = c | 32;
	if (letter < 'a' || letter > 'z') return 15;
	const uint32_t index = c & 31;
	const uint64_t codes = index < 16 ? 0xFF3FCFFB4FFD2E1Full : 0xFFFFFFAF97F865FFull;
	return (uint32_t) (codes >> ((index & 15) * 4)) & 15;
}
AGPU_HD int32_t sam_cigar_op(uint32_t c) { // "MIDNSHP=X" -> 0..8
	switch (c) { case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4; case 'H': return 5; case 'P': return 6; case '=': return 7; case 'X': return 8; default: return -1; }
}
// reg2bin of SAMv1 section 5.3, on signed coordinates: an unplaced read (beg -1, end 0) falls into bin 4680
AGPU_HD uint32_t sam_reg2bin(int64_t beg, int64_t end) {
	--end;
	if (beg >> 14 == end >> 14) return (uint32_t) (((1 << 15) - 1) / 7 + (beg >> 14));
	if (beg >> 17 == end >> 17) return (uint32_t) (((1 << 12) - 1) / 7 + (beg >> 17));
	if (beg >> 20 == end >> 20) return (uint32_t) (((1 << 9) - 1) / 7 + (beg >> 20));
	if (beg >> 23 == end >> 23) return (uint32_t) (((1 << 6) - 1) / 7 + (beg >> 23));
	if (beg >> 26 == end >> 26) return (uint32_t) (((1 << 3) - 1) / 7 + (beg >> 26));
	return 0;
}

// the bytes of a record as they come; SIZE only counts
template <bool EMIT> struct SamWriter {
	uint8_t* out; uint32_t at;
	AGPU_HD void u8(uint32_t v) { if (EMIT) out[at] = (uint8_t) v; ++at; }
	AGPU_HD void u16(uint32_t v) { u8(v); u8(v >> 8); }
	AGPU_HD void u32(uint32_t v) { u8(v); u8(v >> 8); u8(v >> 16); u8(v >> 24); }
};

// one value of an optional field of type c C s S i I f (the elements of a B array)
template <bool EMIT> AGPU_HD bool sam_array_value(const uint8_t* s, uint32_t begin, uint32_t end, uint32_t subtype, SamWriter<EMIT>& w) {
	if (subtype == 'f') { float v; if (!sam_float(s, begin, end, v)) return false; uint32_t bits; { union { float f; uint32_t u; } cast; cast.f = v; bits = cast.u; } w.u32(bits); return true; }
	int64_t lowest, highest; uint32_t width;
	switch (subtype) {
		case 'c': lowest = -128; highest = 127; width = 1; break;
		case 'C': lowest = 0; highest = 255; width = 1; break;
		case 's': lowest = -32768; highest = 32767; width = 2; break;
		case 'S': lowest = 0; highest = 65535; width = 2; break;
		case 'i': lowest = -2147483648ll; highest = 2147483647ll; width = 4; break;
		case 'I': lowest = 0; highest = 4294967295ll; width = 4; break;
		default: return false;
	}
	int64_t v;
	if (!sam_signed(s, begin, end, lowest, highest, v)) return false;
	if (width == 1) w.u8((uint32_t) v); else if (width == 2) w.u16((uint32_t) v); else w.u32((uint32_t) v);
	return true;
}

// line[0 .. n): the line without its "\n" and without one "\r" in front of that.  Returns the size of the record including its block_size word; 0 = malformed.
template <bool EMIT> AGPU_HD uint32_t sam_line(const uint8_t* line, uint32_t n, const SamTargets& targets, uint8_t* out, uint32_t& reason) {
	reason = SAM_OK;
	if (n == 0) { reason = SAM_EMPTY_LINE; return 0; }
	if (line[0] == '@') { reason = SAM_HEADER_LINE; return 0; }
	{ uint32_t tabs = 0; for (uint32_t i = 0; i < n && tabs < 10; ++i) tabs += line[i] == '\t'; if (tabs < 10) { reason = SAM_FEW_FIELDS; return 0; } }
	SamWriter<EMIT> w = { out, 0 };
	uint64_t number; int64_t signed_number;
	// the ten tabs are there: every field_end below stops at one until the tenth is passed
	const uint32_t qname_end = sam_field_end(line, 0, n);
	if (qname_end == 0 || qname_end > 254) { reason = SAM_BAD_NAME; return 0; }
	uint32_t p = qname_end + 1, e = sam_field_end(line, p, n);
	if (!sam_unsigned(line, p, e, 65535, number)) { reason = SAM_BAD_NUMBER; return 0; }
	const uint32_t flag = (uint32_t) number;
	p = e + 1; e = sam_field_end(line, p, n);
	int32_t ref = -1;
	if (!(e - p == 1 && line[p] == '*')) { ref = sam_lookup(targets, line, p, e); if (ref < 0) { reason = SAM_UNKNOWN_REFERENCE; return 0; } }
	p = e + 1; e = sam_field_end(line, p, n);
	if (!sam_unsigned(line, p, e, 2147483647, number)) { reason = SAM_BAD_NUMBER; return 0; }
	const int32_t pos = (int32_t) number - 1;
	p = e + 1; e = sam_field_end(line, p, n);
	if (!sam_unsigned(line, p, e, 255, number)) { reason = SAM_BAD_NUMBER; return 0; }
	const uint32_t mapq = (uint32_t) number;
	p = e + 1; e = sam_field_end(line, p, n);
	const uint32_t cigar_begin = p, cigar_end = e;
	uint32_t n_cigar = 0; uint64_t reference_length = 0;
	if (!(e - p == 1 && line[p] == '*')) {
		if (p == e) { reason = SAM_BAD_CIGAR; return 0; }
		uint32_t i = p;
		while (i < e) {
			uint64_t length = 0; uint32_t digits = 0;
			while (i < e && (uint32_t) line[i] - '0' <= 9) { if (length < ((uint64_t) 1 << 32)) length = length * 10 + ((uint32_t) line[i] - '0'); ++i; ++digits; }
			const int32_t op = i < e ? sam_cigar_op(line[i]) : -1;
			if (digits == 0 || op < 0 || length >= (1u << 28)) { reason = SAM_BAD_CIGAR; return 0; }
			if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) reference_length += length;
			++i;
			if (++n_cigar > 65535) { reason = SAM_BAD_CIGAR; return 0; }
		}
	}
	p = e + 1; e = sam_field_end(line, p, n);
	int32_t next_ref = -1;
	if (e - p == 1 && line[p] == '=') next_ref = ref;
	else if (!(e - p == 1 && line[p] == '*')) { next_ref = sam_lookup(targets, line, p, e); if (next_ref < 0) { reason = SAM_UNKNOWN_REFERENCE; return 0; } }
	p = e + 1; e = sam_field_end(line, p, n);
	if (!sam_unsigned(line, p, e, 2147483647, number)) { reason = SAM_BAD_NUMBER; return 0; }
	const int32_t next_pos = (int32_t) number - 1;
	p = e + 1; e = sam_field_end(line, p, n);
	if (!sam_signed(line, p, e, -2147483648ll, 2147483647ll, signed_number)) { reason = SAM_BAD_NUMBER; return 0; }
	const int32_t tlen = (int32_t) signed_number;
	p = e + 1; e = sam_field_end(line, p, n);
	const uint32_t seq_begin = p;
	const uint32_t l_seq = (e - p == 1 && line[p] == '*') ? 0 : e - p;
	p = e + 1; e = sam_field_end(line, p, n); // (the tenth tab is behind us: e may be n from here on)
	const uint32_t qual_begin = p;
	const bool no_qual = e - p == 1 && line[p] == '*';
	if (!no_qual && e - p != l_seq) { reason = SAM_QUAL_LENGTH; return 0; }

	if (reference_length == 0 || (flag & 4)) reference_length = 1;
	const uint32_t bin = sam_reg2bin(pos, (int64_t) pos + (int64_t) reference_length);
	w.u32(0); // block_size: known at the end
	w.u32((uint32_t) ref); w.u32((uint32_t) pos); w.u8(qname_end + 1); w.u8(mapq); w.u16(bin); w.u16(n_cigar); w.u16(flag); w.u32(l_seq); w.u32((uint32_t) next_ref); w.u32((uint32_t) next_pos); w.u32((uint32_t) tlen);
	for (uint32_t i = 0; i < qname_end; ++i) w.u8(line[i]);
	w.u8(0);
	if (EMIT) {
		uint32_t i = cigar_begin;
		for (uint32_t k = 0; k < n_cigar; ++k) {
			uint32_t length = 0;
			while (i < cigar_end && (uint32_t) line[i] - '0' <= 9) { length = length * 10 + ((uint32_t) line[i] - '0'); ++i; }
			const int32_t op = i < cigar_end ? sam_cigar_op(line[i]) : 0;
			++i;
			w.u32(length << 4 | (uint32_t) op);
		}
		for (uint32_t i = 0; i < l_seq; i += 2) w.u8(sam_base_code(line[seq_begin + i]) << 4 | (i + 1 < l_seq ? sam_base_code(line[seq_begin + i + 1]) : 0));
		for (uint32_t i = 0; i < l_seq; ++i) w.u8(no_qual ? 0xFF : (uint32_t) line[qual_begin + i] - 33);
	} else w.at += 4 * n_cigar + (l_seq + 1) / 2 + l_seq;

	// optional fields TAG:TYPE:VALUE
	while (e < n) {
		p = e + 1; e = sam_field_end(line, p, n);
		if (e - p < 5 || line[p + 2] != ':' || line[p + 4] != ':') { reason = SAM_BAD_TAG; return 0; }
		const uint32_t type = line[p + 3], v = p + 5;
		w.u8(line[p]); w.u8(line[p + 1]);
		if (type == 'A') {
			if (e - v != 1) { reason = SAM_BAD_TAG; return 0; }
			w.u8('A'); w.u8(line[v]);
		} else if (type == 'i') {
			if (!sam_signed(line, v, e, -2147483648ll, 4294967295ll, signed_number)) { reason = SAM_BAD_TAG; return 0; }
			// the smallest type that holds the value, as htslib chooses it
			if (signed_number < 0) {
				if (signed_number >= -128) { w.u8('c'); w.u8((uint32_t) signed_number); }
				else if (signed_number >= -32768) { w.u8('s'); w.u16((uint32_t) signed_number); }
				else { w.u8('i'); w.u32((uint32_t) signed_number); }
			} else {
				if (signed_number <= 255) { w.u8('C'); w.u8((uint32_t) signed_number); }
				else if (signed_number <= 65535) { w.u8('S'); w.u16((uint32_t) signed_number); }
				else { w.u8('I'); w.u32((uint32_t) signed_number); }
			}
		} else if (type == 'f') {
			w.u8('f');
			if (!sam_array_value<EMIT>(line, v, e, 'f', w)) { reason = SAM_BAD_TAG; return 0; }
		} else if (type == 'Z' || type == 'H') {
			if (type == 'H' && ((e - v) & 1)) { reason = SAM_BAD_TAG; return 0; }
			w.u8(type);
			for (uint32_t i = v; i < e; ++i) w.u8(line[i]);
			w.u8(0);
		} else if (type == 'B') {
			if (v >= e) { reason = SAM_BAD_TAG; return 0; }
			const uint32_t subtype = line[v];
			uint32_t count = 0;
			for (uint32_t i = v + 1; i < e; ++i) count += line[i] == ',';
			if (v + 1 < e && line[v + 1] != ',') { reason = SAM_BAD_TAG; return 0; }
			w.u8('B'); w.u8(subtype); w.u32(count);
			uint32_t i = v + 1;
			if (count == 0 && subtype != 'c' && subtype != 'C' && subtype != 's' && subtype != 'S' && subtype != 'i' && subtype != 'I' && subtype != 'f') { reason = SAM_BAD_TAG; return 0; }
			while (i < e) { // (line[i] is a comma)
				uint32_t value_end = i + 1;
				while (value_end < e && line[value_end] != ',') ++value_end;
				if (!sam_array_value<EMIT>(line, i + 1, value_end, subtype, w)) { reason = SAM_BAD_TAG; return 0; }
				i = value_end;
			}
		} else { reason = SAM_BAD_TAG; return 0; }
	}
	if (EMIT) { const uint32_t block_size = w.at - 4; out[0] = (uint8_t) block_size; out[1] = (uint8_t) (block_size >> 8); out[2] = (uint8_t) (block_size >> 16); out[3] = (uint8_t) (block_size >> 24); }
	return w.at;
}

// the end of the line that starts at `begin` in text[0 .. size): index of its "\n", or size when the last line has none
template <class Bytes> AGPU_HD uint64_t sam_line_feed(Bytes text, uint64_t begin, uint64_t size) { while (begin < size && text[begin] != '\n') ++begin; return begin; }

}

#endif
