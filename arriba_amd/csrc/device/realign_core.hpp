// realign_core.hpp -- --realign-reads: the -x input split into the templates that must be aligned again (unmapped, clipped at the 5' end, discordant, on a contig the assembly
// lacks) and the templates that are passed on, both as SAM text, fields 1-11 (DESIGN.md 4.18 has the rule in full).  What decides a byte of either file is here and is shared by
// the kernels of agpu_realign.hip and the host stepping of arriba_amd/csrc/host/realign_split.cpp:
//   realign_parse        the fixed part of a record and where its name, CIGAR, bases and qualities lie; valid: all of them inside the record, the references inside the header
//   realign_says         the predicate of a record: does this end ask for its template to be realigned
//   realign_head         fields 1-9 of its line, with the tab behind each, byte by byte into a sink
//   realign_tail_bytes / realign_tail_byte   SEQ, tab, QUAL, newline: their number, and byte k of them, from the packed bases and the quality bytes (no state: any lane can
//                        produce any byte)
//   realign_line_bytes / realign_line / realign_line_byte   the whole line: its length, its bytes in order, byte k of it
// Names, slots and claims of a paired-end template are those of markdup_core.hpp.  This is the inverse of sam_core.hpp: what `samtools view` prints.
#ifndef AGPU_REALIGN_CORE_HPP
#define AGPU_REALIGN_CORE_HPP 1

#include "markdup_core.hpp"

namespace agpu {

const uint32_t REALIGN_MIN_CLIP = 10; // an S of at least this length is a clip (the two digits of the script's pattern)
enum { REALIGN_FILE_REALIGN = 0, REALIGN_FILE_KEPT = 1 };

struct RealignRecord {
	bool valid;
	uint64_t name_at, cigar_at, seq_at, qual_at; // offsets in the stream
	uint32_t name_length /* without the NUL */, n_cigar, flag, mapq, l_seq;
	int32_t ref, pos, next_ref, next_pos, tlen;
};

// the references of the header, for RNAME and RNEXT
struct RealignNames { const char* names; const uint32_t* name_offset; uint32_t n_ref; };

// Nothing outside the record is read.  valid: the record lies inside the stream, holds a name and all of the fields its counts announce, and names references of the header.
AGPU_HD RealignRecord realign_parse(const uint8_t* stream, uint64_t at, uint64_t stream_size, uint32_t n_ref) {
	RealignRecord r;
	r.valid = false; r.name_at = r.cigar_at = r.seq_at = r.qual_at = 0; r.name_length = r.n_cigar = r.flag = r.mapq = r.l_seq = 0; r.ref = r.next_ref = -1; r.pos = r.next_pos = -1; r.tlen = 0;
	if (at > stream_size || stream_size - at < 36) return r;
	const uint64_t size = (uint64_t) sbam_load32(stream, at) + 4;
	if (size > stream_size - at) return r;
	r.ref = (int32_t) sbam_load32(stream, at + 4); r.pos = (int32_t) sbam_load32(stream, at + 8);
	const uint32_t l_read_name = stream[at + 12];
	r.mapq = stream[at + 13]; r.n_cigar = sbam_load16(stream, at + 16); r.flag = sbam_load16(stream, at + 18); r.l_seq = sbam_load32(stream, at + 20);
	r.next_ref = (int32_t) sbam_load32(stream, at + 24); r.next_pos = (int32_t) sbam_load32(stream, at + 28); r.tlen = (int32_t) sbam_load32(stream, at + 32);
	r.name_at = at + 36; r.name_length = l_read_name > 0 ? l_read_name - 1 : 0;
	r.cigar_at = r.name_at + l_read_name; r.seq_at = r.cigar_at + 4ull * r.n_cigar; r.qual_at = r.seq_at + ((uint64_t) r.l_seq + 1) / 2;
	if (l_read_name == 0 || r.qual_at + r.l_seq > at + size) return r;
	if (r.ref < -1 || r.next_ref < -1 || (r.ref >= 0 && (uint32_t) r.ref >= n_ref) || (r.next_ref >= 0 && (uint32_t) r.next_ref >= n_ref)) return r;
	r.valid = true;
	return r;
}

AGPU_HD bool realign_clip(uint32_t word) { return (word & 15u) == 4u && (word >> 4) >= REALIGN_MIN_CLIP; }
// a placeholder CIGAR (the real one lives in the CG field): kS mN with k = l_seq
AGPU_HD bool realign_placeholder(const uint8_t* stream, const RealignRecord& r) {
	if (r.n_cigar != 2) return false;
	const uint32_t first = sbam_load32(stream, r.cigar_at), second = sbam_load32(stream, r.cigar_at + 4);
	return (first & 15u) == 4u && (first >> 4) == r.l_seq && (second & 15u) == 3u;
}

// in_assembly[refID]: 1 if the reference is a contig of the assembly
AGPU_HD bool realign_says(const uint8_t* stream, const RealignRecord& r, bool paired, const uint8_t* in_assembly) {
	if (r.flag & 4u) return true;
	if (paired && !(r.flag & 2u)) return true;
	if (r.ref < 0 || !in_assembly[r.ref]) return true;
	if (r.n_cigar == 0) return false;
	if (!(r.flag & 0x10u)) { if (realign_clip(sbam_load32(stream, r.cigar_at))) return true; }
	else if (realign_clip(sbam_load32(stream, r.cigar_at + 4ull * (r.n_cigar - 1)))) return true;
	if (!paired) for (uint32_t k = 0; k < r.n_cigar; ++k) if (realign_clip(sbam_load32(stream, r.cigar_at + 4ull * k))) return true;
	return false;
}

// ---- the line ----
AGPU_HD uint32_t realign_digits(uint64_t value) { uint32_t digits = 1; while (value >= 10) { value /= 10; ++digits; } return digits; }
AGPU_HD uint32_t realign_signed_digits(int64_t value) { return value < 0 ? 1 + realign_digits((uint64_t) -value) : realign_digits((uint64_t) value); }
template <class Put> AGPU_HD void realign_put_number(int64_t value, Put& put) {
	uint64_t v = (uint64_t) value;
	if (value < 0) { put((uint8_t) '-'); v = (uint64_t) -value; }
	uint64_t power = 1;
	for (uint64_t rest = v; rest >= 10; rest /= 10) power *= 10;
	for (; power > 0; power /= 10) put((uint8_t) ('0' + (v / power) % 10));
}
AGPU_HD uint8_t realign_cigar_letter(uint32_t op) { return op == 0 ? 'M' : op == 1 ? 'I' : op == 2 ? 'D' : op == 3 ? 'N' : op == 4 ? 'S' : op == 5 ? 'H' : op == 6 ? 'P' : op == 7 ? '=' : op == 8 ? 'X' : '?'; }
AGPU_HD uint8_t realign_base_letter(uint32_t code) {
	// "=ACMGRSVTWYHKDBN" without a table in memory: eight bytes to a word
	const uint64_t low = 0x565352474D43413Dull /* = A C M G R S V */, high = 0x4E42444B48595754ull /* T W Y H K D B N */;
	return (uint8_t) ((code < 8 ? low >> (8 * code) : high >> (8 * (code - 8))) & 0xFFu);
}

// fields 1-9 and the tab behind each
AGPU_HD uint64_t realign_head_bytes(const uint8_t* stream, const RealignRecord& r, const RealignNames& names) {
	uint64_t bytes = (uint64_t) r.name_length + 1 + realign_digits(r.flag) + 1;
	bytes += (r.ref < 0 ? 1u : names.name_offset[r.ref + 1] - names.name_offset[r.ref]) + 1;
	bytes += realign_signed_digits((int64_t) r.pos + 1) + 1 + realign_digits(r.mapq) + 1;
	if (r.n_cigar == 0) bytes += 1;
	else for (uint32_t k = 0; k < r.n_cigar; ++k) bytes += realign_digits(sbam_load32(stream, r.cigar_at + 4ull * k) >> 4) + 1;
	bytes += 1; // the tab behind CIGAR
	bytes += (r.next_ref < 0 || r.next_ref == r.ref ? 1u : names.name_offset[r.next_ref + 1] - names.name_offset[r.next_ref]) + 1;
	bytes += realign_signed_digits((int64_t) r.next_pos + 1) + 1 + realign_signed_digits(r.tlen) + 1;
	return bytes;
}
template <class Put> AGPU_HD void realign_head(const uint8_t* stream, const RealignRecord& r, const RealignNames& names, Put& put) {
	for (uint32_t k = 0; k < r.name_length; ++k) put(stream[r.name_at + k]);
	put((uint8_t) '\t'); realign_put_number(r.flag, put); put((uint8_t) '\t');
	if (r.ref < 0) put((uint8_t) '*'); else for (uint32_t k = names.name_offset[r.ref]; k < names.name_offset[r.ref + 1]; ++k) put((uint8_t) names.names[k]);
	put((uint8_t) '\t'); realign_put_number((int64_t) r.pos + 1, put); put((uint8_t) '\t'); realign_put_number(r.mapq, put); put((uint8_t) '\t');
	if (r.n_cigar == 0) put((uint8_t) '*');
	else for (uint32_t k = 0; k < r.n_cigar; ++k) { const uint32_t word = sbam_load32(stream, r.cigar_at + 4ull * k); realign_put_number(word >> 4, put); put(realign_cigar_letter(word & 15u)); }
	put((uint8_t) '\t');
	if (r.next_ref < 0) put((uint8_t) '*'); else if (r.next_ref == r.ref) put((uint8_t) '='); else for (uint32_t k = names.name_offset[r.next_ref]; k < names.name_offset[r.next_ref + 1]; ++k) put((uint8_t) names.names[k]);
	put((uint8_t) '\t'); realign_put_number((int64_t) r.next_pos + 1, put); put((uint8_t) '\t'); realign_put_number(r.tlen, put); put((uint8_t) '\t');
}

// SEQ, tab, QUAL, newline
struct RealignTail { uint64_t seq_at; uint32_t l_seq; uint32_t no_qual; };
AGPU_HD RealignTail realign_tail_of(const uint8_t* stream, const RealignRecord& r) {
	RealignTail t; t.seq_at = r.seq_at; t.l_seq = r.l_seq; t.no_qual = r.l_seq == 0 || stream[r.qual_at] == 0xFFu ? 1u : 0u;
	return t;
}
AGPU_HD uint64_t realign_tail_bytes(const RealignTail& t) { return (t.l_seq == 0 ? 1ull : t.l_seq) + 1 + (t.no_qual ? 1ull : t.l_seq) + 1; }
AGPU_HD uint8_t realign_tail_byte(const uint8_t* stream, const RealignTail& t, uint64_t k) {
	const uint64_t seq_bytes = t.l_seq == 0 ? 1 : t.l_seq;
	if (k < seq_bytes) {
		if (t.l_seq == 0) return '*';
		const uint32_t packed = stream[t.seq_at + k / 2];
		return realign_base_letter(k & 1 ? packed & 15u : packed >> 4);
	}
	if (k == seq_bytes) return '\t';
	k -= seq_bytes + 1;
	if (t.no_qual) return k == 0 ? '*' : '\n';
	if (k < t.l_seq) return (uint8_t) (stream[t.seq_at + ((uint64_t) t.l_seq + 1) / 2 + k] + 33u);
	return '\n';
}

AGPU_HD uint64_t realign_line_bytes(const uint8_t* stream, const RealignRecord& r, const RealignNames& names) { return realign_head_bytes(stream, r, names) + realign_tail_bytes(realign_tail_of(stream, r)); }
template <class Put> AGPU_HD void realign_line(const uint8_t* stream, const RealignRecord& r, const RealignNames& names, Put& put) {
	realign_head(stream, r, names, put);
	const RealignTail tail = realign_tail_of(stream, r);
	const uint64_t bytes = realign_tail_bytes(tail);
	for (uint64_t k = 0; k < bytes; ++k) put(realign_tail_byte(stream, tail, k));
}
// byte k of the line: the head is walked up to k (it is short), the tail is addressed
struct RealignPick { uint64_t at, wanted; uint8_t byte; AGPU_HD void operator()(uint8_t b) { if (at == wanted) byte = b; ++at; } };
AGPU_HD uint8_t realign_line_byte(const uint8_t* stream, const RealignRecord& r, const RealignNames& names, uint64_t head_bytes, uint64_t k) {
	if (k >= head_bytes) return realign_tail_byte(stream, realign_tail_of(stream, r), k - head_bytes);
	RealignPick pick; pick.at = 0; pick.wanted = k; pick.byte = 0;
	realign_head(stream, r, names, pick);
	return pick.byte;
}

// ---- templates ----
// What a record is to the split.  PE: slot_first are the claims of its name (MDUP_NONE: nobody claimed the slot).
enum { REALIGN_ROLE_DROPPED = 0 /* 0x100 or 0x800 */, REALIGN_ROLE_EXTRA = 1 /* a further primary record of a claimed slot */, REALIGN_ROLE_ORPHAN = 2 /* the only claimed slot of its name */,
       REALIGN_ROLE_MATE = 3 /* slot 1 of a complete template: written by its owner */, REALIGN_ROLE_OWNER = 4 /* slot 0 of a complete template, or a primary record of a single-end stream */ };
AGPU_HD uint32_t realign_role(uint32_t flag, bool paired, uint32_t r, uint32_t first0, uint32_t first1) {
	if (!mdup_primary(flag)) return REALIGN_ROLE_DROPPED;
	if (!paired) return REALIGN_ROLE_OWNER;
	const uint32_t slot = mdup_slot(flag);
	if ((slot == 0 ? first0 : first1) != r) return REALIGN_ROLE_EXTRA;
	if ((slot == 0 ? first1 : first0) == MDUP_NONE) return REALIGN_ROLE_ORPHAN;
	return slot == 0 ? REALIGN_ROLE_OWNER : REALIGN_ROLE_MATE;
}

// the verdict of an owner: which file its template goes to and how many bytes its lines have there; mate: the parsed slot-1 record (PE), ignored when !paired
struct RealignVerdict { uint32_t file; uint64_t bytes; uint32_t placeholders; };
AGPU_HD RealignVerdict realign_verdict(const uint8_t* stream, const RealignRecord& own, const RealignRecord& mate, bool paired, const uint8_t* in_assembly, const RealignNames& names) {
	RealignVerdict v;
	const bool realign = realign_says(stream, own, paired, in_assembly) || (paired && realign_says(stream, mate, paired, in_assembly));
	v.file = realign ? REALIGN_FILE_REALIGN : REALIGN_FILE_KEPT;
	v.bytes = realign_line_bytes(stream, own, names) + (paired ? realign_line_bytes(stream, mate, names) : 0);
	v.placeholders = (realign_placeholder(stream, own) ? 1u : 0u) + (paired && realign_placeholder(stream, mate) ? 1u : 0u);
	return v;
}

}

#endif
