// depth_core.hpp -- --coverage: what decides a byte of the bedGraph depth track (DESIGN.md 4.13 has the rule in full), shared by the kernels of agpu_depth.hip and the host
// stepping of arriba_amd/csrc/host/depth.cpp:
//   depth_parse        whether a record counts (flag bit 0x4 clear, 0 <= refID < n_ref, a CIGAR that is not empty and lies inside the record), its POS and where its CIGAR lies
//   depth_cover        the maximal segments of reference positions that M, =, X and D span, cut to the contig: mark(begin, end) per segment; N advances, I, S, H and P do neither
//   depth_head / depth_tail   where a run of equal depth > 0 begins and ends in the array of depths (LN + 1 slots per contig: the last slot of a contig is always 0, so a run
//                      never spans two contigs and nothing about contigs has to be known to find runs)
//   depth_contig_of    the contig of a slot, by binary search in the offsets of the contigs
//   depth_line_bytes / depth_line   NAME\tSTART\tEND\tDEPTH\n in plain decimal, byte by byte into put(byte)
#ifndef AGPU_DEPTH_CORE_HPP
#define AGPU_DEPTH_CORE_HPP 1

#include "sorted_bam_core.hpp"

namespace agpu {

struct DepthRecord {
	bool counts;
	int32_t ref, pos;
	uint32_t n_cigar;
	uint64_t cigar_at; // offset in the stream
};

// the head of the record is sbam_parse's; nothing outside the record is read
AGPU_HD DepthRecord depth_parse(const uint8_t* stream, uint64_t at, uint64_t stream_size, uint32_t n_ref) {
	DepthRecord r;
	r.counts = false; r.ref = -1; r.pos = -1; r.n_cigar = 0; r.cigar_at = at;
	if (at + 36 > stream_size) return r;
	const SbamRecord head = sbam_parse(stream, at, stream_size);
	const uint32_t l_read_name = stream[at + 12];
	r.ref = head.ref; r.pos = head.pos;
	r.n_cigar = sbam_load16(stream, at + 16);
	r.cigar_at = at + 36 + l_read_name;
	if (36ull + l_read_name + 4ull * r.n_cigar > head.size) r.n_cigar = 0;
	r.counts = (head.flag & 4u) == 0 && head.ref >= 0 && (uint32_t) head.ref < n_ref && r.n_cigar > 0;
	return r;
}

// mark(begin, end) for every maximal segment [begin, end) of positions the record covers on a contig of `length` bases, 0 <= begin < end <= length; returns their number.
// Operations that cover and follow each other (10M2D10M) are one segment.
template <class Mark> AGPU_HD uint32_t depth_cover(const uint8_t* stream, uint64_t cigar_at, uint32_t n_cigar, int32_t pos, uint32_t length, Mark mark) {
	int64_t at = pos, open_begin = 0, open_end = 0; // the segment that is not marked yet: empty while open_begin == open_end
	uint32_t segments = 0;
	for (uint32_t k = 0; k < n_cigar; ++k) {
		const uint32_t word = sbam_load32(stream, cigar_at + 4ull * k), op = word & 15u;
		const int64_t span = word >> 4;
		if ((0x185u >> op) & 1u) { // M (0), D (2), = (7), X (8)
			const int64_t begin = at < 0 ? 0 : at, end = at + span < (int64_t) length ? at + span : (int64_t) length;
			if (begin < end) {
				if (open_begin < open_end && begin == open_end) open_end = end;
				else {
					if (open_begin < open_end) { mark((uint32_t) open_begin, (uint32_t) open_end); ++segments; }
					open_begin = begin; open_end = end;
				}
			}
			at += span;
		} else if (op == 3) at += span; // N
	}
	if (open_begin < open_end) { mark((uint32_t) open_begin, (uint32_t) open_end); ++segments; }
	return segments;
}

// slot g of the array of depths with its neighbours (0 in front of the first slot and behind the last)
AGPU_HD bool depth_head(uint32_t before, uint32_t here) { return here != 0 && here != before; }
AGPU_HD bool depth_tail(uint32_t here, uint32_t after) { return here != 0 && here != after; }

// the contig t with contig_offset[t] <= slot < contig_offset[t + 1] (n_ref + 1 offsets, the last one is the number of slots; n_ref >= 1)
AGPU_HD uint32_t depth_contig_of(const uint64_t* contig_offset, uint32_t n_ref, uint64_t slot) {
	uint32_t low = 0, high = n_ref;
	while (high - low > 1) { const uint32_t middle = low + (high - low) / 2; if (contig_offset[middle] <= slot) low = middle; else high = middle; }
	return low;
}

AGPU_HD uint32_t depth_digits(uint32_t value) { uint32_t digits = 1; while (value >= 10) { value /= 10; ++digits; } return digits; }
AGPU_HD uint32_t depth_line_bytes(uint32_t name_bytes, uint32_t start, uint32_t end, uint32_t depth) { return name_bytes + 4 + depth_digits(start) + depth_digits(end) + depth_digits(depth); }
template <class Put> AGPU_HD void depth_number(uint32_t value, Put& put) {
	uint32_t power = 1;
	for (uint32_t rest = value; rest >= 10; rest /= 10) power *= 10;
	for (; power > 0; power /= 10) { put((uint8_t) ('0' + value / power)); value %= power; }
}
template <class Put> AGPU_HD void depth_line(const char* name, uint32_t name_bytes, uint32_t start, uint32_t end, uint32_t depth, Put& put) {
	for (uint32_t k = 0; k < name_bytes; ++k) put((uint8_t) name[k]);
	put((uint8_t) '\t'); depth_number(start, put);
	put((uint8_t) '\t'); depth_number(end, put);
	put((uint8_t) '\t'); depth_number(depth, put);
	put((uint8_t) '\n');
}

}

#endif
