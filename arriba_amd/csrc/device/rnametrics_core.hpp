// rnametrics_core.hpp -- --rna-metrics: the alignment QC table of the -x input (what Picard CollectRnaSeqMetrics / CollectInsertSizeMetrics, samtools flagstat and RSeQC
// read_distribution / infer_experiment / geneBody_coverage are run for): flag and MAPQ counts, bases per class of the annotation, strandedness, insert sizes and the 5'->3' coverage
// of gene bodies (DESIGN.md 4.19 has the rule in full).  What decides a number of the file is here and is shared by the kernel of agpu_rnametrics.hip and the host stepping of
// arriba_amd/csrc/host/rna_metrics.cpp:
//   rnam_class        the class of a base from the bits of its run: ribosomal, coding, UTR, intronic, intergenic -- the first that applies
//   rnam_run_of       the run of a contig's track that holds a position: a lower bound into the run starts, galloping from a hint when the caller has one
//   rnam_body_bins    a segment of a run that has a body gene -> its bins of the gene-body histogram, found with integer ceilings of k * L / 100, not base by base
//   rnam_block        one block through the runs it touches: class counters, body bins, the strand bits seen
//   rnam_record       one record: every counter and bin it adds to
// The track (agpu_region_track, include/arriba_gpu.h) is built on the host by arriba_amd/csrc/host/region_track.cpp.  Records are as sbam_parse reads them; NH is gcount_nh, the
// blocks are gcount_blocks, mapped is mdup_mapped.  The scalar counters of a lane live in RnamLane, whose words are only ever indexed by constants (registers on the device); the
// three histograms go through `hist`, which the kernel backs by LDS or global atomics and the host by plain adds.
#ifndef AGPU_RNAMETRICS_CORE_HPP
#define AGPU_RNAMETRICS_CORE_HPP 1

#include "../../../include/arriba_gpu.h"
#include "genecount_core.hpp"

namespace agpu {

// the words of a counter block, in the order of the lines of "## METRICS"; two statistics behind them; then the three histograms
enum {
	RNAM_RECORDS = 0, RNAM_SECONDARY, RNAM_SUPPLEMENTARY, RNAM_PRIMARY, RNAM_UNMAPPED, RNAM_MAPPED, RNAM_QC_FAIL, RNAM_DUPLICATE, RNAM_MULTIMAPPING, RNAM_PAIRED, RNAM_PROPER_PAIR, RNAM_READ1,
	RNAM_READ2, RNAM_MATE_UNMAPPED, RNAM_MATE_OTHER_CONTIG, RNAM_BASE_RECORDS, RNAM_BASES, RNAM_SOFT_CLIPPED_BASES, RNAM_INSERTED_BASES, RNAM_DELETED_BASES, RNAM_SKIPPED_BASES,
	RNAM_SPLICED_RECORDS, RNAM_ALIGNED_BASES, RNAM_RIBOSOMAL_BASES, RNAM_CODING_BASES, RNAM_UTR_BASES, RNAM_INTRONIC_BASES, RNAM_INTERGENIC_BASES, RNAM_UNKNOWN_CONTIG_BASES,
	RNAM_SENSE_STRAND_RECORDS, RNAM_ANTISENSE_STRAND_RECORDS, RNAM_AMBIGUOUS_STRAND_RECORDS, RNAM_NO_GENE_RECORDS, RNAM_INSERT_SIZE_PAIRS,
	RNAM_FILE_SCALARS, // (the lines of the file end here)
	RNAM_BLOCKS = RNAM_FILE_SCALARS, RNAM_SEGMENTS, // statistics: blocks of base records; the pieces of runs they were cut into
	RNAM_SCALARS,
	RNAM_MAPQ_AT = RNAM_SCALARS, RNAM_MAPQ_BINS = 256,
	RNAM_INSERT_AT = RNAM_MAPQ_AT + RNAM_MAPQ_BINS, RNAM_INSERT_BINS = 1002, // sizes 0 .. 1000 and ">1000"
	RNAM_BODY_AT = RNAM_INSERT_AT + RNAM_INSERT_BINS, RNAM_BODY_BINS = 100,
	RNAM_WORDS = RNAM_BODY_AT + RNAM_BODY_BINS
};
static_assert(RNAM_WORDS == AGPU_RNA_METRICS_WORDS && RNAM_FILE_SCALARS == AGPU_RNA_METRICS_SCALARS, "include/arriba_gpu.h states the size of a counter block");

enum : uint8_t { RNAM_BIT_R = AGPU_TRACK_RRNA, RNAM_BIT_C = AGPU_TRACK_CODING, RNAM_BIT_E = AGPU_TRACK_EXON, RNAM_BIT_GENE_FORWARD = AGPU_TRACK_GENE_FORWARD, RNAM_BIT_GENE_REVERSE = AGPU_TRACK_GENE_REVERSE };
enum { RNAM_CLASS_RIBOSOMAL = 0, RNAM_CLASS_CODING, RNAM_CLASS_UTR, RNAM_CLASS_INTRONIC, RNAM_CLASS_INTERGENIC };
const uint32_t RNAM_NO_GENE = 0xFFFFFFFFu, RNAM_FORWARD_GENE = 0x80000000u; // run_gene of a run without a body gene; gene_body[g] = L | RNAM_FORWARD_GENE of a forward gene
const uint32_t RNAM_MIN_BODY_LENGTH = 100;

AGPU_HD uint32_t rnam_class(uint32_t bits) {
	return (bits & RNAM_BIT_R) ? RNAM_CLASS_RIBOSOMAL : (bits & RNAM_BIT_C) ? RNAM_CLASS_CODING : (bits & RNAM_BIT_E) ? RNAM_CLASS_UTR : (bits & (RNAM_BIT_GENE_FORWARD | RNAM_BIT_GENE_REVERSE)) ? RNAM_CLASS_INTRONIC
	       : RNAM_CLASS_INTERGENIC;
}

struct RnamLane { uint64_t c[RNAM_SCALARS]; };
AGPU_HD void rnam_clear(RnamLane& lane) { AGPU_UNROLL for (int k = 0; k < RNAM_SCALARS; ++k) lane.c[k] = 0; }

// The run of [begin, end) that holds position p: the last one whose start is <= p.  run_start[begin] is 0, so there always is one.  near: a run of the contig whose start is <= p
// (the run the previous block ended in: blocks ascend), from which the search gallops; or `begin`.
AGPU_HD uint32_t rnam_run_of(const int32_t* run_start, uint32_t near, uint32_t end, int32_t p) {
	uint32_t low = near, step = 1;
	while (low + step < end && run_start[low + step] <= p) { low += step; step <<= 1; }
	uint32_t high = low + step < end ? low + step : end; // run_start[high] > p, or high == end
	while (high - low > 1) { // (run_start[low] <= p throughout)
		const uint32_t middle = low + (high - low) / 2;
		if (run_start[middle] <= p) low = middle; else high = middle;
	}
	return low;
}

// `count` consecutive exonic ranks from `rank` (ascending along the contig) of a gene of `body` = L | strand: offsets t = rank .. rank + count - 1 of a forward gene, mirrored
// (L - 1 - t) for a reverse one -- consecutive either way.  Bin k holds the offsets ceil(k * L / 100) .. ceil((k + 1) * L / 100) - 1.
template <class Hist> AGPU_HD void rnam_body_bins(uint32_t body, uint32_t rank, uint32_t count, Hist& hist) {
	const uint64_t L = body & ~RNAM_FORWARD_GENE;
	if (count == 0 || L < RNAM_MIN_BODY_LENGTH || (uint64_t) rank + count > L) return; // (a track that disagrees with itself adds nothing)
	const uint64_t first = (body & RNAM_FORWARD_GENE) ? rank : L - rank - count, last = first + count - 1;
	const uint64_t bin_first = 100 * first / L, bin_last = 100 * last / L;
	for (uint64_t k = bin_first; k <= bin_last; ++k) {
		const uint64_t from = (k * L + 99) / 100, to = ((k + 1) * L + 99) / 100 - 1; // the offsets of bin k
		const uint64_t a = from > first ? from : first, b = to < last ? to : last;
		if (a <= b) hist.body((uint32_t) k, b - a + 1);
	}
}

// one block [s, e] (0-based, inclusive, inside the contig) through the runs [begin, end) of its contig; near (in/out): see rnam_run_of; seen: the gene strand bits of the runs touched
template <class Hist> AGPU_HD void rnam_block(const agpu_region_track& track, uint32_t end, int32_t s, int32_t e, uint32_t& near, uint32_t& seen, RnamLane& lane, Hist& hist) {
	uint32_t k = rnam_run_of(track.run_start, near, end, s);
	int64_t at = s;
	uint64_t ribosomal = 0, coding = 0, utr = 0, intronic = 0, intergenic = 0, pieces = 0; // (added to the lane's words once, behind the walk)
	for (;;) {
		const int64_t run_last = k + 1 < end ? (int64_t) track.run_start[k + 1] - 1 : (int64_t) 0x7FFFFFFF;
		const int64_t piece_last = run_last < e ? run_last : e;
		const uint64_t length = (uint64_t) (piece_last - at + 1);
		const uint32_t bits = track.run_bits[k], kind = rnam_class(bits);
		ribosomal += kind == RNAM_CLASS_RIBOSOMAL ? length : 0; coding += kind == RNAM_CLASS_CODING ? length : 0; utr += kind == RNAM_CLASS_UTR ? length : 0;
		intronic += kind == RNAM_CLASS_INTRONIC ? length : 0; intergenic += kind == RNAM_CLASS_INTERGENIC ? length : 0;
		++pieces;
		seen |= bits & (RNAM_BIT_GENE_FORWARD | RNAM_BIT_GENE_REVERSE);
		const uint32_t gene = track.run_gene[k];
		if (gene != RNAM_NO_GENE && gene < track.n_genes) rnam_body_bins(track.gene_body[gene], track.run_rank[k] + (uint32_t) (at - track.run_start[k]), (uint32_t) length, hist);
		if (piece_last >= e) break;
		at = piece_last + 1; ++k;
	}
	lane.c[RNAM_RIBOSOMAL_BASES] += ribosomal; lane.c[RNAM_CODING_BASES] += coding; lane.c[RNAM_UTR_BASES] += utr; lane.c[RNAM_INTRONIC_BASES] += intronic; lane.c[RNAM_INTERGENIC_BASES] += intergenic;
	lane.c[RNAM_SEGMENTS] += pieces;
	near = k;
}

// what a record is counted against
struct RnamInput {
	const uint8_t* stream; uint64_t stream_size;
	agpu_region_track track;
	const uint32_t* tid_to_contig; // [n_ref] reference id -> contig of the session (anything >= track.n_contigs: none the track knows)
	const uint32_t* ref_length;    // [n_ref] LN
	uint32_t n_ref;
};

template <class Hist> struct RnamVisit {
	const RnamInput& in; uint32_t contig, begin, end; uint32_t& near; uint32_t& seen; RnamLane& lane; Hist& hist;
	AGPU_HD void operator()(int32_t s, int32_t e) {
		lane.c[RNAM_ALIGNED_BASES] += (uint64_t) (e - s) + 1;
		const bool unknown = contig >= in.track.n_contigs || begin == end;
		lane.c[RNAM_UNKNOWN_CONTIG_BASES] += unknown ? (uint64_t) (e - s) + 1 : 0; // (no branch of its own: see rnam_record)
		if (!unknown) rnam_block(in.track, end, s, e, near, seen, lane, hist);
	}
};

// The record at offset `at` of the stream.  A record whose 36 fixed bytes are cut off by the end of the stream counts as a record and nothing else; one cut short behind them is
// clamped as gcount_template clamps it.
template <class Hist> AGPU_HD void rnam_record(const RnamInput& in, uint64_t at, RnamLane& lane, Hist& hist) {
	// (Every word of the lane is added to without a branch of its own: paths that add to different words and meet again make the compiler pick the word by a pointer, which takes the
	// words out of the registers.)
	const bool whole = at < in.stream_size && in.stream_size - at >= 36;
	lane.c[RNAM_RECORDS] += 1;
	if (!whole) return;
	uint64_t size = (uint64_t) sbam_load32(in.stream, at) + 4;
	if (size > in.stream_size - at) size = in.stream_size - at;
	const int32_t ref = (int32_t) sbam_load32(in.stream, at + 4), pos = (int32_t) sbam_load32(in.stream, at + 8);
	const uint32_t l_read_name = in.stream[at + 12], mapq = in.stream[at + 13], flag = sbam_load16(in.stream, at + 18);
	const bool secondary = (flag & 0x100u) != 0, supplementary = !secondary && (flag & 0x800u) != 0, primary = !secondary && !supplementary, mapped = primary && mdup_mapped(flag, ref);
	lane.c[RNAM_SECONDARY] += secondary ? 1 : 0;
	lane.c[RNAM_SUPPLEMENTARY] += supplementary ? 1 : 0;
	lane.c[RNAM_PRIMARY] += primary ? 1 : 0;
	lane.c[RNAM_UNMAPPED] += primary && !mapped ? 1 : 0;
	if (!mapped) return;
	const uint64_t l_seq = sbam_load32(in.stream, at + 20);
	const int32_t next_ref = (int32_t) sbam_load32(in.stream, at + 24), tlen = (int32_t) sbam_load32(in.stream, at + 32);
	uint32_t n_cigar = sbam_load16(in.stream, at + 16);
	const uint64_t aux = 36ull + l_read_name + 4ull * n_cigar + (l_seq + 1) / 2 + l_seq;
	const bool paired = (flag & 1u) != 0;
	lane.c[RNAM_MAPPED] += 1;
	lane.c[RNAM_QC_FAIL] += (flag & 0x200u) ? 1 : 0;
	lane.c[RNAM_DUPLICATE] += (flag & 0x400u) ? 1 : 0;
	lane.c[RNAM_MULTIMAPPING] += aux < size && gcount_nh(in.stream, at + aux, at + size) > 1 ? 1 : 0;
	lane.c[RNAM_PAIRED] += paired ? 1 : 0;
	lane.c[RNAM_PROPER_PAIR] += paired && (flag & 2u) ? 1 : 0;
	lane.c[RNAM_READ1] += paired && (flag & 0x40u) ? 1 : 0;
	lane.c[RNAM_READ2] += paired && (flag & 0x80u) ? 1 : 0;
	lane.c[RNAM_MATE_UNMAPPED] += paired && (flag & 8u) ? 1 : 0;
	lane.c[RNAM_MATE_OTHER_CONTIG] += paired && !(flag & 8u) && next_ref != ref ? 1 : 0;
	hist.mapq(mapq);
	if ((flag & 0x200u) || pos < 0 || (uint32_t) ref >= in.n_ref) return; // no base record
	lane.c[RNAM_BASE_RECORDS] += 1;
	lane.c[RNAM_BASES] += l_seq;
	if (36ull + l_read_name + 4ull * n_cigar > size) n_cigar = 0;
	const uint64_t cigar_at = at + 36 + l_read_name;
	bool spliced = false;
	uint64_t soft_clipped = 0, inserted = 0, deleted = 0, skipped = 0;
	for (uint32_t k = 0; k < n_cigar; ++k) { // (lengths as written: nothing here is clipped to the contig)
		const uint32_t word = sbam_load32(in.stream, cigar_at + 4ull * k), op = word & 15u;
		const uint64_t span = word >> 4;
		soft_clipped += op == 4 ? span : 0; inserted += op == 1 ? span : 0; deleted += op == 2 ? span : 0; skipped += op == 3 ? span : 0;
		spliced = spliced || op == 3;
	}
	lane.c[RNAM_SOFT_CLIPPED_BASES] += soft_clipped; lane.c[RNAM_INSERTED_BASES] += inserted; lane.c[RNAM_DELETED_BASES] += deleted; lane.c[RNAM_SKIPPED_BASES] += skipped;
	lane.c[RNAM_SPLICED_RECORDS] += spliced ? 1 : 0;
	const uint32_t contig = in.tid_to_contig[ref];
	uint32_t begin = 0, end = 0, seen = 0;
	if (contig < in.track.n_contigs) { begin = in.track.contig_offset[contig]; end = in.track.contig_offset[contig + 1]; }
	uint32_t near = begin;
	RnamVisit<Hist> visit = { in, contig, begin, end, near, seen, lane, hist };
	lane.c[RNAM_BLOCKS] += gcount_blocks(in.stream, cigar_at, n_cigar, pos, in.ref_length[ref], visit);
	// strand: the read's, inverted for the second mate, against the one gene strand its blocks saw
	const bool read_forward = ((flag & 0x10u) == 0) != (paired && (flag & 0x80u));
	const bool saw_forward = (seen & RNAM_BIT_GENE_FORWARD) != 0, saw_reverse = (seen & RNAM_BIT_GENE_REVERSE) != 0;
	lane.c[RNAM_SENSE_STRAND_RECORDS] += saw_forward != saw_reverse && saw_forward == read_forward ? 1 : 0;
	lane.c[RNAM_ANTISENSE_STRAND_RECORDS] += saw_forward != saw_reverse && saw_forward != read_forward ? 1 : 0;
	lane.c[RNAM_AMBIGUOUS_STRAND_RECORDS] += saw_forward && saw_reverse ? 1 : 0;
	lane.c[RNAM_NO_GENE_RECORDS] += !saw_forward && !saw_reverse ? 1 : 0;
	// insert size: counted once per pair, at its first mate
	if (paired && (flag & 0x40u) && !(flag & 8u) && next_ref == ref && tlen != 0) {
		const int64_t wide = tlen; // (|INT32_MIN| does not fit 32 bits)
		const uint64_t magnitude = (uint64_t) (wide < 0 ? -wide : wide);
		hist.insert(magnitude > 1000 ? 1001u : (uint32_t) magnitude);
		lane.c[RNAM_INSERT_SIZE_PAIRS] += 1;
	}
}

}

#endif
