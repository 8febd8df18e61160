// genecount_core.hpp -- --gene-counts: reads per gene of the -x input, the file STAR writes as ReadsPerGene.out.tab and htseq-count -m union gives with -s no / yes / reverse
// (DESIGN.md 4.15 has the rule in full).  What decides a number of the file is here and is shared by the kernels of agpu_genecount.hip and the host stepping of
// arriba_amd/csrc/host/gene_counts.cpp:
//   gcount_nh          the NH of a record: the first aux field of that name if it has an integer type (bam_aux2i), else 1; the walk rule is scan_aux's of ingest_core.hpp
//   gcount_blocks      the blocks of an end: maximal runs of reference positions under M, = and X, cut to the contig; D and N advance without covering (htseq-count's rule, not
//                      the one of depth_core.hpp), I, S, H and P do neither: visit(s, e), 0-based inclusive, per block
//   gcount_fold        one block through the exon index into a three-column state: per column the first gene seen and how many different ones, saturating at 2 -- all in
//                      registers; folding a gene twice changes nothing, so exons repeated across buckets and transcripts are harmless
//   gcount_outcome     the row of a column: N_noFeature, the one gene, N_ambiguous
//   gcount_template    the two claimed ends of a template -> its row in each of the three columns
// Names, slots and claims are those of markdup_core.hpp.  Records are as sbam_parse reads them.
#ifndef AGPU_GENECOUNT_CORE_HPP
#define AGPU_GENECOUNT_CORE_HPP 1

#include "annotate_core.hpp"
#include "markdup_core.hpp"

namespace agpu {

// counts[c * (n_genes + GCOUNT_SPECIAL) + row], c < GCOUNT_COLUMNS: the four special rows in the order of the file, then the genes in table order
enum { GCOUNT_UNMAPPED = 0, GCOUNT_MULTIMAPPING = 1, GCOUNT_NO_FEATURE = 2, GCOUNT_AMBIGUOUS = 3, GCOUNT_SPECIAL = 4, GCOUNT_COLUMNS = 3 };

// Nothing outside the record is read.  aux: where the optional fields begin, end: where the record ends (offsets in the stream)
AGPU_HD int64_t gcount_nh(const uint8_t* stream, uint64_t aux, uint64_t end) {
	uint64_t s = aux;
	while (s + 3 <= end) {
		const uint64_t value = s + 2;
		const uint8_t type = stream[value];
		uint64_t size;
		switch (type) {
			case 'A': case 'c': case 'C': size = 2; break;
			case 's': case 'S': size = 3; break;
			case 'i': case 'I': case 'f': size = 5; break;
			case 'd': size = 9; break;
			case 'Z': case 'H': { uint64_t p = value + 1; while (p < end && stream[p]) ++p; if (p >= end) return 1; size = p - value + 1; break; }
			case 'B': {
				if (value + 6 > end) return 1;
				const uint8_t of = stream[value + 1];
				const uint64_t element = (of == 'c' || of == 'C') ? 1 : (of == 's' || of == 'S') ? 2 : 4;
				size = 6 + element * (uint64_t) sbam_load32(stream, value + 2);
				break;
			}
			default: return 1;
		}
		if (value + size > end) return 1;
		if (stream[s] == 'N' && stream[s + 1] == 'H') {
			switch (type) { // bam_aux2i
				case 'c': return (int8_t) stream[value + 1];
				case 'C': return stream[value + 1];
				case 's': return (int16_t) sbam_load16(stream, value + 1);
				case 'S': return sbam_load16(stream, value + 1);
				case 'i': return (int32_t) sbam_load32(stream, value + 1);
				case 'I': return sbam_load32(stream, value + 1);
				default: return 1;
			}
		}
		s = value + size;
	}
	return 1;
}

// visit(s, e) for every block [s, e] of the CIGAR walked from pos on a contig of `length` bases, 0 <= s <= e < length; returns their number.  Runs that touch are one block.
template <class Visit> AGPU_HD uint32_t gcount_blocks(const uint8_t* stream, uint64_t cigar_at, uint32_t n_cigar, int32_t pos, uint32_t length, Visit& visit) {
	int64_t at = pos, open_begin = 0, open_end = 0; // the block that is not visited yet: empty while open_begin == open_end
	uint32_t blocks = 0;
	for (uint32_t k = 0; k < n_cigar; ++k) {
		const uint32_t word = sbam_load32(stream, cigar_at + 4ull * k), op = word & 15u;
		const int64_t span = word >> 4;
		if ((0x181u >> op) & 1u) { // M (0), = (7), X (8)
			const int64_t begin = at < 0 ? 0 : at, end = at + span < (int64_t) length ? at + span : (int64_t) length;
			if (begin < end) {
				if (open_begin < open_end && begin == open_end) open_end = end;
				else {
					if (open_begin < open_end) { visit((int32_t) open_begin, (int32_t) (open_end - 1)); ++blocks; }
					open_begin = begin; open_end = end;
				}
			}
			at += span;
		} else if (op == 2 || op == 3) at += span; // D, N
	}
	if (open_begin < open_end) { visit((int32_t) open_begin, (int32_t) (open_end - 1)); ++blocks; }
	return blocks;
}

// per column c (0: unstranded, 1: read strand = gene strand, 2: read strand != gene strand) the first gene and the number of different genes, which stops at 2
struct GcountState { uint32_t first[GCOUNT_COLUMNS]; uint32_t n[GCOUNT_COLUMNS]; };
AGPU_HD void gcount_clear(GcountState& state) { AGPU_UNROLL for (int c = 0; c < GCOUNT_COLUMNS; ++c) { state.first[c] = 0; state.n[c] = 0; } }
AGPU_HD void gcount_add(uint32_t& first, uint32_t& n, uint32_t gene) {
	if (n == 0) { first = gene; n = 1; }
	else if (first != gene) n = 2;
}

// The genes < n_genes that own an exon on `contig` which overlaps [s, e], into the columns their strand admits for an end of strand `forward`.  Bucket k of the index holds the
// exons that cover (keys[k - 1], keys[k]]: the first bucket is the one of the first key >= s, the last the one of the first key >= e.  hint (in/out): a key near s.
AGPU_HD void gcount_fold(const AnnotationView& ann, uint32_t contig, int32_t s, int32_t e, bool forward, uint32_t& hint, GcountState& state) {
	const FlatIndexView& index = ann.exon_index;
	if (contig >= index.n_contigs) return;
	const uint32_t contig_end = index.contig_offset[contig + 1];
	uint32_t k = index_lower_bound_near(index, contig, s, hint);
	hint = k;
	for (; k != contig_end; ++k) {
		const uint32_t begin = index.member_offset[k], end = index.member_offset[k + 1];
		for (uint32_t m = begin; m < end; ++m) {
			const uint32_t gene = ann.exon_gene[index.members[m]];
			if (gene >= ann.n_genes) continue;
			const bool gene_forward = (ann.gene_bits[gene] & GBIT_STRAND) != 0;
			gcount_add(state.first[0], state.n[0], gene);
			if (gene_forward == forward) gcount_add(state.first[1], state.n[1], gene);
			else gcount_add(state.first[2], state.n[2], gene);
		}
		if (index.keys[k] >= e) break;
	}
}

AGPU_HD uint32_t gcount_outcome(uint32_t first, uint32_t n) { return n == 0 ? (uint32_t) GCOUNT_NO_FEATURE : n == 1 ? (uint32_t) GCOUNT_SPECIAL + first : (uint32_t) GCOUNT_AMBIGUOUS; }

// what a template is counted against: the stream, the claims, the annotation, the references of the header
struct GcountInput {
	const uint8_t* stream; uint64_t stream_size;
	const uint64_t* record_offset;
	AnnotationView ann;
	const uint32_t* tid_to_contig; // [n_ref] reference id -> contig of the session
	const uint32_t* ref_length;    // [n_ref] LN
	uint32_t n_ref;
};
struct GcountTemplate { bool counted; uint32_t row[GCOUNT_COLUMNS]; uint32_t ends, blocks; }; // counted: it has a primary record; ends: its mapped ends; blocks: of a template of class `counted`

struct GcountFold {
	const AnnotationView& ann; uint32_t contig; bool forward; uint32_t& hint; GcountState& state;
	AGPU_HD void operator()(int32_t s, int32_t e) { gcount_fold(ann, contig, s, e, forward, hint, state); }
};

// first0, first1: the records that claimed the slots of the template (MDUP_NONE: nobody did).  A claimed record holds its 36 fixed bytes inside the stream (the name pass saw to it).
AGPU_HD GcountTemplate gcount_template(const GcountInput& in, uint32_t first0, uint32_t first1) {
	GcountTemplate out;
	out.counted = first0 != MDUP_NONE || first1 != MDUP_NONE; out.ends = 0; out.blocks = 0;
	AGPU_UNROLL for (int c = 0; c < GCOUNT_COLUMNS; ++c) out.row[c] = GCOUNT_UNMAPPED;
	if (!out.counted) return out;
	bool multimapping = false;
	AGPU_UNROLL for (int slot = 0; slot < 2; ++slot) {
		const uint32_t r = slot == 0 ? first0 : first1;
		if (r == MDUP_NONE) continue;
		const uint64_t at = in.record_offset[r];
		uint64_t size = (uint64_t) sbam_load32(in.stream, at) + 4;
		if (size > in.stream_size - at) size = in.stream_size - at;
		const int32_t ref = (int32_t) sbam_load32(in.stream, at + 4);
		const uint32_t flag = sbam_load16(in.stream, at + 18);
		if (!mdup_mapped(flag, ref)) continue;
		++out.ends;
		const uint64_t l_seq = sbam_load32(in.stream, at + 20);
		const uint64_t aux = 36ull + in.stream[at + 12] + 4ull * sbam_load16(in.stream, at + 16) + (l_seq + 1) / 2 + l_seq;
		if (aux < size && gcount_nh(in.stream, at + aux, at + size) > 1) multimapping = true;
	}
	if (out.ends == 0) return out;
	if (multimapping) { AGPU_UNROLL for (int c = 0; c < GCOUNT_COLUMNS; ++c) out.row[c] = GCOUNT_MULTIMAPPING; return out; }
	GcountState state;
	gcount_clear(state);
	uint32_t hint = NO_HINT;
	AGPU_UNROLL for (int slot = 0; slot < 2; ++slot) {
		const uint32_t r = slot == 0 ? first0 : first1;
		if (r == MDUP_NONE) continue;
		const uint64_t at = in.record_offset[r];
		uint64_t size = (uint64_t) sbam_load32(in.stream, at) + 4;
		if (size > in.stream_size - at) size = in.stream_size - at;
		const int32_t ref = (int32_t) sbam_load32(in.stream, at + 4), pos = (int32_t) sbam_load32(in.stream, at + 8);
		const uint32_t flag = sbam_load16(in.stream, at + 18), l_read_name = in.stream[at + 12];
		if (!mdup_mapped(flag, ref) || pos < 0 || (uint32_t) ref >= in.n_ref) continue;
		uint32_t n_cigar = sbam_load16(in.stream, at + 16);
		if (36ull + l_read_name + 4ull * n_cigar > size) n_cigar = 0;
		const bool forward = ((flag & 0x10u) == 0) != (slot == 1); // (the second mate reads the other strand of the fragment)
		GcountFold fold = { in.ann, in.tid_to_contig[ref], forward, hint, state };
		out.blocks += gcount_blocks(in.stream, at + 36 + l_read_name, n_cigar, pos, in.ref_length[ref], fold);
	}
	AGPU_UNROLL for (int c = 0; c < GCOUNT_COLUMNS; ++c) out.row[c] = gcount_outcome(state.first[c], state.n[c]);
	return out;
}

}

#endif
