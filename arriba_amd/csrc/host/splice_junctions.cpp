// arriba_amd/csrc/host/splice_junctions.cpp -- the host side of --splice-junctions (include/arriba_host.h: ahost_splice_junctions_*): arriba_amd/csrc/device/junction_core.hpp
// stepped sequentially over records in host memory against the annotation and the assembly of a session -- the comparator of agpu_junctions.hip, and what --host-ingest and the CPU
// tier run.  The steps are the device's: the kept introns of every contributing record, read names into the table of markdup_core.hpp, the crossings ordered by their two key words
// (std::sort), the heads of the (junction, template) and of the junction runs, the table of annotated introns, the class of every row; and the text of the file:
// NAME, s + 1, e + 1, strand, motif, annotated, unique, multimapping, overhang, tab-separated, a line per row.
#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include "arriba_host.h"
#include "../device/junction_core.hpp"

namespace arriba {

namespace {
struct Crossing { uint64_t high, low; uint32_t overhang; };
struct Collect {
	std::vector<Crossing>& out; uint32_t ref, name; bool multimapping;
	void operator()(int32_t s, int32_t e, uint32_t least) { Crossing c = { agpu::junc_key_high(ref, s), agpu::junc_key_low(e, name, multimapping), least }; out.push_back(c); }
};
struct Nothing { void operator()(int32_t, int32_t, uint32_t) {} };
struct Intron { uint64_t high, low; uint32_t mask; };
}

void splice_junctions_of(const JunctionReferences& references, const std::vector<uint32_t>& tid_to_contig, const std::vector<uint32_t>& ref_length, const uint8_t* records, uint64_t size, std::vector<agpu_junction_row>& rows,
                         agpu_junction_stats& stats) {
	using namespace agpu;
	memset(&stats, 0, sizeof(stats));
	rows.clear();
	if (tid_to_contig.size() != ref_length.size()) throw std::runtime_error("splice junctions: the references and their lengths differ in number");
	std::vector<uint64_t> offset;
	for (uint64_t at = 0; at < size; ) {
		uint32_t block_size;
		if (size - at < 36) throw std::runtime_error("failed to load alignments");
		memcpy(&block_size, records + at, 4);
		if ((uint64_t) block_size + 4 > size - at || block_size < 32) throw std::runtime_error("failed to load alignments");
		offset.push_back(at);
		at += (uint64_t) block_size + 4;
	}
	const uint64_t n = offset.size();
	if (n >= 0xFFFFFFF0ull) throw std::runtime_error("more than 2^32-16 alignment records");
	stats.records = n;
	const uint32_t n_ref = (uint32_t) ref_length.size();
	// count
	uint64_t total = 0;
	for (uint64_t r = 0; r < n; ++r) {
		JuncRecord record;
		if (!junc_record(records, size, offset.data(), r, n_ref, record)) continue;
		++stats.contributing;
		Nothing nothing;
		total += junc_walk(records, record.cigar_at, record.n_cigar, record.pos, ref_length[record.ref], nothing);
	}
	stats.crossings = total;
	if (total == 0) return;
	if (total >= 0xFFFFFFF0ull) throw std::runtime_error("more than 2^32-16 crossings of splice junctions");
	// name ids and the crossings
	const uint64_t slots = support_table_slots(n);
	std::vector<unsigned long long> table(slots, 0);
	std::vector<Crossing> crossings;
	crossings.reserve(total);
	for (uint64_t r = 0; r < n; ++r) {
		uint32_t id = mdup_name_insert(table.data(), slots, records, size, offset.data(), (uint32_t) r, 64);
		if (id == MDUP_NONE) id = (uint32_t) r;
		JuncRecord record;
		if (!junc_record(records, size, offset.data(), r, n_ref, record)) continue;
		Collect collect = { crossings, record.ref, id, record.multimapping };
		junc_walk(records, record.cigar_at, record.n_cigar, record.pos, ref_length[record.ref], collect);
	}
	if (crossings.size() != total) throw std::runtime_error("splice junctions: the two walks differ");
	std::sort(crossings.begin(), crossings.end(), [](const Crossing& a, const Crossing& b) { return a.high != b.high ? a.high < b.high : a.low < b.low; });
	// heads of runs
	for (uint64_t i = 0; i < total; ++i) {
		const Crossing& c = crossings[i];
		const bool junction_head = i == 0 || !junc_same_junction(c.high, c.low, crossings[i - 1].high, crossings[i - 1].low);
		const bool pair_head = i == 0 || !junc_same_pair(c.high, c.low, crossings[i - 1].high, crossings[i - 1].low);
		if (junction_head) {
			agpu_junction_row row;
			memset(&row, 0, sizeof(row));
			row.ref = junc_key_ref(c.high); row.start = junc_key_s(c.high); row.end = junc_key_e(c.low);
			rows.push_back(row);
		}
		agpu_junction_row& row = rows.back();
		if (pair_head) { ++stats.pairs; if (junc_key_multimapping(c.low)) ++row.multimapping; else ++row.unique; }
		row.overhang = std::max(row.overhang, c.overhang);
	}
	// the annotated introns
	const AnnotationView& ann = references.view;
	std::vector<Intron> made(ann.n_exons);
	for (uint32_t x = 0; x < ann.n_exons; ++x) made[x].high = junc_intron_key_high(ann, x, made[x].low, made[x].mask);
	std::sort(made.begin(), made.end(), [](const Intron& a, const Intron& b) { return a.high != b.high ? a.high < b.high : a.low < b.low; });
	std::vector<uint64_t> intron_high(made.size()), intron_low(made.size()); std::vector<uint32_t> intron_mask(made.size());
	for (size_t k = 0; k < made.size(); ++k) { intron_high[k] = made[k].high; intron_low[k] = made[k].low; intron_mask[k] = made[k].mask; }
	const JuncIntrons introns = { intron_high.data(), intron_low.data(), intron_mask.data(), made.size() };
	// classes
	for (size_t j = 0; j < rows.size(); ++j) {
		agpu_junction_row& row = rows[j];
		const uint32_t contig = tid_to_contig[row.ref];
		const uint32_t motif = junc_motif(references.genome, contig, row.start, row.end), seen = junc_annotated(introns, contig, row.start, row.end);
		row.motif = (uint8_t) motif; row.annotated = seen != 0 ? 1 : 0; row.strand = (uint8_t) junc_strand(motif, seen);
		stats.annotated += row.annotated;
	}
	stats.junctions = rows.size();
}

std::string splice_junctions_text(const ahost_depth_contigs& contigs, const agpu_junction_row* rows, uint64_t n_rows) {
	std::string text;
	for (uint64_t j = 0; j < n_rows; ++j) {
		const agpu_junction_row& row = rows[j];
		if (row.ref >= contigs.n_ref) throw std::runtime_error("splice junctions: a row on a reference the header does not have");
		text.append(contigs.names + contigs.name_offset[row.ref], contigs.name_offset[row.ref + 1] - contigs.name_offset[row.ref]);
		const uint64_t fields[8] = { (uint64_t) row.start + 1, (uint64_t) row.end + 1, row.strand, row.motif, row.annotated, row.unique, row.multimapping, row.overhang };
		for (int f = 0; f < 8; ++f) { text += '\t'; text += std::to_string(fields[f]); }
		text += '\n';
	}
	return text;
}

}
