// arriba_amd/csrc/host/gene_counts.cpp -- the host side of --gene-counts (include/arriba_host.h: ahost_gene_counts_*): arriba_amd/csrc/device/genecount_core.hpp stepped
// sequentially over records in host memory against the annotation of a session -- the comparator of agpu_genecount.hip, and what --host-ingest and the CPU tier run.  The steps
// are the device's: read names into the table of markdup_core.hpp, the first primary record of every slot, the row of every template in the three columns; and
// the text of the file: N_unmapped, N_multimapping, N_noFeature, N_ambiguous, then a line per gene of the table.
#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#include "arriba_host.h"
#include "../device/genecount_core.hpp"

namespace arriba {

void gene_counts_of(const GeneCountAnnotation& annotation, const std::vector<uint32_t>& tid_to_contig, const std::vector<uint32_t>& ref_length, const uint8_t* records, uint64_t size, std::vector<uint64_t>& counts,
                    agpu_gene_count_stats& stats) {
	using namespace agpu;
	memset(&stats, 0, sizeof(stats));
	const uint64_t stride = (uint64_t) annotation.view.n_genes + GCOUNT_SPECIAL;
	counts.assign(GCOUNT_COLUMNS * stride, 0);
	if (tid_to_contig.size() != ref_length.size()) throw std::runtime_error("gene counts: the references and their lengths differ in number");
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
	if (n == 0) return;
	// name ids and claims
	const uint64_t slots = support_table_slots(n);
	std::vector<unsigned long long> table(slots, 0);
	std::vector<uint32_t> name_id(n), slot_first(2 * n, MDUP_NONE);
	for (uint64_t r = 0; r < n; ++r) {
		const uint32_t id = name_id[r] = mdup_name_insert(table.data(), slots, records, size, offset.data(), (uint32_t) r, 64);
		const uint32_t flags = sbam_load16(records, offset[r] + 18);
		if (id != MDUP_NONE && mdup_primary(flags)) { uint32_t& first = slot_first[2ull * id + mdup_slot(flags)]; first = std::min(first, (uint32_t) r); }
	}
	// the rows
	GcountInput in;
	in.stream = records; in.stream_size = size; in.record_offset = offset.data(); in.ann = annotation.view;
	in.tid_to_contig = tid_to_contig.data(); in.ref_length = ref_length.data(); in.n_ref = (uint32_t) ref_length.size();
	for (uint64_t t = 0; t < n; ++t) {
		if (name_id[t] != t) continue;
		++stats.templates;
		const GcountTemplate result = gcount_template(in, slot_first[2 * t], slot_first[2 * t + 1]);
		if (!result.counted) { ++stats.without_primary; continue; }
		stats.ends += result.ends; stats.blocks += result.blocks;
		for (int c = 0; c < GCOUNT_COLUMNS; ++c) {
			if (result.row[c] >= stride) throw std::runtime_error("gene counts: a row beyond the table");
			++counts[c * stride + result.row[c]];
		}
	}
}

std::string gene_counts_text(const std::vector<std::string>& gene_ids, const uint64_t* counts) {
	using namespace agpu;
	static const char* const special[GCOUNT_SPECIAL] = { "N_unmapped", "N_multimapping", "N_noFeature", "N_ambiguous" };
	const uint64_t stride = gene_ids.size() + GCOUNT_SPECIAL;
	std::string text;
	for (uint64_t row = 0; row < stride; ++row) {
		text += row < GCOUNT_SPECIAL ? std::string(special[row]) : gene_ids[row - GCOUNT_SPECIAL];
		for (int c = 0; c < GCOUNT_COLUMNS; ++c) { text += '\t'; text += std::to_string(counts[c * stride + row]); }
		text += '\n';
	}
	return text;
}

}
