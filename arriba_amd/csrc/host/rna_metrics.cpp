// arriba_amd/csrc/host/rna_metrics.cpp -- the host side of --rna-metrics (include/arriba_host.h: ahost_rna_metrics_*): arriba_amd/csrc/device/rnametrics_core.hpp stepped
// sequentially over records in host memory against a region track (region_track.cpp) -- the comparator of agpu_rnametrics.hip, and what --host-ingest and the CPU tier run; and the
// text of the file from a counter block, the host's or the device's.
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#include "arriba_host.h"
#include "../device/rnametrics_core.hpp"

namespace arriba {

namespace {
struct PlainBins { // the three histograms of a counter block, added to directly
	uint64_t* words;
	void mapq(uint32_t q) { ++words[agpu::RNAM_MAPQ_AT + q]; }
	void insert(uint32_t bin) { ++words[agpu::RNAM_INSERT_AT + bin]; }
	void body(uint32_t bin, uint64_t bases) { words[agpu::RNAM_BODY_AT + bin] += bases; }
};
}

void rna_metrics_of(const agpu_region_track& track, const std::vector<uint32_t>& tid_to_contig, const std::vector<uint32_t>& ref_length, const uint8_t* records, uint64_t size, std::vector<uint64_t>& counters,
                    agpu_rna_metrics_stats& stats) {
	using namespace agpu;
	memset(&stats, 0, sizeof(stats));
	counters.assign(RNAM_WORDS, 0);
	if (tid_to_contig.size() != ref_length.size()) throw std::runtime_error("rna metrics: the references and their lengths differ in number");
	uint64_t n = 0;
	for (uint64_t at = 0; at < size; ++n) { // (refused before anything is counted: the device never sees a stream that ends inside a record either)
		uint32_t block_size;
		if (size - at < 36) throw std::runtime_error("failed to load alignments");
		memcpy(&block_size, records + at, 4);
		if ((uint64_t) block_size + 4 > size - at || block_size < 32) throw std::runtime_error("failed to load alignments");
		at += (uint64_t) block_size + 4;
	}
	if (n >= 0xFFFFFFF0ull) throw std::runtime_error("more than 2^32-16 alignment records");
	RnamInput in;
	in.stream = records; in.stream_size = size; in.track = track;
	in.tid_to_contig = tid_to_contig.data(); in.ref_length = ref_length.data(); in.n_ref = (uint32_t) ref_length.size();
	RnamLane lane;
	rnam_clear(lane);
	PlainBins bins = { counters.data() };
	for (uint64_t at = 0; at < size; ) {
		uint32_t block_size;
		memcpy(&block_size, records + at, 4);
		rnam_record(in, at, lane, bins);
		at += (uint64_t) block_size + 4;
	}
	for (int k = 0; k < RNAM_SCALARS; ++k) counters[k] = lane.c[k];
	stats.records = lane.c[RNAM_RECORDS]; stats.base_records = lane.c[RNAM_BASE_RECORDS]; stats.blocks = lane.c[RNAM_BLOCKS]; stats.segments = lane.c[RNAM_SEGMENTS]; stats.track_runs = track.n_runs;
}

// a counter block (AGPU_RNA_METRICS_WORDS words) -> the text of the file
std::string rna_metrics_text(const uint64_t* c) {
	using namespace agpu;
	static const char* const names[RNAM_FILE_SCALARS] = { "RECORDS", "SECONDARY", "SUPPLEMENTARY", "PRIMARY", "UNMAPPED", "MAPPED", "QC_FAIL", "DUPLICATE", "MULTIMAPPING", "PAIRED", "PROPER_PAIR", "READ1", "READ2",
		"MATE_UNMAPPED", "MATE_OTHER_CONTIG", "BASE_RECORDS", "BASES", "SOFT_CLIPPED_BASES", "INSERTED_BASES", "DELETED_BASES", "SKIPPED_BASES", "SPLICED_RECORDS", "ALIGNED_BASES", "RIBOSOMAL_BASES", "CODING_BASES",
		"UTR_BASES", "INTRONIC_BASES", "INTERGENIC_BASES", "UNKNOWN_CONTIG_BASES", "SENSE_STRAND_RECORDS", "ANTISENSE_STRAND_RECORDS", "AMBIGUOUS_STRAND_RECORDS", "NO_GENE_RECORDS", "INSERT_SIZE_PAIRS" };
	std::string text = "## METRICS\n";
	for (int k = 0; k < RNAM_FILE_SCALARS; ++k) { text += names[k]; text += '\t'; text += std::to_string(c[k]); text += '\n'; }
	// the median insert size: the smallest size whose cumulative count reaches ceil(pairs / 2)
	text += "MEDIAN_INSERT_SIZE\t";
	const uint64_t pairs = c[RNAM_INSERT_SIZE_PAIRS];
	if (pairs == 0) text += "NA";
	else {
		const uint64_t half = pairs / 2 + pairs % 2;
		uint64_t sum = 0; uint32_t bin = 0;
		for (; bin < RNAM_INSERT_BINS; ++bin) { sum += c[RNAM_INSERT_AT + bin]; if (sum >= half) break; }
		text += bin >= RNAM_INSERT_BINS - 1 ? std::string(">1000") : std::to_string(bin); // (bins that do not add up to `pairs`: a block that is not the kernel's; the overflow bin says so)
	}
	text += '\n';
	struct Fraction { const char* name; uint64_t numerator, denominator; };
	const Fraction fractions[] = {
		{ "PCT_RIBOSOMAL_BASES", c[RNAM_RIBOSOMAL_BASES], c[RNAM_ALIGNED_BASES] }, { "PCT_CODING_BASES", c[RNAM_CODING_BASES], c[RNAM_ALIGNED_BASES] }, { "PCT_UTR_BASES", c[RNAM_UTR_BASES], c[RNAM_ALIGNED_BASES] },
		{ "PCT_INTRONIC_BASES", c[RNAM_INTRONIC_BASES], c[RNAM_ALIGNED_BASES] }, { "PCT_INTERGENIC_BASES", c[RNAM_INTERGENIC_BASES], c[RNAM_ALIGNED_BASES] },
		{ "PCT_SENSE_STRAND", c[RNAM_SENSE_STRAND_RECORDS], c[RNAM_SENSE_STRAND_RECORDS] + c[RNAM_ANTISENSE_STRAND_RECORDS] }, { "PCT_MAPPED", c[RNAM_MAPPED], c[RNAM_PRIMARY] },
		{ "PCT_DUPLICATE", c[RNAM_DUPLICATE], c[RNAM_MAPPED] }, { "PCT_MULTIMAPPING", c[RNAM_MULTIMAPPING], c[RNAM_MAPPED] } };
	for (size_t f = 0; f < sizeof(fractions) / sizeof(fractions[0]); ++f) {
		text += fractions[f].name; text += '\t';
		if (fractions[f].denominator == 0) text += "NA";
		else { char number[64]; snprintf(number, sizeof(number), "%.6f", (double) fractions[f].numerator / (double) fractions[f].denominator); text += number; }
		text += '\n';
	}
	text += "## MAPQ\n";
	for (uint32_t q = 0; q < RNAM_MAPQ_BINS; ++q) if (c[RNAM_MAPQ_AT + q] != 0) { text += std::to_string(q); text += '\t'; text += std::to_string(c[RNAM_MAPQ_AT + q]); text += '\n'; }
	text += "## INSERT_SIZE\n";
	for (uint32_t bin = 0; bin < RNAM_INSERT_BINS; ++bin) if (c[RNAM_INSERT_AT + bin] != 0) { text += bin == RNAM_INSERT_BINS - 1 ? std::string(">1000") : std::to_string(bin); text += '\t'; text += std::to_string(c[RNAM_INSERT_AT + bin]); text += '\n'; }
	text += "## GENE_BODY\n";
	for (uint32_t bin = 0; bin < RNAM_BODY_BINS; ++bin) { text += std::to_string(bin); text += '\t'; text += std::to_string(c[RNAM_BODY_AT + bin]); text += '\n'; }
	return text;
}

}
