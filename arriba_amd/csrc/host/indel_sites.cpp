// arriba_amd/csrc/host/indel_sites.cpp -- the host side of --indel-sites (include/arriba_host.h: ahost_indel_sites_*): arriba_amd/csrc/device/indel_core.hpp and allele_core.hpp
// stepped sequentially over records in host memory -- the comparator of agpu_indels.hip, and what --host-ingest and the CPU tier run --, and the text of the file from a row table,
// the host's or the device's.  The steps are the device's: the normalised events of every counting record by (site, shape) (a map here, a sort and runs there), the distinct sites
// of the events with at least min_alt records, their eight counters from the stepping of --allele-counts with min_baseq 0, the percent test.
#include <cstdlib>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include "arriba_host.h"
#include "../device/indel_core.hpp"

namespace arriba {

namespace {
struct EventCounter { // the sink of indel_walk: a map instead of the device's buffer
	std::map<std::pair<uint64_t, uint64_t>, uint32_t>& support;
	void operator()(uint64_t site, uint64_t shape) { ++support[std::make_pair(site, shape)]; }
};
uint32_t max_shift_knob() { // ARRIBA_INDEL_MAX_SHIFT, as agpu_indels.hip reads it
	const char* knob = getenv("ARRIBA_INDEL_MAX_SHIFT");
	uint64_t value = agpu::INDEL_MAX_SHIFT;
	if (knob != nullptr && knob[0] != 0) { value = strtoull(knob, nullptr, 10); if (value < 1) value = 1; }
	return (uint32_t) (value < agpu::INDEL_MAX_SHIFT ? value : agpu::INDEL_MAX_SHIFT);
}
}

void indel_sites_of(const agpu::GenomeView& genome, const std::vector<uint32_t>& tid_to_contig, const std::vector<uint32_t>& ref_length, const uint8_t* records, uint64_t size, uint32_t min_mapq, uint32_t min_alt,
                    uint32_t min_percent, std::vector<agpu_indel_row>& rows, agpu_indel_stats& stats) {
	using namespace agpu;
	memset(&stats, 0, sizeof(stats));
	rows.clear();
	if (min_mapq > 255) throw std::runtime_error("indel sites: a threshold above 255");
	if (min_alt < 1 || min_alt > 0x7FFFFFFFu) throw std::runtime_error("indel sites: min_alt is 1 to 2^31-1");
	if (min_percent > 100) throw std::runtime_error("indel sites: min_percent is 0 to 100");
	if (tid_to_contig.size() != ref_length.size()) throw std::runtime_error("indel sites: the references and their lengths differ in number");
	const uint32_t n_ref = (uint32_t) ref_length.size(), max_shift = max_shift_knob();
	// the events of the records
	std::map<std::pair<uint64_t, uint64_t>, uint32_t> support;
	EventCounter counter = { support };
	for (uint64_t at = 0; at < size; ) {
		uint32_t block_size;
		if (size - at < 36) throw std::runtime_error("failed to load alignments");
		memcpy(&block_size, records + at, 4);
		if ((uint64_t) block_size + 4 > size - at || block_size < 32) throw std::runtime_error("failed to load alignments");
		++stats.records;
		AlleleRecord record;
		if (allele_record(records, at, size, n_ref, min_mapq, record)) {
			++stats.contributing;
			IndelTally tally = { 0, 0, 0, 0 };
			indel_walk(records, record, genome, tid_to_contig[record.ref], ref_length[record.ref], max_shift, true, tally, counter);
			stats.operations += tally.operations; stats.events += tally.events; stats.unkeyed_insertions += tally.unkeyed; stats.shift_capped += tally.capped;
		}
		at += (uint64_t) block_size + 4;
	}
	if (stats.records >= 0xFFFFFFF0ull) throw std::runtime_error("more than 2^32-16 alignment records");
	if (stats.events > INDEL_MAX_EVENTS) throw std::runtime_error("indel sites: more than 2^31 insertions and deletions");
	stats.runs = support.size();
	// the candidate sites, ascending
	std::vector<agpu_allele_site> sites;
	for (std::map<std::pair<uint64_t, uint64_t>, uint32_t>::const_iterator run = support.begin(); run != support.end(); ++run) {
		if (run->second < min_alt) continue;
		++stats.candidates;
		agpu_allele_site site; site.ref = (uint32_t) (run->first.first >> 32); site.pos = (int32_t) (uint32_t) run->first.first;
		if (sites.empty() || sites.back().ref != site.ref || sites.back().pos != site.pos) sites.push_back(site);
	}
	stats.sites = sites.size();
	if (sites.size() > ALLELE_MAX_SITES) throw std::runtime_error("indel sites: more than 2^29-1 candidate sites");
	// their counters: the rows of --allele-counts there, every base whatever its quality
	std::vector<agpu_allele_row> counted; agpu_allele_stats allele_stats;
	allele_counts_of(genome, tid_to_contig, ref_length, sites.data(), sites.size(), records, size, min_mapq, 0, counted, allele_stats);
	size_t slot = 0;
	for (std::map<std::pair<uint64_t, uint64_t>, uint32_t>::const_iterator run = support.begin(); run != support.end(); ++run) {
		if (run->second < min_alt) continue;
		const uint32_t ref = (uint32_t) (run->first.first >> 32), pos = (uint32_t) run->first.first;
		while (slot < sites.size() && (sites[slot].ref != ref || (uint32_t) sites[slot].pos != pos)) ++slot; // (both are ascending)
		if (slot >= sites.size()) throw std::runtime_error("indel sites: internal error: a candidate without its site");
		const agpu_allele_row& from = counted[slot];
		const uint64_t depth = (uint64_t) from.a + from.c + from.g + from.t + from.n + from.del;
		if (!indel_reported(run->second, depth, min_alt, min_percent)) continue;
		agpu_indel_row row;
		memset(&row, 0, sizeof(row));
		row.ref = ref; row.pos = (int32_t) pos; row.bases = indel_shape_bases(run->first.second); row.length = indel_shape_length(run->first.second); row.support = run->second; row.depth = (uint32_t) depth;
		row.type = (uint8_t) indel_shape_type(run->first.second); row.ref_base = from.ref_base;
		rows.push_back(row);
	}
	stats.reported = rows.size();
}

std::string indel_sites_text(const agpu::GenomeView& genome, const std::vector<uint32_t>& tid_to_contig, const ahost_depth_contigs& contigs, const agpu_indel_row* rows, uint64_t n_rows) {
	using namespace agpu;
	std::string text = "#CONTIG\tPOS\tREF\tTYPE\tLENGTH\tBASES\tSUPPORT\tDEPTH\n";
	for (uint64_t r = 0; r < n_rows; ++r) {
		const agpu_indel_row& row = rows[r];
		if (row.ref >= contigs.n_ref || row.ref >= tid_to_contig.size()) throw std::runtime_error("indel sites: a row on a reference the header does not have");
		if (row.type > INDEL_INS || row.length < 1 || (row.type == INDEL_INS && row.length > INDEL_MAX_INSERTION)) throw std::runtime_error("indel sites: a row that is no insertion and no deletion");
		text.append(contigs.names + contigs.name_offset[row.ref], contigs.name_offset[row.ref + 1] - contigs.name_offset[row.ref]);
		text += '\t'; text += std::to_string((uint64_t) (uint32_t) row.pos + 1);
		text += '\t'; text += (char) row.ref_base;
		text += row.type == INDEL_INS ? "\tINS\t" : "\tDEL\t"; text += std::to_string(row.length);
		text += '\t';
		if (row.type == INDEL_INS) for (uint32_t j = 0; j < row.length; ++j) text += "ACGT"[row.bases >> (54 - 2 * j) & 3u];
		else if (row.length <= INDEL_TEXT_DELETION) for (uint32_t j = 1; j <= row.length; ++j) text += (char) allele_ref_base(genome, tid_to_contig[row.ref], (uint32_t) row.pos + j);
		else text += '.';
		text += '\t'; text += std::to_string(row.support);
		text += '\t'; text += std::to_string(row.depth);
		text += '\n';
	}
	return text;
}

}
