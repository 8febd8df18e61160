// arriba_amd/csrc/host/variant_sites.cpp -- the host side of --variant-sites (include/arriba_host.h: ahost_variant_sites_*): arriba_amd/csrc/device/variant_core.hpp and
// allele_core.hpp stepped sequentially over records in host memory -- the comparator of agpu_variants.hip, and what --host-ingest and the CPU tier run --, and the text of the file
// from a row table, the host's or the device's.  The steps are the device's: the mismatch events of every counting record by key (a map here, a sort and runs there), the sites
// with an alt of at least min_alt events, their eight counters from the stepping of --allele-counts, the percent test and the check of every support against its counter
// (DESIGN.md 4.21).
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>
#include "arriba_host.h"
#include "../device/variant_core.hpp"

namespace arriba {

void variant_sites_of(const agpu::GenomeView& genome, const std::vector<uint32_t>& tid_to_contig, const std::vector<uint32_t>& ref_length, const uint8_t* records, uint64_t size, uint32_t min_mapq, uint32_t min_baseq,
                      uint32_t min_alt, uint32_t min_percent, std::vector<agpu_variant_row>& rows, agpu_variant_stats& stats) {
	using namespace agpu;
	memset(&stats, 0, sizeof(stats));
	rows.clear();
	if (min_mapq > 255 || min_baseq > 255) throw std::runtime_error("variant sites: a threshold above 255");
	if (min_alt < 1 || min_alt > 0x7FFFFFFFu) throw std::runtime_error("variant sites: min_alt is 1 to 2^31-1");
	if (min_percent > 100) throw std::runtime_error("variant sites: min_percent is 0 to 100");
	if (tid_to_contig.size() != ref_length.size()) throw std::runtime_error("variant sites: the references and their lengths differ in number");
	if (ref_length.size() >= VARIANT_MAX_REFERENCES) throw std::runtime_error("variant sites: 2^30 references or more");
	const uint32_t n_ref = (uint32_t) ref_length.size();
	// the events of the records by key
	std::map<uint64_t, uint32_t> support;
	for (uint64_t at = 0; at < size; ) {
		uint32_t block_size;
		if (size - at < 36) throw std::runtime_error("failed to load alignments");
		memcpy(&block_size, records + at, 4);
		if ((uint64_t) block_size + 4 > size - at || block_size < 32) throw std::runtime_error("failed to load alignments");
		++stats.records;
		AlleleRecord record;
		if (allele_record(records, at, size, n_ref, min_mapq, record)) {
			++stats.contributing;
			const uint32_t length = ref_length[record.ref], contig = tid_to_contig[record.ref];
			int64_t position = record.pos; uint64_t read_index = 0;
			for (uint32_t k = 0; k < record.n_cigar; ++k) {
				const uint32_t word = sbam_load32(records, record.cigar_at + 4ull * k), op = word & 15u;
				const int64_t span = word >> 4;
				if (op == 0 || op == 7 || op == 8) { // M, =, X
					const int64_t lo = position < 0 ? -position : 0, hi = position + span < (int64_t) length ? span : (int64_t) length - position;
					for (int64_t j = lo; j < hi; ++j) {
						const uint32_t alt = variant_base_event(records, record, genome, contig, length, position, read_index, (uint64_t) j, min_baseq);
						if (alt != VARIANT_NO_EVENT) { ++support[variant_key(record.ref, (uint32_t) (position + j), alt)]; ++stats.events; }
					}
					position += span; read_index += (uint64_t) span;
				}
				else if (op == 2 || op == 3) position += span;
				else if (op == 1 || op == 4) read_index += (uint64_t) span;
			}
		}
		at += (uint64_t) block_size + 4;
	}
	if (stats.records >= 0xFFFFFFF0ull) throw std::runtime_error("more than 2^32-16 alignment records");
	if (stats.events > VARIANT_MAX_EVENTS) throw std::runtime_error("variant sites: more than 2^31 bases differ from the assembly: the assembly of -a hardly matches the sample");
	stats.runs = support.size();
	// the candidate sites, ascending
	std::vector<agpu_allele_site> candidates;
	for (std::map<uint64_t, uint32_t>::const_iterator run = support.begin(); run != support.end(); ++run) {
		if (run->second < min_alt) continue;
		const uint64_t site = variant_key_site(run->first);
		agpu_allele_site candidate; candidate.ref = (uint32_t) (site >> 32); candidate.pos = (int32_t) (uint32_t) site;
		if (candidates.empty() || candidates.back().ref != candidate.ref || candidates.back().pos != candidate.pos) candidates.push_back(candidate);
	}
	stats.candidates = candidates.size();
	if (candidates.size() > ALLELE_MAX_SITES) throw std::runtime_error("variant sites: more than 2^29-1 candidate sites: the assembly of -a hardly matches the sample");
	// their counters: the rows of --allele-counts there
	std::vector<agpu_allele_row> counted; agpu_allele_stats allele_stats;
	allele_counts_of(genome, tid_to_contig, ref_length, candidates.data(), candidates.size(), records, size, min_mapq, min_baseq, counted, allele_stats);
	for (size_t c = 0; c < candidates.size(); ++c) {
		const agpu_allele_row& from = counted[c];
		const uint32_t counts[ALLELE_COLUMNS] = { from.a, from.c, from.g, from.t, from.n, from.del, from.skip, from.lowq };
		uint32_t of_alt[4] = { 0, 0, 0, 0 };
		const uint64_t site = allele_key(candidates[c].ref, (uint32_t) candidates[c].pos);
		for (std::map<uint64_t, uint32_t>::const_iterator run = support.lower_bound(site << 2); run != support.end() && variant_key_site(run->first) == site; ++run) of_alt[variant_key_alt(run->first)] = run->second;
		bool consistent = true;
		const uint32_t mask = variant_row_mask(counts, of_alt, from.ref_base, min_alt, min_percent, consistent);
		if (!consistent) ++stats.inconsistent;
		if (mask == 0) continue;
		agpu_variant_row row;
		row.ref = candidates[c].ref; row.pos = candidates[c].pos;
		row.a = from.a; row.c = from.c; row.g = from.g; row.t = from.t; row.n = from.n; row.del = from.del; row.skip = from.skip; row.lowq = from.lowq;
		row.ref_base = from.ref_base; row.alt_mask = (uint8_t) mask; row.reserved[0] = row.reserved[1] = 0;
		rows.push_back(row);
	}
	stats.reported = rows.size();
	if (stats.inconsistent != 0) throw std::runtime_error("variant sites: internal error: the events of " + std::to_string(stats.inconsistent) + " candidate sites disagree with their counters");
}

std::string variant_sites_text(const ahost_depth_contigs& contigs, const agpu_variant_row* rows, uint64_t n_rows) {
	std::string text = "#CONTIG\tPOS\tREF\tALT\tA\tC\tG\tT\tN\tDEL\tSKIP\tLOWQ\n";
	for (uint64_t r = 0; r < n_rows; ++r) {
		const agpu_variant_row& row = rows[r];
		if (row.ref >= contigs.n_ref) throw std::runtime_error("variant sites: a row on a reference the header does not have");
		if ((row.alt_mask & 15u) == 0) throw std::runtime_error("variant sites: a row without a reported alt");
		text.append(contigs.names + contigs.name_offset[row.ref], contigs.name_offset[row.ref + 1] - contigs.name_offset[row.ref]);
		text += '\t'; text += std::to_string((uint64_t) (uint32_t) row.pos + 1);
		text += '\t'; text += (char) row.ref_base;
		text += '\t';
		bool further = false;
		for (uint32_t alt = 0; alt < 4; ++alt) if (row.alt_mask >> alt & 1u) { if (further) text += ','; text += "ACGT"[alt]; further = true; }
		const uint32_t fields[8] = { row.a, row.c, row.g, row.t, row.n, row.del, row.skip, row.lowq };
		for (int f = 0; f < 8; ++f) { text += '\t'; text += std::to_string(fields[f]); }
		text += '\n';
	}
	return text;
}

}
