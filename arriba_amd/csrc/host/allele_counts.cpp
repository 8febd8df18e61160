// arriba_amd/csrc/host/allele_counts.cpp -- the host side of --allele-counts (include/arriba_host.h: ahost_allele_*): the reader of the sites file, which places every line on the
// references of a header; arriba_amd/csrc/device/allele_core.hpp stepped sequentially over records in host memory -- the comparator of agpu_alleles.hip, and what --host-ingest
// and the CPU tier run --; and the text of the file from a row table, the host's or the device's.  The steps are the device's: the placed sites sorted by key with their lines, the
// window bitmap, the filter and the walk of every record, one add per (site slot, column), the rows in the order of the lines with REF from the assembly.
#include <algorithm>
#include <cstring>
#include <cstdio>
#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include "arriba_host.h"
#include "../device/allele_core.hpp"

namespace arriba {

void AlleleSiteList::place(const uint8_t* header, size_t header_size) {
	std::vector<std::string> references; std::vector<uint32_t> lengths;
	if (header != nullptr && header_size > 0) header_contigs(header, header_size, references, lengths);
	std::map<std::string, uint32_t> index_of; // (the first reference of a name)
	for (size_t t = 0; t < references.size(); ++t) index_of.insert(std::make_pair(references[t], (uint32_t) t));
	placed = 0;
	for (size_t line = 0; line < sites.size(); ++line) {
		const std::string name = names.substr(name_offset[line], name_offset[line + 1] - name_offset[line]);
		std::map<std::string, uint32_t>::const_iterator found = index_of.find(name); // byte for byte ...
		if (found == index_of.end()) found = index_of.find(name.compare(0, 3, "chr") == 0 ? name.substr(3) : "chr" + name); // ... and once more with a leading chr removed or added
		sites[line].ref = agpu::ALLELE_UNPLACED;
		if (found != index_of.end() && (uint32_t) sites[line].pos < lengths[found->second]) { sites[line].ref = found->second; ++placed; }
	}
}

// the lines of a sites file: contig and 1-based position, cut at tabs; every line unplaced
void allele_sites_parse(const std::string& path, AlleleSiteList& list) {
	list = AlleleSiteList();
	std::string text;
	{ FILE* file = fopen(path.c_str(), "rb");
	  if (file == nullptr) throw std::runtime_error("--allele-sites: cannot read '" + path + "'");
	  char piece[1 << 16];
	  for (size_t got; (got = fread(piece, 1, sizeof(piece), file)) > 0; ) text.append(piece, got);
	  const bool failed = ferror(file) != 0; // (a directory opens and then fails to read)
	  fclose(file);
	  if (failed) throw std::runtime_error("--allele-sites: cannot read '" + path + "'"); }
	list.name_offset.push_back(0);
	uint64_t number = 0;
	for (size_t at = 0; at < text.size(); ) {
		size_t end = text.find('\n', at);
		if (end == std::string::npos) end = text.size();
		++number;
		const size_t begin = at;
		at = end + 1;
		if (end == begin || text[begin] == '#') continue;
		const std::string where = "--allele-sites: '" + path + "' line " + std::to_string(number) + ": ";
		const size_t tab = text.find('\t', begin);
		if (tab == std::string::npos || tab >= end) throw std::runtime_error(where + "fewer than two fields (contig and 1-based position, separated by a tab)");
		size_t stop = text.find('\t', tab + 1);
		if (stop == std::string::npos || stop > end) stop = end;
		if (stop == tab + 1) throw std::runtime_error(where + "the position is empty");
		uint64_t position = 0;
		for (size_t k = tab + 1; k < stop; ++k) {
			if (text[k] < '0' || text[k] > '9') throw std::runtime_error(where + "the position holds something that is not a digit");
			if (position <= 0x7FFFFFFFull) position = position * 10 + (uint64_t) (text[k] - '0');
		}
		if (position == 0 || position > 0x7FFFFFFFull) throw std::runtime_error(where + "the position is 0 or above 2^31-1");
		agpu_allele_site site; site.ref = agpu::ALLELE_UNPLACED; site.pos = (int32_t) (position - 1);
		list.sites.push_back(site);
		list.names.append(text, begin, tab - begin);
		list.name_offset.push_back(list.names.size());
	}
	if (list.sites.size() > agpu::ALLELE_MAX_SITES) throw std::runtime_error("--allele-sites: '" + path + "' has more than 2^29-1 sites");
}

void allele_counts_of(const agpu::GenomeView& genome, const std::vector<uint32_t>& tid_to_contig, const std::vector<uint32_t>& ref_length, const agpu_allele_site* sites, uint64_t n_sites, const uint8_t* records, uint64_t size,
                      uint32_t min_mapq, uint32_t min_baseq, std::vector<agpu_allele_row>& rows, agpu_allele_stats& stats) {
	using namespace agpu;
	memset(&stats, 0, sizeof(stats));
	rows.assign(n_sites, agpu_allele_row());
	if (min_mapq > 255 || min_baseq > 255) throw std::runtime_error("allele counts: a threshold above 255");
	if (n_sites > ALLELE_MAX_SITES) throw std::runtime_error("allele counts: more than 2^29-1 sites");
	if (tid_to_contig.size() != ref_length.size()) throw std::runtime_error("allele counts: the references and their lengths differ in number");
	const uint32_t n_ref = (uint32_t) ref_length.size();
	// the placed sites by key, each with its line
	std::vector<std::pair<uint64_t, uint32_t> > order;
	for (uint64_t line = 0; line < n_sites; ++line) {
		const agpu_allele_site& site = sites[line];
		if (site.ref == ALLELE_UNPLACED) continue;
		if (site.ref >= n_ref || site.pos < 0 || (uint32_t) site.pos >= ref_length[site.ref]) throw std::runtime_error("allele counts: site " + std::to_string(line) + " lies on no reference of the header or beyond its length");
		order.push_back(std::make_pair(allele_key(site.ref, (uint32_t) site.pos), (uint32_t) line));
	}
	std::stable_sort(order.begin(), order.end(), [](const std::pair<uint64_t, uint32_t>& a, const std::pair<uint64_t, uint32_t>& b) { return a.first < b.first; });
	const uint64_t placed = order.size();
	std::vector<uint64_t> keys(placed), window_offset((size_t) n_ref + 1, 0);
	for (uint64_t k = 0; k < placed; ++k) keys[k] = order[k].first;
	for (uint32_t t = 0; t < n_ref; ++t) window_offset[t + 1] = window_offset[t] + allele_windows_of(ref_length[t]);
	std::vector<uint32_t> bitmap(window_offset[n_ref] / 32 + 1, 0);
	for (uint64_t k = 0; k < placed; ++k) { const uint64_t window = allele_window(window_offset.data(), (uint32_t) (keys[k] >> 32), (uint32_t) keys[k]); bitmap[window >> 5] |= 1u << (window & 31u); }
	const AlleleSites view = { keys.data(), placed, bitmap.data(), window_offset.data() };
	// the records
	std::vector<uint32_t> counts(placed * ALLELE_COLUMNS, 0);
	for (uint64_t at = 0; at < size; ) {
		uint32_t block_size;
		if (size - at < 36) throw std::runtime_error("failed to load alignments");
		memcpy(&block_size, records + at, 4);
		if ((uint64_t) block_size + 4 > size - at || block_size < 32) throw std::runtime_error("failed to load alignments");
		++stats.records;
		AlleleRecord record;
		if (allele_record(records, at, size, n_ref, min_mapq, record)) {
			++stats.contributing;
			AlleleWalk walk;
			allele_walk_begin(walk, record, ref_length[record.ref]);
			uint32_t slot, column;
			while (allele_walk_next(walk, records, view, min_baseq, slot, column)) ++counts[(uint64_t) slot * ALLELE_COLUMNS + column];
		}
		at += (uint64_t) block_size + 4;
	}
	if (stats.records >= 0xFFFFFFF0ull) throw std::runtime_error("more than 2^32-16 alignment records");
	// the rows in the order of the lines
	for (uint64_t k = 0; k < placed; ++k) {
		agpu_allele_row& row = rows[order[k].second];
		const uint32_t* mine = &counts[k * ALLELE_COLUMNS];
		row.a = mine[ALLELE_A]; row.c = mine[ALLELE_C]; row.g = mine[ALLELE_G]; row.t = mine[ALLELE_T]; row.n = mine[ALLELE_N]; row.del = mine[ALLELE_DEL]; row.skip = mine[ALLELE_SKIP]; row.lowq = mine[ALLELE_LOWQ];
	}
	for (uint64_t line = 0; line < n_sites; ++line) {
		agpu_allele_row& row = rows[line];
		row.ref_base = sites[line].ref != ALLELE_UNPLACED ? allele_ref_base(genome, tid_to_contig[sites[line].ref], (uint32_t) sites[line].pos) : (uint8_t) '.';
		const uint64_t sum = (uint64_t) row.a + row.c + row.g + row.t + row.n + row.del + row.skip + row.lowq;
		stats.hits += sum; if (sum != 0) ++stats.covered;
	}
	stats.sites = n_sites; stats.placed = placed;
}

std::string allele_counts_text(const AlleleSiteList& list, const agpu_allele_row* rows, uint64_t n_rows) {
	if (n_rows != list.sites.size()) throw std::runtime_error("allele counts: " + std::to_string(n_rows) + " rows for " + std::to_string(list.sites.size()) + " sites");
	std::string text = "#CONTIG\tPOS\tREF\tA\tC\tG\tT\tN\tDEL\tSKIP\tLOWQ\n";
	for (uint64_t line = 0; line < n_rows; ++line) {
		const agpu_allele_row& row = rows[line];
		text.append(list.names, list.name_offset[line], list.name_offset[line + 1] - list.name_offset[line]);
		text += '\t'; text += std::to_string((uint64_t) list.sites[line].pos + 1);
		text += '\t'; text += (char) row.ref_base;
		const uint32_t fields[8] = { row.a, row.c, row.g, row.t, row.n, row.del, row.skip, row.lowq };
		for (int f = 0; f < 8; ++f) { text += '\t'; text += std::to_string(fields[f]); }
		text += '\n';
	}
	return text;
}

}
