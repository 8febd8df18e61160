// arriba_amd/csrc/host/virus.cpp -- the host side of --virus-expression (include/arriba_host.h: ahost_virus_*): the viral contigs of a header by the patterns of -v,
// arriba_amd/csrc/device/virus_core.hpp stepped over records in host memory -- the comparator of agpu_virus.hip, and what --host-ingest and the CPU tier run --, and the part that
// is the host's on every path: counters to text.  The double arithmetic, the removal of related strains, the thresholds, the number forms and the row order are those of the
// reference's scripts/quantify_virus_expression.sh under mawk and `LC_ALL=C sort -k6,6gr`.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#include "arriba_host.h"
#include "../device/virus_core.hpp"

namespace arriba {

namespace {
uint32_t get32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
// a number as awk's print writes it: an integral value as an integer, anything else with OFMT "%.6g"
std::string awk_number(double value) {
	char text[64];
	if (value == std::floor(value) && std::fabs(value) < 1e15) snprintf(text, sizeof(text), "%lld", (long long) value);
	else snprintf(text, sizeof(text), "%.6g", value);
	return text;
}
}

ahost_virus_contigs VirusContigs::view() {
	ahost_virus_contigs v;
	v.n_ref = n_ref; v.n_viruses = (uint32_t) ref.size(); v.viral_ref = ref.data(); v.viral_length = length.data(); v.names = names.data(); v.name_offset = name_offset.data();
	return v;
}

agpu_virus_counters VirusCounters::view() const {
	agpu_virus_counters v; memset(&v, 0, sizeof(v));
	v.total = total; v.n_viruses = (uint32_t) reads.size(); v.n_active = (uint32_t) active.size();
	v.reads = reads.data(); v.covered = covered.data(); v.kmer_count = kmer_count.data(); v.active = active.data(); v.shared = shared.data();
	v.candidates = candidates; v.kmer_keys = kmer_keys; v.kmer_rounds = kmer_keys > 0 ? 1 : 0;
	return v;
}

// the references of a header (a BAM header, or the '@' lines of SAM text) in their order
void header_contigs(const uint8_t* input, size_t size, std::vector<std::string>& names, std::vector<uint32_t>& lengths) {
	names.clear(); lengths.clear();
	if (size >= 4 && memcmp(input, "BAM\1", 4) == 0) {
		if (size < 12) throw std::runtime_error("failed to read SAM header");
		const uint64_t l_text = get32(input + 4);
		if (size < 12 + l_text) throw std::runtime_error("failed to read SAM header");
		const uint32_t n_ref = get32(input + 8 + l_text);
		uint64_t at = 12 + l_text;
		for (uint32_t t = 0; t < n_ref; ++t) {
			if (size < at + 4) throw std::runtime_error("failed to read SAM header");
			const uint64_t l_name = get32(input + at);
			if (size < at + 4 + l_name + 4) throw std::runtime_error("failed to read SAM header");
			names.push_back(std::string((const char*) input + at + 4, l_name > 0 ? l_name - 1 : 0));
			lengths.push_back(get32(input + at + 4 + l_name));
			at += 8 + l_name;
		}
	} else {
		for (size_t at = 0; at < size && input[at] == '@'; ) {
			const uint8_t* feed = (const uint8_t*) memchr(input + at, '\n', size - at);
			size_t end = feed != NULL ? (size_t) (feed - input) : size;
			const size_t next = feed != NULL ? end + 1 : size;
			if (end > at && input[end - 1] == '\r') --end;
			const std::string line((const char*) input + at, end - at);
			if (line.compare(0, 4, "@SQ\t") == 0) {
				std::string name; uint64_t length = 0;
				for (size_t field = 4; field < line.size(); ) {
					size_t field_end = line.find('\t', field);
					if (field_end == std::string::npos) field_end = line.size();
					if (line.compare(field, 3, "SN:") == 0) name = line.substr(field + 3, field_end - field - 3);
					else if (line.compare(field, 3, "LN:") == 0) length = strtoull(line.c_str() + field + 3, NULL, 10);
					field = field_end + 1;
				}
				names.push_back(name); lengths.push_back((uint32_t) length);
			}
			at = next;
		}
	}
}

// a virus's index is its position in the list of the header; those of the references that -v names
void virus_contigs_of(const uint8_t* input, size_t size, const std::string& viral_contigs, VirusContigs& contigs) {
	std::vector<std::string> names; std::vector<uint32_t> lengths;
	header_contigs(input, size, names, lengths);
	contigs = VirusContigs();
	contigs.n_ref = (uint32_t) names.size();
	contigs.name_offset.push_back(0);
	for (size_t t = 0; t < names.size(); ++t) {
		if (!is_interesting_contig(names[t], viral_contigs)) continue;
		contigs.ref.push_back((int32_t) t); contigs.length.push_back(lengths[t]); contigs.name.push_back(names[t]);
		contigs.names += names[t]; contigs.name_offset.push_back((uint32_t) contigs.names.size());
	}
}

// ---- the stepping on the host ----

void virus_expression(const uint8_t* records, uint64_t size, const int32_t* viral_ref, const uint32_t* viral_length, uint32_t n_viruses, uint32_t n_ref, VirusCounters& counters) {
	using namespace agpu;
	if (n_viruses > VIRUS_MAX_SLOTS) throw std::runtime_error("--virus-expression: " + std::to_string(n_viruses) + " viral contigs, more than the 65535 that a k-mer key can name");
	std::vector<uint32_t> slot_of_ref(n_ref, VIRUS_NO_SLOT);
	std::vector<uint64_t> bitmap_offset((size_t) n_viruses + 1, 0);
	for (uint32_t v = 0; v < n_viruses; ++v) {
		if (viral_ref[v] < 0 || (uint32_t) viral_ref[v] >= n_ref || (v > 0 && viral_ref[v] <= viral_ref[v - 1])) throw std::runtime_error("the viral refIDs must ascend and lie below n_ref");
		slot_of_ref[viral_ref[v]] = v; bitmap_offset[v + 1] = bitmap_offset[v] + virus_bitmap_words(viral_length[v]);
	}
	std::vector<uint32_t> bitmap(bitmap_offset[n_viruses], 0);
	counters = VirusCounters();
	counters.reads.assign(n_viruses, 0); counters.covered.assign(n_viruses, 0); counters.kmer_count.assign(n_viruses, 0);
	std::vector<uint64_t> keys;
	for (uint64_t at = 0; at < size; ) {
		if (size - at < 36 || (uint64_t) get32(records + at) + 4 > size - at || get32(records + at) < 32) throw std::runtime_error("failed to load alignments");
		const VirusRecord record = virus_parse(records, at, size);
		at += (uint64_t) get32(records + at) + 4;
		if (!virus_mapped(record.flag)) continue;
		++counters.total;
		if (!virus_flag_ok(record.flag) || !record.whole || record.ref < 0 || (uint32_t) record.ref >= n_ref || slot_of_ref[record.ref] == VIRUS_NO_SLOT) continue;
		if (!virus_cigar_ok(records, record.cigar_at, record.n_cigar)) continue;
		++counters.candidates;
		const uint32_t slot = slot_of_ref[record.ref];
		const uint8_t* seq = records + record.seq_at;
		if (virus_tandem(seq, record.l_seq)) continue;
		++counters.reads[slot];
		uint32_t* words = bitmap.data() + bitmap_offset[slot];
		virus_cover(records, record.cigar_at, record.n_cigar, record.pos, viral_length[slot], [words](uint32_t word, uint32_t mask) { words[word] |= mask; });
		for (uint32_t i = 0; i < virus_kmer_count(record.l_seq); ++i) keys.push_back(virus_kmer_key(seq, i, slot));
	}
	counters.kmer_keys = keys.size();
	std::sort(keys.begin(), keys.end());
	keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
	std::vector<uint32_t> dense(n_viruses, VIRUS_NO_SLOT);
	for (uint32_t v = 0; v < n_viruses; ++v) {
		for (uint64_t w = bitmap_offset[v]; w < bitmap_offset[v + 1]; ++w) counters.covered[v] += (uint64_t) __builtin_popcount(bitmap[w]);
		if (counters.reads[v] > 0) { dense[v] = (uint32_t) counters.active.size(); counters.active.push_back(v); }
	}
	const size_t n_active = counters.active.size();
	counters.shared.assign(n_active * n_active, 0);
	for (size_t i = 0; i < keys.size(); ) {
		size_t end = i + 1;
		while (end < keys.size() && keys[end] >> 16 == keys[i] >> 16) ++end;
		for (size_t a = i; a < end; ++a) {
			++counters.kmer_count[keys[a] & 0xFFFFu];
			for (size_t b = i; b < end; ++b) if (a != b) ++counters.shared[dense[keys[a] & 0xFFFFu] * n_active + dense[keys[b] & 0xFFFFu]];
		}
		i = end;
	}
}

// ---- counters to text ----

std::string virus_expression_table(const agpu_virus_counters& c, const ahost_virus_contigs& contigs) {
	if (c.n_viruses != contigs.n_viruses) throw std::runtime_error("the counters are not those of the viral contigs");
	const uint32_t n_active = c.n_active;
	// rpkm: for the viruses with reads, a genome size and a total
	std::vector<double> rpkm(n_active, 0); std::vector<bool> has_rpkm(n_active, false), removed(n_active, false);
	for (uint32_t a = 0; a < n_active; ++a) {
		const uint32_t v = c.active[a];
		if (v >= c.n_viruses || (a > 0 && v <= c.active[a - 1])) throw std::runtime_error("the active slots of the counters must ascend");
		if (c.reads[v] > 0 && contigs.viral_length[v] > 0 && c.total > 0) { rpkm[a] = 1000000000.0 * (double) c.reads[v] / (double) contigs.viral_length[v] / (double) c.total; has_rpkm[a] = true; }
	}
	// a virus is removed by every related one that beats it, whether that one is removed itself or not (slots ascend with the index of the virus in the header)
	for (uint32_t i = 0; i < n_active; ++i)
		for (uint32_t j = 0; j < n_active; ++j) {
			if (i == j || !has_rpkm[i] || !has_rpkm[j]) continue;
			const bool beats = rpkm[i] > rpkm[j] || (rpkm[i] == rpkm[j] && i < j);
			if (beats && c.shared[(size_t) i * n_active + j] * 100 > c.kmer_count[c.active[j]] * agpu::VIRUS_SHARED_PCT) removed[j] = true; // (shared > kmer_count * 10 / 100, in integers)
		}
	struct Row { double key; std::string line; };
	std::vector<Row> rows;
	for (uint32_t a = 0; a < n_active; ++a) {
		if (!has_rpkm[a] || removed[a]) continue;
		const uint32_t v = c.active[a];
		const double covered = (double) c.covered[v], length = (double) contigs.viral_length[v];
		if (!(c.covered[v] >= agpu::VIRUS_MIN_COVERED_BASES && covered / length > (double) agpu::VIRUS_MIN_COVERED_PCT / 100)) continue;
		Row row;
		const std::string printed = awk_number(rpkm[a]);
		row.key = strtod(printed.c_str(), NULL); // (sort -g reads the printed column)
		row.line = std::string(contigs.names + contigs.name_offset[v], contigs.name_offset[v + 1] - contigs.name_offset[v]) + "\t" + std::to_string(contigs.viral_length[v]) + "\t" + std::to_string(c.covered[v]) + "\t" +
		           awk_number(covered / length) + "\t" + std::to_string(c.reads[v]) + "\t" + printed;
		rows.push_back(row);
	}
	std::sort(rows.begin(), rows.end(), [](const Row& a, const Row& b) { return a.key != b.key ? a.key > b.key : a.line < b.line; }); // (std::string compares bytes as unsigned: LC_ALL=C)
	std::string text = "VIRUS\tGENOME_SIZE\tCOVERED_BASES\tCOVERED_GENOME_FRACTION\tHIGH_QUALITY_ALIGNMENTS\tRPKM\n";
	for (size_t r = 0; r < rows.size(); ++r) text += rows[r].line + "\n";
	return text;
}

void virus_expression_write(const std::string& text, const std::string& path) {
	const std::string temporary = path + ".tmp";
	FILE* file = fopen(temporary.c_str(), "wb");
	if (file == NULL) throw std::runtime_error("failed to open '" + temporary + "' for writing");
	const bool written = fwrite(text.data(), 1, text.size(), file) == text.size();
	if (fclose(file) != 0 || !written) { remove(temporary.c_str()); throw std::runtime_error("failed to write '" + temporary + "'"); }
	if (rename(temporary.c_str(), path.c_str()) != 0) { remove(temporary.c_str()); throw std::runtime_error("failed to write '" + path + "'"); }
}

}
