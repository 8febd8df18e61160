// tools/rna_metrics_main.cpp -- stand-alone driver of the host side of --rna-metrics for tools/sanitize_rna_metrics.sh (test tooling): the reader of the interval file, the sweep
// that builds the region track (arriba_amd/csrc/host/region_track.cpp) and rnametrics_core.hpp stepped on the host over the records of an input
// (arriba_amd/csrc/host/rna_metrics.cpp), the table written through METRICS.tmp.
//   rna_metrics_main GENOME.fa ANNOTATION.gtf "INTERESTING CONTIGS" INPUT INTERVALS.bed METRICS.tsv
// INPUT: BAM (BGZF, gzip or raw) or SAM text.  If it is a raw BAM stream, the same records are stepped again from memory, and then with the stream cut short at every byte of its
// last records: a truncated stream must be refused, never read past its end.  INTERVALS.bed is read once more with every line cut short, which must be refused or give fewer
// intervals, never read past the end of the text.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>
#include "arriba_host.h"

int main(int argc, char** argv) {
	if (argc != 7) { fprintf(stderr, "usage: rna_metrics_main GENOME.fa ANNOTATION.gtf \"INTERESTING CONTIGS\" INPUT INTERVALS.bed METRICS.tsv\n"); return 2; }
	ahost_session* session = ahost_open(argv[1], argv[2], argv[3], NULL, NULL);
	if (!session) { fprintf(stderr, "ERROR: %s\n", ahost_last_error()); return 1; }
	agpu_rna_metrics_stats stats;
	if (ahost_rna_metrics_file(session, argv[4], argv[5], argv[6], &stats) != 0) { fprintf(stderr, "ERROR: %s\n", ahost_last_error()); return 1; }
	printf("%llu records, %llu base records, %llu blocks, %llu segments, %llu runs\n", (unsigned long long) stats.records, (unsigned long long) stats.base_records, (unsigned long long) stats.blocks,
	       (unsigned long long) stats.segments, (unsigned long long) stats.track_runs);
	std::ifstream raw(argv[4], std::ios::binary);
	std::vector<char> stream((std::istreambuf_iterator<char>(raw)), std::istreambuf_iterator<char>());
	if (stream.size() >= 12 && memcmp(stream.data(), "BAM\1", 4) == 0) {
		auto word = [&](size_t at) { uint32_t v = 0; if (at + 4 <= stream.size()) memcpy(&v, &stream[at], 4); return v; };
		size_t at = 8 + word(4);
		const uint32_t n_ref = word(at);
		at += 4;
		for (uint32_t t = 0; t < n_ref; ++t) at += 8 + word(at);
		if (at > stream.size()) { fprintf(stderr, "ERROR: truncated header\n"); return 1; }
		std::vector<uint64_t> counters(AGPU_RNA_METRICS_WORDS); // (exactly what a block takes)
		// (the records in a buffer of exactly their size: a read behind the last byte is a read behind the allocation)
		std::vector<char> header(stream.begin(), stream.begin() + at), records(stream.begin() + at, stream.end());
		agpu_rna_metrics_stats again;
		if (ahost_rna_metrics_of(session, argv[5], header.data(), header.size(), records.data(), records.size(), counters.data(), counters.size(), &again) != 0) { fprintf(stderr, "ERROR: %s\n", ahost_last_error()); return 1; }
		if (again.blocks != stats.blocks || again.segments != stats.segments || again.base_records != stats.base_records) { fprintf(stderr, "ERROR: the records in memory give other statistics than the file\n"); return 1; }
		size_t refused = 0;
		for (size_t cut = 1; cut <= 400 && cut < records.size(); ++cut) {
			std::vector<char> shorter(records.begin(), records.end() - cut);
			if (ahost_rna_metrics_of(session, argv[5], header.data(), header.size(), shorter.data(), shorter.size(), counters.data(), counters.size(), &again) != 0) ++refused;
		}
		printf("%llu truncated streams refused\n", (unsigned long long) refused);
	}
	{ // the interval file cut short at every byte of its last lines
		std::ifstream text(argv[5], std::ios::binary);
		const std::string whole((std::istreambuf_iterator<char>(text)), std::istreambuf_iterator<char>());
		const std::string path = std::string(argv[6]) + ".bed";
		size_t refused = 0, read = 0;
		for (size_t cut = 1; cut <= 200 && cut <= whole.size(); ++cut) {
			{ std::ofstream out(path.c_str(), std::ios::binary); out.write(whole.data(), (std::streamsize) (whole.size() - cut)); }
			uint64_t n = 0;
			if (ahost_rrna_intervals_load(path.c_str(), &n) != 0) ++refused; else ++read;
		}
		remove(path.c_str());
		printf("%llu shortened interval files refused, %llu read\n", (unsigned long long) refused, (unsigned long long) read);
	}
	ahost_close(session);
	return 0;
}
