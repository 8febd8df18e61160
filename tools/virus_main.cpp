// tools/virus_main.cpp -- stand-alone driver of the host side of --virus-expression for tools/sanitize_virus.sh (test tooling): virus_core.hpp stepped on the host over the
// records of an uncompressed BAM stream, and the counters turned into the table by arriba_amd/csrc/host/virus.cpp.
//   virus_main STREAM.raw TABLE.tsv [VIRAL_CONTIGS]
// Behind the table it steps the same records again with the stream cut short at every byte of its last records: a truncated stream must be refused, never read past its end.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>
#include "arriba_host.h"

int main(int argc, char** argv) {
	if (argc != 3 && argc != 4) { fprintf(stderr, "usage: virus_main STREAM.raw TABLE.tsv [VIRAL_CONTIGS]\n"); return 2; }
	std::ifstream raw(argv[1], std::ios::binary);
	std::vector<char> stream((std::istreambuf_iterator<char>(raw)), std::istreambuf_iterator<char>());
	if (stream.size() < 12 || memcmp(stream.data(), "BAM\1", 4) != 0) { fprintf(stderr, "ERROR: no BAM stream\n"); return 1; }
	auto word = [&](size_t at) { uint32_t v = 0; if (at + 4 <= stream.size()) memcpy(&v, &stream[at], 4); return v; };
	size_t at = 8 + word(4);
	const uint32_t n_ref = word(at);
	at += 4;
	for (uint32_t t = 0; t < n_ref; ++t) at += 8 + word(at);
	if (at > stream.size()) { fprintf(stderr, "ERROR: truncated header\n"); return 1; }
	ahost_virus_contigs contigs; agpu_virus_counters counters;
	if (ahost_virus_contigs_of(stream.data(), at, argc == 4 ? argv[3] : NULL, &contigs) != 0) { fprintf(stderr, "ERROR: %s\n", ahost_last_error()); return 1; }
	// (the records in a buffer of exactly their size: a read behind the last byte is a read behind the allocation)
	std::vector<char> records(stream.begin() + at, stream.end());
	if (ahost_virus_expression(records.data(), records.size(), &contigs, &counters) != 0) { fprintf(stderr, "ERROR: %s\n", ahost_last_error()); return 1; }
	if (ahost_virus_expression_write(&counters, &contigs, argv[2]) != 0) { fprintf(stderr, "ERROR: %s\n", ahost_last_error()); return 1; }
	printf("%llu mapped records, %u viral contigs, %u with reads, %llu candidates, %llu k-mer keys\n", (unsigned long long) counters.total, counters.n_viruses, counters.n_active, (unsigned long long) counters.candidates,
	       (unsigned long long) counters.kmer_keys);
	size_t refused = 0;
	for (size_t cut = 1; cut <= 400 && cut < records.size(); ++cut) {
		std::vector<char> shorter(records.begin(), records.end() - cut);
		agpu_virus_counters again;
		if (ahost_virus_expression(shorter.data(), shorter.size(), &contigs, &again) != 0) ++refused;
	}
	printf("%llu truncated streams refused\n", (unsigned long long) refused);
	return 0;
}
