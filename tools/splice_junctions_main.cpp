// tools/splice_junctions_main.cpp -- stand-alone driver of the host side of --splice-junctions for tools/sanitize_splice_junctions.sh (test tooling): junction_core.hpp stepped on
// the host over the records of an input (arriba_amd/csrc/host/splice_junctions.cpp) against the annotation and the assembly of a session, the table written through JUNCTIONS.tmp.
//   splice_junctions_main GENOME.fa ANNOTATION.gtf "INTERESTING CONTIGS" INPUT JUNCTIONS.tab
// INPUT: BAM (BGZF, gzip or raw) or SAM text.  If it is a raw BAM stream, the same records are stepped again with the stream cut short at every byte of its last records: a truncated
// stream must be refused, never read past its end.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>
#include "arriba_host.h"

int main(int argc, char** argv) {
	if (argc != 6) { fprintf(stderr, "usage: splice_junctions_main GENOME.fa ANNOTATION.gtf \"INTERESTING CONTIGS\" INPUT JUNCTIONS.tab\n"); return 2; }
	ahost_session* session = ahost_open(argv[1], argv[2], argv[3], NULL, NULL);
	if (!session) { fprintf(stderr, "ERROR: %s\n", ahost_last_error()); return 1; }
	agpu_junction_stats stats;
	if (ahost_splice_junctions_file(session, argv[4], argv[5], &stats) != 0) { fprintf(stderr, "ERROR: %s\n", ahost_last_error()); return 1; }
	printf("%llu records, %llu contributing, %llu crossings, %llu pairs, %llu junctions, %llu annotated\n", (unsigned long long) stats.records, (unsigned long long) stats.contributing, (unsigned long long) stats.crossings,
	       (unsigned long long) stats.pairs, (unsigned long long) stats.junctions, (unsigned long long) stats.annotated);
	std::ifstream raw(argv[4], std::ios::binary);
	std::vector<char> stream((std::istreambuf_iterator<char>(raw)), std::istreambuf_iterator<char>());
	if (stream.size() >= 12 && memcmp(stream.data(), "BAM\1", 4) == 0) {
		auto word = [&](size_t at) { uint32_t v = 0; if (at + 4 <= stream.size()) memcpy(&v, &stream[at], 4); return v; };
		size_t at = 8 + word(4);
		const uint32_t n_ref = word(at);
		at += 4;
		for (uint32_t t = 0; t < n_ref; ++t) at += 8 + word(at);
		if (at > stream.size()) { fprintf(stderr, "ERROR: truncated header\n"); return 1; }
		// (the records in a buffer of exactly their size: a read behind the last byte is a read behind the allocation)
		std::vector<char> header(stream.begin(), stream.begin() + at), records(stream.begin() + at, stream.end());
		const agpu_junction_row* rows = NULL; uint64_t n_rows = 0;
		agpu_junction_stats again;
		if (ahost_splice_junctions_of(session, header.data(), header.size(), records.data(), records.size(), &rows, &n_rows, &again) != 0) { fprintf(stderr, "ERROR: %s\n", ahost_last_error()); return 1; }
		if (again.pairs != stats.pairs || again.crossings != stats.crossings || n_rows != stats.junctions) { fprintf(stderr, "ERROR: the records in memory give other statistics than the file\n"); return 1; }
		size_t refused = 0;
		for (size_t cut = 1; cut <= 400 && cut < records.size(); ++cut) {
			std::vector<char> shorter(records.begin(), records.end() - cut);
			if (ahost_splice_junctions_of(session, header.data(), header.size(), shorter.data(), shorter.size(), &rows, &n_rows, &again) != 0) ++refused;
		}
		printf("%llu truncated streams refused\n", (unsigned long long) refused);
	}
	ahost_close(session);
	return 0;
}
