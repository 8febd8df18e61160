// tools/realign_split_main.cpp -- stand-alone driver of the host side of --realign-reads for tools/sanitize_realign_split.sh (test tooling): realign_core.hpp stepped on the host
// over the records of an input (arriba_amd/csrc/host/realign_split.cpp) with the contigs of the assembly of a session, both files written through NAME.tmp.
//   realign_split_main GENOME.fa ANNOTATION.gtf "INTERESTING CONTIGS" INPUT REALIGN.sam KEPT.sam
// INPUT: BAM (BGZF, gzip or raw) or SAM text.  If it is a raw BAM stream, the same records are stepped again from memory, and then with the stream cut short at every byte of its
// last records -- the name, the CIGAR, SEQ and QUAL end inside the record there, which is where a formatter per byte would read past the end: a truncated stream must be refused,
// never read past its end.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>
#include "arriba_host.h"

int main(int argc, char** argv) {
	if (argc != 7) { fprintf(stderr, "usage: realign_split_main GENOME.fa ANNOTATION.gtf \"INTERESTING CONTIGS\" INPUT REALIGN.sam KEPT.sam\n"); return 2; }
	ahost_session* session = ahost_open(argv[1], argv[2], argv[3], NULL, NULL);
	if (!session) { fprintf(stderr, "ERROR: %s\n", ahost_last_error()); return 1; }
	agpu_realign_stats stats;
	if (ahost_realign_split_file(session, argv[4], argv[5], argv[6], &stats) != 0) { fprintf(stderr, "ERROR: %s\n", ahost_last_error()); return 1; }
	printf("%llu records, %llu templates, %llu realign, %llu kept, %llu dropped, %llu extra, %llu orphans\n", (unsigned long long) stats.records, (unsigned long long) stats.templates, (unsigned long long) stats.realign_templates,
	       (unsigned long long) stats.kept_templates, (unsigned long long) stats.dropped_secondary, (unsigned long long) stats.extra, (unsigned long long) stats.orphans);
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
		const char* realign = NULL; const char* kept = NULL; uint64_t realign_bytes = 0, kept_bytes = 0;
		agpu_realign_stats again;
		if (ahost_realign_split_of(session, header.data(), header.size(), records.data(), records.size(), 1, &realign, &realign_bytes, &kept, &kept_bytes, &again) != 0) { fprintf(stderr, "ERROR: %s\n", ahost_last_error()); return 1; }
		if (again.realign_bytes != stats.realign_bytes || again.kept_bytes != stats.kept_bytes || again.templates != stats.templates || realign_bytes != stats.realign_bytes) { fprintf(stderr, "ERROR: the records in memory give other statistics than the file\n"); return 1; }
		size_t refused = 0;
		for (size_t cut = 1; cut <= 400 && cut < records.size(); ++cut) {
			std::vector<char> shorter(records.begin(), records.end() - cut);
			if (ahost_realign_split_of(session, header.data(), header.size(), shorter.data(), shorter.size(), 1, &realign, &realign_bytes, &kept, &kept_bytes, &again) != 0) ++refused;
		}
		printf("%llu truncated streams refused\n", (unsigned long long) refused);
	}
	ahost_close(session);
	return 0;
}
