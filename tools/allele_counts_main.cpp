// tools/allele_counts_main.cpp -- stand-alone driver of the host side of --allele-counts for tools/sanitize_allele_counts.sh (test tooling): the reader of the sites file and
// allele_core.hpp stepped on the host over the records of an input (arriba_amd/csrc/host/allele_counts.cpp) with REF from the assembly of a session, the table written through
// COUNTS.tmp.
//   allele_counts_main GENOME.fa ANNOTATION.gtf "INTERESTING CONTIGS" INPUT SITES MIN_MAPQ MIN_BASEQ COUNTS.tsv
// INPUT: BAM (BGZF, gzip or raw) or SAM text.  If it is a raw BAM stream, the same records are stepped again from memory, and then with the stream cut short at every byte of its
// last records -- SEQ and QUAL end inside the record there, which is where a walk per base would read past the end: a truncated stream must be refused, never read past its end.
// SITES is read once more with every line cut short, which must be refused or give fewer sites, never read past the end of the text.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>
#include "arriba_host.h"

int main(int argc, char** argv) {
	if (argc != 9) { fprintf(stderr, "usage: allele_counts_main GENOME.fa ANNOTATION.gtf \"INTERESTING CONTIGS\" INPUT SITES MIN_MAPQ MIN_BASEQ COUNTS.tsv\n"); return 2; }
	ahost_session* session = ahost_open(argv[1], argv[2], argv[3], NULL, NULL);
	if (!session) { fprintf(stderr, "ERROR: %s\n", ahost_last_error()); return 1; }
	const uint32_t min_mapq = (uint32_t) atoi(argv[6]), min_baseq = (uint32_t) atoi(argv[7]);
	agpu_allele_stats stats;
	if (ahost_allele_counts_file(session, argv[4], argv[5], argv[8], min_mapq, min_baseq, &stats) != 0) { fprintf(stderr, "ERROR: %s\n", ahost_last_error()); return 1; }
	printf("%llu records, %llu contributing, %llu hits, %llu sites, %llu placed, %llu covered\n", (unsigned long long) stats.records, (unsigned long long) stats.contributing, (unsigned long long) stats.hits,
	       (unsigned long long) stats.sites, (unsigned long long) stats.placed, (unsigned long long) stats.covered);
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
		ahost_allele_sites sites;
		if (ahost_allele_sites_load(argv[5], header.data(), header.size(), &sites) != 0) { fprintf(stderr, "ERROR: %s\n", ahost_last_error()); return 1; }
		const agpu_allele_row* rows = NULL;
		agpu_allele_stats again;
		if (ahost_allele_counts_of(session, header.data(), header.size(), records.data(), records.size(), &sites, min_mapq, min_baseq, &rows, &again) != 0) { fprintf(stderr, "ERROR: %s\n", ahost_last_error()); return 1; }
		if (again.hits != stats.hits || again.contributing != stats.contributing || again.covered != stats.covered || again.placed != stats.placed) { fprintf(stderr, "ERROR: the records in memory give other statistics than the file\n"); return 1; }
		size_t refused = 0;
		for (size_t cut = 1; cut <= 400 && cut < records.size(); ++cut) {
			std::vector<char> shorter(records.begin(), records.end() - cut);
			if (ahost_allele_counts_of(session, header.data(), header.size(), shorter.data(), shorter.size(), &sites, min_mapq, min_baseq, &rows, &again) != 0) ++refused;
		}
		printf("%llu truncated streams refused\n", (unsigned long long) refused);
		ahost_allele_sites_free(&sites);
	}
	{ // the sites file cut short at every byte of its last lines
		std::ifstream text(argv[5], std::ios::binary);
		const std::string whole((std::istreambuf_iterator<char>(text)), std::istreambuf_iterator<char>());
		const std::string path = std::string(argv[8]) + ".sites";
		size_t refused = 0, read = 0;
		for (size_t cut = 1; cut <= 200 && cut <= whole.size(); ++cut) {
			{ std::ofstream out(path.c_str(), std::ios::binary); out.write(whole.data(), (std::streamsize) (whole.size() - cut)); }
			ahost_allele_sites sites;
			if (ahost_allele_sites_load(path.c_str(), NULL, 0, &sites) != 0) ++refused; else { ++read; ahost_allele_sites_free(&sites); }
		}
		remove(path.c_str());
		printf("%llu shortened sites files refused, %llu read\n", (unsigned long long) refused, (unsigned long long) read);
	}
	ahost_close(session);
	return 0;
}
