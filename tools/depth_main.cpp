// tools/depth_main.cpp -- stand-alone driver of the host side of --coverage for tools/sanitize_depth.sh (test tooling): depth_core.hpp stepped on the host over the records of an
// uncompressed BAM stream (arriba_amd/csrc/host/depth.cpp), the text written through TRACK.tmp.
//   depth_main STREAM.raw TRACK.bedgraph
// Behind the track it steps the same records again with the stream cut short at every byte of its last records: a truncated stream must be refused, never read past its end; and
// the line formatter on the largest values.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>
#include "arriba_host.h"

int main(int argc, char** argv) {
	if (argc != 3) { fprintf(stderr, "usage: depth_main STREAM.raw TRACK.bedgraph\n"); return 2; }
	std::ifstream raw(argv[1], std::ios::binary);
	std::vector<char> stream((std::istreambuf_iterator<char>(raw)), std::istreambuf_iterator<char>());
	if (stream.size() < 12 || memcmp(stream.data(), "BAM\1", 4) != 0) { fprintf(stderr, "ERROR: no BAM stream\n"); return 1; }
	auto word = [&](size_t at) { uint32_t v = 0; if (at + 4 <= stream.size()) memcpy(&v, &stream[at], 4); return v; };
	size_t at = 8 + word(4);
	const uint32_t n_ref = word(at);
	at += 4;
	for (uint32_t t = 0; t < n_ref; ++t) at += 8 + word(at);
	if (at > stream.size()) { fprintf(stderr, "ERROR: truncated header\n"); return 1; }
	ahost_depth_contigs contigs; agpu_depth_stats stats;
	if (ahost_depth_contigs_of(stream.data(), at, &contigs) != 0) { fprintf(stderr, "ERROR: %s\n", ahost_last_error()); return 1; }
	// (the records in a buffer of exactly their size: a read behind the last byte is a read behind the allocation)
	std::vector<char> records(stream.begin() + at, stream.end());
	const char* text = NULL; uint64_t bytes = 0;
	if (ahost_depth_track(records.data(), records.size(), &contigs, &text, &bytes, &stats) != 0) { fprintf(stderr, "ERROR: %s\n", ahost_last_error()); return 1; }
	if (ahost_depth_write(text, bytes, argv[2]) != 0) { fprintf(stderr, "ERROR: %s\n", ahost_last_error()); return 1; }
	printf("%llu records, %llu segments, %llu runs, %llu covered positions, depth up to %llu, %llu bytes of text\n", (unsigned long long) stats.records, (unsigned long long) stats.segments, (unsigned long long) stats.runs,
	       (unsigned long long) stats.covered_positions, (unsigned long long) stats.max_depth, (unsigned long long) stats.text_bytes);
	size_t refused = 0;
	for (size_t cut = 1; cut <= 400 && cut < records.size(); ++cut) {
		std::vector<char> shorter(records.begin(), records.end() - cut);
		agpu_depth_stats again;
		if (ahost_depth_track(shorter.data(), shorter.size(), &contigs, &text, &bytes, &again) != 0) ++refused;
	}
	printf("%llu truncated streams refused\n", (unsigned long long) refused);
	std::vector<char> line(45); uint32_t length = 0; // (exactly what the longest line of this name takes)
	if (ahost_depth_line("contig_name", 4294967295u, 4294967295u, 4294967295u, line.data(), (uint32_t) line.size(), &length) != 0 || length != 45 || memcmp(line.data(), "contig_name\t4294967295\t4294967295\t4294967295\n", 45) != 0) {
		fprintf(stderr, "ERROR: the line formatter\n"); return 1;
	}
	return 0;
}
