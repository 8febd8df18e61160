// tools/supporting_main.cpp -- stand-alone driver of the host side of --supporting-alignments for tools/sanitize_supporting.sh (test tooling): supporting_core.hpp stepped on
// the host over the records of an uncompressed BAM stream, the files cut and indexed by the writer of arriba_amd/csrc/host/supporting.cpp.
//   supporting_main STREAM.raw ROWS.txt WINDOW PREFIX
// ROWS.txt: lines "N <name>" (the list of names, in order) and "R <ref1> <breakpoint1> <ref2> <breakpoint2> <entry> ..." (a row: 0-based breakpoints, entries of the list).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>
#include "arriba_host.h"

int main(int argc, char** argv) {
	if (argc != 5) { fprintf(stderr, "usage: supporting_main STREAM.raw ROWS.txt WINDOW PREFIX\n"); return 2; }
	std::ifstream raw(argv[1], std::ios::binary);
	std::vector<char> stream((std::istreambuf_iterator<char>(raw)), std::istreambuf_iterator<char>());
	if (stream.size() < 12 || memcmp(stream.data(), "BAM\1", 4) != 0) { fprintf(stderr, "ERROR: no BAM stream\n"); return 1; }
	auto word = [&](size_t at) { uint32_t v = 0; if (at + 4 <= stream.size()) memcpy(&v, &stream[at], 4); return v; };
	size_t at = 8 + word(4);
	const uint32_t n_ref = word(at);
	at += 4;
	for (uint32_t t = 0; t < n_ref; ++t) at += 8 + word(at);
	if (at > stream.size()) { fprintf(stderr, "ERROR: truncated header\n"); return 1; }
	std::string names; std::vector<uint64_t> name_offset(1, 0), name_begin(1, 0); std::vector<int32_t> ref, breakpoint; std::vector<uint32_t> entries;
	std::ifstream text(argv[2]);
	for (std::string line; std::getline(text, line); ) {
		if (line.compare(0, 2, "N ") == 0) { names += line.substr(2); name_offset.push_back(names.size()); }
		else if (line.compare(0, 2, "R ") == 0) {
			std::istringstream fields(line.substr(2));
			for (int k = 0; k < 2; ++k) { int32_t r, b; fields >> r >> b; ref.push_back(r); breakpoint.push_back(b); }
			for (uint32_t entry; fields >> entry; ) entries.push_back(entry);
			name_begin.push_back(entries.size());
		}
	}
	const agpu_supporting_rows rows = { (uint32_t) (name_begin.size() - 1), ref.data(), breakpoint.data(), name_begin.data(), entries.data() };
	agpu_supporting_info info;
	if (ahost_supporting_alignments(stream.data(), at, stream.data() + at, stream.size() - at, names.data(), name_offset.data(), name_offset.size() - 1, &rows, atoll(argv[3]), argv[4], &info) != 0) {
		fprintf(stderr, "ERROR: %s\n", ahost_last_error()); return 1;
	}
	printf("%llu rows, %llu records, %llu bytes uncompressed, %llu bytes of record blocks in %llu blocks\n", (unsigned long long) info.rows, (unsigned long long) info.records, (unsigned long long) info.uncompressed_bytes,
	       (unsigned long long) info.file_bytes, (unsigned long long) info.blocks);
	// a row that lists an entry the list does not have is refused, and nothing is written
	const uint32_t bad_entry = (uint32_t) (name_offset.size() - 1); const uint64_t one_begin[2] = { 0, 1 }; const int32_t one_ref[2] = { 0, 0 }, one_breakpoint[2] = { 10, 20 };
	const agpu_supporting_rows bad = { 1, one_ref, one_breakpoint, one_begin, &bad_entry };
	const std::string bad_prefix = std::string(argv[4]) + "_refused";
	if (ahost_supporting_alignments(stream.data(), at, stream.data() + at, stream.size() - at, names.data(), name_offset.data(), name_offset.size() - 1, &bad, 1000, bad_prefix.c_str(), NULL) == 0) { fprintf(stderr, "ERROR: a bad row was accepted\n"); return 1; }
	return 0;
}
