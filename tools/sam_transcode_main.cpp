// tools/sam_transcode_main.cpp -- ahost_sam_transcode on the alignment lines of SAM files, for tools/sanitize_sam.sh (test tooling): the @SQ names are read from the
// header lines of every file; prints "FILE status bad_line n_records out_bytes".  With ARRIBA_SAM_ISOLATE_LINES=1 every line is parsed from a heap copy of exactly its
// size, so that AddressSanitizer sees a read outside the line.
#include "../include/arriba_host.h"
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

int main(int argc, char** argv) {
	for (int a = 1; a < argc; ++a) {
		std::ifstream in(argv[a], std::ios::binary);
		const std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
		std::string names; std::vector<uint32_t> offsets(1, 0);
		for (size_t at = 0; at < text.size() && text[at] == '@'; ) {
			size_t end = text.find('\n', at);
			if (end == std::string::npos) end = text.size();
			const std::string line = text.substr(at, end - at);
			const size_t name = line.find("\tSN:");
			if (line.compare(0, 3, "@SQ") == 0 && name != std::string::npos) { names += line.substr(name + 4, line.find('\t', name + 4) - name - 4); offsets.push_back((uint32_t) names.size()); }
			at = end + 1;
		}
		if (offsets.size() == 1) for (const char* fallback : { "chr1", "chr2", "chrUn_KI270442v1" }) { names += fallback; offsets.push_back((uint32_t) names.size()); } // (the names of the hand-made lines of tests/test_sam_input.py)
		std::vector<uint8_t> out(2 * text.size() + 64);
		uint64_t out_bytes = 0, n_records = 0, bad_line = 0;
		const int status = ahost_sam_transcode(text.data(), text.size(), names.data(), offsets.data(), (uint32_t) offsets.size() - 1, out.data(), out.size(), &out_bytes, &n_records, &bad_line);
		printf("%s %d %llu %llu %llu\n", argv[a], status, (unsigned long long) bad_line, (unsigned long long) n_records, (unsigned long long) out_bytes);
	}
	return 0;
}
