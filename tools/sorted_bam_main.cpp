// tools/sorted_bam_main.cpp -- stand-alone driver of the host side of --sorted-bam for tools/sanitize_sorted_bam.sh (test tooling): the records of a file in coordinate
// order with their index (ahost_sorted_bam_file: sorted_bam_core.hpp stepped on the host), and the header rewriting on the head of the same file.
//   sorted_bam_main INPUT.bam OUTPUT.bam
#include <cstdio>
#include <cstdlib>
#include "arriba_host.h"

int main(int argc, char** argv) {
	if (argc != 3) { fprintf(stderr, "usage: sorted_bam_main INPUT.bam OUTPUT.bam\n"); return 2; }
	agpu_sorted_bam_info info;
	if (ahost_sorted_bam_file(argv[1], argv[2], &info) != 0) { fprintf(stderr, "ERROR: %s\n", ahost_last_error()); return 1; }
	printf("%llu records, %llu bytes uncompressed, %llu bytes of record blocks\n", (unsigned long long) info.records, (unsigned long long) info.uncompressed_bytes, (unsigned long long) info.file_bytes);
	// the header of SAM text, with and without LN (the latter is an error that names the line)
	const char* texts[] = { "@SQ\tSN:chr1\tLN:1000\n@PG\tID:x\n", "@HD\tVN:1.6\tSO:queryname\tGO:query\n@SQ\tSN:chr1\n" };
	for (int k = 0; k < 2; ++k) {
		const uint8_t* framed = NULL; uint64_t bytes = 0; const uint32_t* lengths = NULL; uint32_t n_ref = 0;
		size_t size = 0; while (texts[k][size] != 0) ++size;
		const int status = ahost_sorted_bam_header_of(texts[k], size, &framed, &bytes, &lengths, &n_ref);
		if ((status == 0) != (k == 0)) { fprintf(stderr, "ERROR: header %d: status %d (%s)\n", k, status, ahost_last_error()); return 1; }
	}
	return 0;
}
