// tools/deflate_out_main.cpp -- stand-alone driver of the host stepping of --sorted-bam-compression for tools/sanitize_host.sh (test tooling): the records of a file sorted and
// deflated at level 1 (ahost_sorted_bam_file_level: arriba_amd/csrc/device/deflate_out_core.hpp stepped on the host), and the code-length builder of that header on counts that
// make trees deeper than the limits (Fibonacci-like counts, random counts): every code must be complete and within its limit.
//   deflate_out_main INPUT.bam OUTPUT.bam
#include <cstdio>
#include <cstdint>
#include <cstring>
#include <vector>
#include "arriba_host.h"
#include "../arriba_amd/csrc/device/deflate_out_core.hpp"

static bool complete(const std::vector<uint32_t>& count, uint32_t limit) {
	using namespace agpu;
	const uint32_t n = (uint32_t) count.size();
	std::vector<uint16_t> sorted(n + 2); std::vector<uint32_t> work(n + 2); std::vector<uint8_t> length(n + 2, 0); uint32_t per_length[34], used = 0;
	for (uint32_t t = 0; t < n; ++t) if (count[t] != 0) { sorted[dfo_rank(count.data(), n, t)] = (uint16_t) t; ++used; }
	dfo_code_lengths(count.data(), sorted.data(), used, limit, work.data(), per_length, length.data());
	uint64_t kraft = 0;
	for (uint32_t t = 0; t < n; ++t) {
		if ((count[t] != 0) != (length[t] != 0) || length[t] > limit) return false;
		if (length[t] != 0) kraft += 1ull << (limit - length[t]);
	}
	return used < 2 ? kraft == (used == 1 ? 1ull << (limit - 1) : 0) : kraft == 1ull << limit;
}

int main(int argc, char** argv) {
	if (argc != 3) { fprintf(stderr, "usage: deflate_out_main INPUT.bam OUTPUT.bam\n"); return 2; }
	agpu_sorted_bam_info info;
	if (ahost_sorted_bam_file_level(argv[1], argv[2], 1, &info) != 0) { fprintf(stderr, "ERROR: %s\n", ahost_last_error()); return 1; }
	printf("%llu records, %llu bytes in %llu bytes of blocks\n", (unsigned long long) info.records, (unsigned long long) info.uncompressed_bytes, (unsigned long long) info.file_bytes);
	uint32_t state = 12345, failures = 0, cases = 0;
	for (uint32_t round = 0; round < 4000; ++round) {
		const bool code_lengths = round % 2 == 1;
		const uint32_t n = code_lengths ? agpu::DFO_CL : agpu::DFO_LL, limit = code_lengths ? 7 : 15;
		std::vector<uint32_t> count(n, 0);
		uint64_t a = 1, b = 1;
		for (uint32_t t = 0; t < n; ++t) {
			state = state * 1664525u + 1013904223u;
			const uint32_t kind = round % 8;
			if (kind < 2) { count[t] = (uint32_t) (a > 60000 ? 60000 : a); const uint64_t c = a + b; a = b; b = c; } // deeper than any limit
			else if (kind < 4) count[t] = (state >> 8) % 3 == 0 ? 0 : 1u << ((state >> 16) % 16);
			else count[t] = (state >> 12) % (1 + round % 500);
			if ((state >> 28) == 0) count[t] = 0;
		}
		++cases;
		if (!complete(count, limit)) { ++failures; fprintf(stderr, "round %u: the code is not complete or exceeds %u bits\n", round, limit); }
	}
	printf("%u count tables, %u failures\n", cases, failures);
	return failures == 0 ? 0 : 1;
}
