// arriba_amd/csrc/host/depth.cpp -- the host side of --coverage (include/arriba_host.h: ahost_depth_*): the contigs of a header, and arriba_amd/csrc/device/depth_core.hpp stepped
// over records in host memory -- the comparator of agpu_depth.hip, and what --host-ingest and the CPU tier run.  The steps are the device's: marks into a difference array of
// LN + 1 slots per contig, one inclusive scan, the first and the last slot of every run of equal depth > 0, the lines.
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#include "arriba_host.h"
#include "../device/depth_core.hpp"

namespace arriba {

namespace {
uint32_t get32(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
struct StringPut { std::string& text; void operator()(uint8_t byte) { text.push_back((char) byte); } };
}

ahost_depth_contigs DepthContigs::view() const {
	ahost_depth_contigs v;
	v.n_ref = (uint32_t) length.size(); v.length = length.data(); v.names = names.data(); v.name_offset = name_offset.data();
	return v;
}

void depth_contigs_of(const uint8_t* input, size_t size, DepthContigs& contigs) {
	std::vector<std::string> names;
	contigs = DepthContigs();
	header_contigs(input, size, names, contigs.length);
	contigs.name_offset.push_back(0);
	for (size_t t = 0; t < names.size(); ++t) { contigs.names += names[t]; contigs.name_offset.push_back((uint32_t) contigs.names.size()); }
}

std::string depth_line_text(const std::string& name, uint32_t start, uint32_t end, uint32_t depth) {
	std::string line;
	StringPut put = { line };
	agpu::depth_line(name.data(), (uint32_t) name.size(), start, end, depth, put);
	if (line.size() != agpu::depth_line_bytes((uint32_t) name.size(), start, end, depth)) throw std::runtime_error("the line of a run does not have the length that was announced");
	return line;
}

void depth_track(const uint8_t* records, uint64_t size, const ahost_depth_contigs& contigs, std::string& text, agpu_depth_stats& stats) {
	using namespace agpu;
	const uint32_t n_ref = contigs.n_ref;
	std::vector<uint64_t> contig_offset((size_t) n_ref + 1, 0);
	for (uint32_t t = 0; t < n_ref; ++t) contig_offset[t + 1] = contig_offset[t] + contigs.length[t] + 1;
	const uint64_t slots = contig_offset[n_ref];
	std::vector<uint32_t> depth(slots, 0);
	memset(&stats, 0, sizeof(stats));
	text.clear();
	for (uint64_t at = 0; at < size; ) {
		if (size - at < 36 || (uint64_t) get32(records + at) + 4 > size - at || get32(records + at) < 32) throw std::runtime_error("failed to load alignments");
		const DepthRecord record = depth_parse(records, at, size, n_ref);
		at += (uint64_t) get32(records + at) + 4;
		if (!record.counts) continue;
		++stats.records;
		uint32_t* contig = depth.data() + contig_offset[record.ref];
		stats.segments += depth_cover(records, record.cigar_at, record.n_cigar, record.pos, contigs.length[record.ref], [contig](uint32_t begin, uint32_t end) { contig[begin] += 1u; contig[end] -= 1u; });
	}
	for (uint64_t g = 1; g < slots; ++g) depth[g] += depth[g - 1];
	StringPut put = { text };
	uint64_t first = 0; bool open = false;
	for (uint64_t g = 0; g < slots; ++g) {
		const uint32_t here = depth[g], before = g > 0 ? depth[g - 1] : 0u, after = g + 1 < slots ? depth[g + 1] : 0u;
		if (depth_head(before, here)) { if (open) throw std::runtime_error("a run of the coverage track begins inside another"); first = g; open = true; }
		if (depth_tail(here, after)) {
			if (!open) throw std::runtime_error("a run of the coverage track ends without a beginning");
			const uint32_t ref = depth_contig_of(contig_offset.data(), n_ref, first);
			const uint32_t start = (uint32_t) (first - contig_offset[ref]), end = (uint32_t) (g + 1 - contig_offset[ref]);
			depth_line(contigs.names + contigs.name_offset[ref], contigs.name_offset[ref + 1] - contigs.name_offset[ref], start, end, here, put);
			++stats.runs; stats.covered_positions += end - start; stats.aligned_bases += (uint64_t) (end - start) * here;
			if (here > stats.max_depth) stats.max_depth = here;
			open = false;
		}
	}
	if (open) throw std::runtime_error("a run of the coverage track is open behind the last contig");
	stats.text_bytes = text.size();
	stats.position_windows = slots > 0 ? 1 : 0; stats.text_windows = text.empty() ? 0 : 1;
}

}
