// arriba_amd/csrc/host/realign_split.cpp -- the host side of --realign-reads (include/arriba_host.h: ahost_realign_*): arriba_amd/csrc/device/realign_core.hpp stepped
// sequentially over records in host memory -- the comparator of agpu_realign.hip, and what --host-ingest and the CPU tier run.  The steps are the device's: the layout from the
// first record, read names into the table of markdup_core.hpp and the claims of the two slots (paired-end only), the role of every record, the verdict and the line lengths of
// every owner, and the lines in the order of the owners; and the header of the file of the kept templates from the contigs of the assembly.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>
#include "arriba_host.h"
#include "../device/realign_core.hpp"

namespace arriba {

namespace {
struct StringPut { std::string& text; void operator()(uint8_t byte) { text.push_back((char) byte); } };
uint32_t hash_bits_knob() { // (ARRIBA_REALIGN_HASH_BITS: the tests force names to collide)
	const char* knob = getenv("ARRIBA_REALIGN_HASH_BITS");
	if (knob == nullptr || knob[0] == 0) return 64;
	const long bits = atol(knob);
	return bits < 0 ? 0u : bits > 64 ? 64u : (uint32_t) bits;
}
}

void realign_plan_of(const Assembly& assembly, const uint8_t* header, size_t size, RealignPlan& plan) {
	std::vector<std::string> names; std::vector<uint32_t> lengths;
	if (size > 0) header_contigs(header, size, names, lengths);
	// the spelling of the input wins where it names a contig of the assembly: the lines of the kept templates carry it in RNAME and RNEXT
	std::map<std::string, size_t> input_by_name;
	for (size_t t = names.size(); t > 0; --t) input_by_name[remove_chr(names[t - 1])] = t - 1; // (the first of two references that differ by "chr" only)
	std::map<std::string, size_t> assembly_by_name;
	for (size_t c = 0; c < assembly.file_names.size(); ++c) assembly_by_name.insert(std::make_pair(remove_chr(assembly.file_names[c]), c));
	plan.in_assembly.assign(names.size(), 0);
	for (size_t t = 0; t < names.size(); ++t) plan.in_assembly[t] = assembly_by_name.count(remove_chr(names[t])) ? 1 : 0;
	plan.header = "@HD\tVN:1.4\tSO:unsorted\n";
	for (size_t c = 0; c < assembly.file_names.size(); ++c) {
		std::map<std::string, size_t>::const_iterator spelled = input_by_name.find(remove_chr(assembly.file_names[c]));
		plan.header += "@SQ\tSN:" + (spelled != input_by_name.end() ? names[spelled->second] : assembly.file_names[c]) + "\tLN:" + std::to_string(assembly.file_lengths[c]) + "\n";
	}
}

void realign_split_of(const uint8_t* in_assembly, const ahost_depth_contigs& contigs, const uint8_t* records, uint64_t size, bool want_kept, std::string& realign, std::string& kept, agpu_realign_stats& stats) {
	using namespace agpu;
	memset(&stats, 0, sizeof(stats));
	realign.clear(); kept.clear();
	std::vector<uint64_t> offset;
	for (uint64_t at = 0; at < size; ) {
		uint32_t block_size;
		if (size - at < 36) throw std::runtime_error("failed to load alignments");
		memcpy(&block_size, records + at, 4);
		if ((uint64_t) block_size + 4 > size - at || block_size < 32) throw std::runtime_error("failed to load alignments");
		offset.push_back(at);
		at += (uint64_t) block_size + 4;
	}
	const uint64_t n = offset.size();
	if (n >= 0xFFFFFFF0ull) throw std::runtime_error("more than 2^32-16 alignment records");
	stats.records = n;
	if (n == 0) return;
	const bool paired = (sbam_load16(records, offset[0] + 18) & 1u) != 0;
	stats.layout = paired ? 1 : 0;
	const RealignNames names = { contigs.names, contigs.name_offset, contigs.n_ref };
	// name ids and claims
	std::vector<uint32_t> name_id, slot_first;
	if (paired) {
		const uint64_t slots = support_table_slots(n);
		std::vector<unsigned long long> table(slots, 0);
		name_id.resize(n); slot_first.assign(2 * n, MDUP_NONE);
		const uint32_t hash_bits = hash_bits_knob();
		for (uint64_t r = 0; r < n; ++r) {
			const uint32_t id = name_id[r] = mdup_name_insert(table.data(), slots, records, size, offset.data(), (uint32_t) r, hash_bits);
			const uint32_t flags = sbam_load16(records, offset[r] + 18);
			if (id != MDUP_NONE && mdup_primary(flags)) { uint32_t& first = slot_first[2ull * id + mdup_slot(flags)]; first = std::min(first, (uint32_t) r); }
		}
	}
	// roles, verdicts and lines, in the order of the owners
	for (uint64_t r = 0; r < n; ++r) {
		const RealignRecord own = realign_parse(records, offset[r], size, names.n_ref);
		if (!own.valid || (paired && name_id[r] == MDUP_NONE)) throw std::runtime_error("failed to load alignments (a record is cut short, has no name or names a reference the header does not have)");
		const uint32_t first0 = paired ? slot_first[2ull * name_id[r]] : MDUP_NONE, first1 = paired ? slot_first[2ull * name_id[r] + 1] : MDUP_NONE;
		const uint32_t role = realign_role(own.flag, paired, (uint32_t) r, first0, first1);
		if (role == REALIGN_ROLE_DROPPED) { ++stats.dropped_secondary; continue; }
		if (role == REALIGN_ROLE_EXTRA) { ++stats.extra; continue; }
		if (role == REALIGN_ROLE_ORPHAN) { ++stats.templates; ++stats.orphans; continue; }
		if (role == REALIGN_ROLE_MATE) continue;
		RealignRecord mate = own;
		if (paired) mate = realign_parse(records, offset[first1], size, names.n_ref);
		if (!mate.valid) throw std::runtime_error("failed to load alignments (a record is cut short, has no name or names a reference the header does not have)");
		const RealignVerdict verdict = realign_verdict(records, own, mate, paired, in_assembly, names);
		if (verdict.bytes > 0xFFFFFFFFull) throw std::runtime_error("failed to load alignments (the lines of a template exceed 4 GiB)");
		++stats.templates; stats.placeholder_cigar += verdict.placeholders;
		const bool to_realign = verdict.file == REALIGN_FILE_REALIGN;
		(to_realign ? stats.realign_templates : stats.kept_templates) += 1;
		(to_realign ? stats.realign_bytes : stats.kept_bytes) += verdict.bytes;
		if (!to_realign && !want_kept) continue;
		std::string& text = to_realign ? realign : kept;
		const size_t before = text.size();
		StringPut put = { text };
		realign_line(records, own, names, put);
		if (paired) realign_line(records, mate, names, put);
		if (text.size() - before != verdict.bytes) throw std::runtime_error("the lines of a template do not have the length that was announced");
	}
}

}
