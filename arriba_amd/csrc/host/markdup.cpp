// arriba_amd/csrc/host/markdup.cpp -- the host side of --mark-duplicates (include/arriba_host.h: ahost_markdup, ahost_sorted_bam_file_marked): arriba_amd/csrc/device/markdup_core.hpp
// stepped sequentially over records in host memory -- the comparator of agpu_markdup.hip, and what --host-ingest and the CPU tier run.  The steps are the device's: read names into
// the table of the core, the first primary record of every slot, end keys and scores, pairs sorted by (min end, max end, tie) and ends by (end key, mark, tie), the heads of the
// segments survive.  One byte per record comes out: MDUP_FLAG_MASK if the record leaves with bit 0x400, else 0.
#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <tuple>
#include <vector>
#include "arriba_host.h"
#include "../device/markdup_core.hpp"

namespace arriba {

void markdup_flags(const uint8_t* records, uint64_t size, std::vector<uint8_t>& flag, agpu_markdup_counts& counts) {
	using namespace agpu;
	memset(&counts, 0, sizeof(counts));
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
	flag.assign(n, 0);
	if (n == 0) return;
	// name ids and claims
	const uint64_t slots = support_table_slots(n);
	std::vector<unsigned long long> table(slots, 0);
	std::vector<uint32_t> name_id(n), slot_first(2 * n, MDUP_NONE);
	std::vector<uint8_t> input(n, 0);
	for (uint64_t r = 0; r < n; ++r) {
		const uint32_t id = name_id[r] = mdup_name_insert(table.data(), slots, records, size, offset.data(), (uint32_t) r, 64);
		const uint32_t flags = sbam_load16(records, offset[r] + 18);
		input[r] = (flags & 0x400u) != 0;
		if (id != MDUP_NONE && mdup_primary(flags)) { uint32_t& first = slot_first[2ull * id + mdup_slot(flags)]; first = std::min(first, (uint32_t) r); }
	}
	// ends, then pairs and fragments
	struct Pair { uint64_t low, high, tie; uint32_t template_of; };
	struct Entry { uint64_t key, mark, tie; uint32_t template_of; };
	std::vector<Pair> pairs; std::vector<Entry> entries;
	for (uint64_t t = 0; t < n; ++t) {
		if (name_id[t] != t) continue;
		++counts.templates;
		MdupEnd end[2];
		for (int k = 0; k < 2; ++k) { end[k].key = MDUP_NO_END; end[k].score = 0; if (slot_first[2 * t + k] != MDUP_NONE) end[k] = mdup_end(records, offset[slot_first[2 * t + k]], size); }
		const uint32_t rank = std::min(slot_first[2 * t], slot_first[2 * t + 1]);
		uint32_t score = 0;
		for (int k = 0; k < 2; ++k) if (end[k].key != MDUP_NO_END) score += end[k].score;
		if (end[0].key != MDUP_NO_END && end[1].key != MDUP_NO_END) {
			pairs.push_back({ std::min(end[0].key, end[1].key), std::max(end[0].key, end[1].key), mdup_tie(score, rank), (uint32_t) t });
			for (int k = 0; k < 2; ++k) entries.push_back({ end[k].key, 0, 0, (uint32_t) t });
		} else if (end[0].key != MDUP_NO_END || end[1].key != MDUP_NO_END)
			entries.push_back({ end[0].key != MDUP_NO_END ? end[0].key : end[1].key, 1, mdup_tie(score, rank), (uint32_t) t });
	}
	counts.pairs = pairs.size(); counts.fragments = entries.size() - 2 * pairs.size();
	// selection: whoever is not the head of its segment is a duplicate
	std::vector<uint8_t> duplicate_template(n, 0);
	std::sort(pairs.begin(), pairs.end(), [](const Pair& a, const Pair& b) { return std::tie(a.low, a.high, a.tie) < std::tie(b.low, b.high, b.tie); });
	for (size_t i = 1; i < pairs.size(); ++i) if (pairs[i].low == pairs[i - 1].low && pairs[i].high == pairs[i - 1].high) { duplicate_template[pairs[i].template_of] = 1; ++counts.duplicate_pairs; }
	std::stable_sort(entries.begin(), entries.end(), [](const Entry& a, const Entry& b) { return std::tie(a.key, a.mark, a.tie) < std::tie(b.key, b.mark, b.tie); });
	for (size_t i = 1; i < entries.size(); ++i) if (entries[i].mark != 0 && entries[i].key == entries[i - 1].key) { duplicate_template[entries[i].template_of] = 1; ++counts.duplicate_fragments; }
	for (uint64_t r = 0; r < n; ++r) {
		const bool out = name_id[r] != MDUP_NONE && duplicate_template[name_id[r]] != 0;
		flag[r] = out ? (uint8_t) MDUP_FLAG_MASK : (uint8_t) 0;
		if (out) ++counts.records_flagged;
		if (out != (input[r] != 0)) ++counts.records_changed;
	}
}

}
