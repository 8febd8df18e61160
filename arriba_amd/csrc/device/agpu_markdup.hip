// arriba_amd/csrc/device/agpu_markdup.hip -- --mark-duplicates on the MI355X: one byte per record of the stream of the last ingest that says whether the record leaves the sorted
// file with bit 0x400 (include/arriba_gpu.h: agpu_sorted_bam_set_mark_duplicates, agpu_markdup_stats).  What decides the byte is markdup_core.hpp, which the host steps as well
// (arriba_amd/csrc/host/markdup.cpp); the rule is DESIGN.md 4.14.  Here are
//   markdup_name_kernel      one lane per record through ingest.record_offset: its QNAME into the open-addressing table (64-bit atomicCAS, every hit confirmed by the bytes), the id
//                            of its template -- the record whose name got there first --, and, if it is primary, its claim on its slot of the template: atomicMin of the record number
//   markdup_end_kernel       one lane per claimed slot: the CIGAR of that record (clips, reference length) and its qualities -> end key and score; no other record reads its qualities
//   markdup_template_kernel  one lane per template: pairs (two 64-bit key words, a tie word, two marked entries in the array of ends) and fragments (one entry), placed by
//                            wavefront-aggregated counters; the order of the arrays does not matter, the sorts below are total
//   rocPRIM radix sorts, least significant word first, stable: pairs by (min end, max end, tie), ends by (end key, mark, tie); markdup_gather_kernel between the passes
//   markdup_pair_kernel / markdup_entry_kernel   heads of segments by neighbour compares: whoever is not the head of its segment is a duplicate (entries of pairs sort in front of the
//                            fragments of their end key, so a fragment beside a pair never is a head) -> one byte per template
//   markdup_flag_kernel      one lane per record: the byte of its template -> "markdup.flag", the two counts of records
// The stream is only read.  Integer work bound by the dependent loads in front of a record's bytes and by the sorts; no MFMA, no LDS.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <rocprim/rocprim.hpp>
#define AGPU_OPTION "--mark-duplicates"
#include "resident_stream.hpp"
#include "device_utils.hpp"
#include "markdup_core.hpp"

using namespace agpu;

namespace {

enum { COUNT_TEMPLATES = 0, COUNT_PAIRS = 1, COUNT_ENTRIES = 2, COUNT_DUPLICATE_PAIRS = 3, COUNT_DUPLICATE_FRAGMENTS = 4, COUNT_FLAGGED = 5, COUNT_CHANGED = 6, COUNT_WORDS = 8 }; // 64-bit words

// Every lane of the wavefront calls it: room for `amount` items of this lane behind *counter, one atomic per wavefront; returns where the lane's items begin
__device__ __forceinline__ uint64_t wave_reserve(unsigned long long* counter, uint32_t amount) {
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t inclusive = amount;
	for (int distance = 1; distance < 64; distance <<= 1) { const uint32_t other = __shfl_up(inclusive, distance); if (lane >= (uint32_t) distance) inclusive += other; }
	const uint32_t total = __shfl(inclusive, 63);
	unsigned long long base = 0;
	if (lane == 63 && total != 0) base = atomicAdd(counter, (unsigned long long) total);
	base = __shfl(base, 63);
	return base + inclusive - amount;
}
__device__ __forceinline__ void wave_count(unsigned long long* counter, uint32_t mine) {
	unsigned long long sum = mine;
	for (int offset = 32; offset > 0; offset >>= 1) sum += __shfl_down(sum, offset);
	if ((threadIdx.x & 63u) == 0 && sum != 0) atomicAdd(counter, sum);
}

// flag[r]: 2 if the input carries 0x400 (markdup_flag_kernel reads it and writes the byte of the output)
__global__ void __launch_bounds__(BLOCK) markdup_name_kernel(const uint8_t* __restrict__ stream, uint64_t stream_size, const uint64_t* __restrict__ record_offset, uint64_t n, unsigned long long* table, uint64_t slots,
		uint32_t hash_bits, uint32_t* name_id, uint32_t* slot_first, uint8_t* flag) {
	const uint64_t r = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (r >= n) return;
	uint32_t id = MDUP_NONE; uint8_t input = 0;
	const uint64_t at = record_offset[r];
	if (at + 36 <= stream_size) {
		id = mdup_name_insert(table, slots, stream, stream_size, record_offset, (uint32_t) r, hash_bits);
		const uint32_t flags = sbam_load16(stream, at + 18);
		if (flags & 0x400u) input = 2;
		if (id != MDUP_NONE && mdup_primary(flags)) atomicMin(&slot_first[2ull * id + mdup_slot(flags)], (uint32_t) r);
	}
	name_id[r] = id; flag[r] = input;
}

// slot `first + lane` of the 2 n slots: key and score of the record that claimed it
__global__ void __launch_bounds__(BLOCK) markdup_end_kernel(const uint8_t* __restrict__ stream, uint64_t stream_size, const uint64_t* __restrict__ record_offset, const uint32_t* __restrict__ slot_first, uint64_t n_slots, uint64_t first,
		uint64_t* end_key, uint32_t* end_score) {
	const uint64_t s = first + (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (s >= n_slots) return;
	const uint32_t r = slot_first[s];
	MdupEnd end; end.key = MDUP_NO_END; end.score = 0;
	if (r != MDUP_NONE) end = mdup_end(stream, record_offset[r], stream_size);
	end_key[s] = end.key; end_score[s] = end.score;
}

struct PairArrays { uint64_t* key_low; uint64_t* key_high; uint64_t* tie; uint32_t* template_of; };
struct EntryArrays { uint64_t* key; uint64_t* mark; uint64_t* tie; uint32_t* template_of; }; // mark: 0 an end of a pair, 1 a fragment

// One lane per record: record t is a template if it is the id of its own name.  No lane leaves before the last wave_reserve.
__global__ void __launch_bounds__(BLOCK) markdup_template_kernel(const uint32_t* __restrict__ name_id, const uint32_t* __restrict__ slot_first, const uint64_t* __restrict__ end_key, const uint32_t* __restrict__ end_score, uint64_t n,
		PairArrays pairs, EntryArrays entries, unsigned long long* counters) {
	const uint64_t t = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	const bool is_template = t < n && name_id[t] == (uint32_t) t;
	uint64_t key0 = MDUP_NO_END, key1 = MDUP_NO_END; uint32_t score = 0, rank = MDUP_NONE;
	if (is_template) {
		key0 = end_key[2 * t]; key1 = end_key[2 * t + 1];
		if (key0 != MDUP_NO_END) score += end_score[2 * t];
		if (key1 != MDUP_NO_END) score += end_score[2 * t + 1];
		const uint32_t first0 = slot_first[2 * t], first1 = slot_first[2 * t + 1];
		rank = first0 < first1 ? first0 : first1;
	}
	const bool pair = key0 != MDUP_NO_END && key1 != MDUP_NO_END, fragment = !pair && (key0 != MDUP_NO_END || key1 != MDUP_NO_END);
	wave_count(&counters[COUNT_TEMPLATES], is_template ? 1u : 0u);
	const uint64_t p = wave_reserve(&counters[COUNT_PAIRS], pair ? 1u : 0u);
	const uint64_t e = wave_reserve(&counters[COUNT_ENTRIES], pair ? 2u : fragment ? 1u : 0u);
	if (pair) {
		pairs.key_low[p] = key0 < key1 ? key0 : key1; pairs.key_high[p] = key0 < key1 ? key1 : key0; pairs.tie[p] = mdup_tie(score, rank); pairs.template_of[p] = (uint32_t) t;
		entries.key[e] = key0; entries.key[e + 1] = key1; entries.mark[e] = 0; entries.mark[e + 1] = 0; entries.tie[e] = 0; entries.tie[e + 1] = 0; entries.template_of[e] = (uint32_t) t; entries.template_of[e + 1] = (uint32_t) t;
	} else if (fragment) {
		entries.key[e] = key0 != MDUP_NO_END ? key0 : key1; entries.mark[e] = 1; entries.tie[e] = mdup_tie(score, rank); entries.template_of[e] = (uint32_t) t;
	}
}

__global__ void __launch_bounds__(BLOCK) markdup_identity_kernel(uint32_t* order, uint64_t count) {
	const uint64_t i = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (i < count) order[i] = (uint32_t) i;
}
__global__ void __launch_bounds__(BLOCK) markdup_gather_kernel(const uint64_t* __restrict__ words, const uint32_t* __restrict__ order, uint64_t count, uint64_t* out) {
	const uint64_t i = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (i < count) out[i] = words[order[i]];
}

// Pair order[i] of the sorted pairs (key_low_sorted[i] is its low key): the head of a segment of equal (low, high) survives -- it has the highest score, then the lowest rank
__global__ void __launch_bounds__(BLOCK) markdup_pair_kernel(const uint64_t* __restrict__ key_low_sorted, const uint64_t* __restrict__ key_high, const uint32_t* __restrict__ order, const uint32_t* __restrict__ template_of, uint64_t count,
		uint8_t* duplicate_template, unsigned long long* counters) {
	const uint64_t i = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	uint32_t duplicate = 0;
	if (i < count) {
		const uint32_t mine = order[i];
		if (i > 0 && key_low_sorted[i] == key_low_sorted[i - 1] && key_high[mine] == key_high[order[i - 1]]) { duplicate = 1; duplicate_template[template_of[mine]] = 1; }
	}
	wave_count(&counters[COUNT_DUPLICATE_PAIRS], duplicate);
}

// Entry order[i] of the sorted ends: a fragment that is not the head of the segment of its key has a pair on its end, or a better fragment, in front of it
__global__ void __launch_bounds__(BLOCK) markdup_entry_kernel(const uint64_t* __restrict__ key_sorted, const uint64_t* __restrict__ mark, const uint32_t* __restrict__ order, const uint32_t* __restrict__ template_of, uint64_t count,
		uint8_t* duplicate_template, unsigned long long* counters) {
	const uint64_t i = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	uint32_t duplicate = 0;
	if (i < count) {
		const uint32_t mine = order[i];
		if (mark[mine] != 0 && i > 0 && key_sorted[i] == key_sorted[i - 1]) { duplicate = 1; duplicate_template[template_of[mine]] = 1; }
	}
	wave_count(&counters[COUNT_DUPLICATE_FRAGMENTS], duplicate);
}

__global__ void __launch_bounds__(BLOCK) markdup_flag_kernel(const uint32_t* __restrict__ name_id, const uint8_t* __restrict__ duplicate_template, uint64_t n, uint8_t* flag, unsigned long long* counters) {
	const uint64_t r = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	uint32_t flagged = 0, changed = 0;
	if (r < n) {
		const uint32_t id = name_id[r];
		const bool out = id != MDUP_NONE && duplicate_template[id] != 0, in = flag[r] != 0;
		flag[r] = out ? (uint8_t) MDUP_FLAG_MASK : (uint8_t) 0;
		flagged = out ? 1u : 0u; changed = out != in ? 1u : 0u;
	}
	wave_count(&counters[COUNT_FLAGGED], flagged);
	wave_count(&counters[COUNT_CHANGED], changed);
}

struct SortWord { const uint64_t* words; unsigned int end_bit; };

// `count` items ordered by their words, words[0] the least significant: one stable radix sort per word over (the word gathered in the order so far, the order).  order_out: the
// items in their order; sorted_out: the most significant word in that order.  Both point into "markdup.order*" / "markdup.sort*" of the state.
int sort_by_words(agpu_ctx* ctx, const SortWord* words, int n_words, uint64_t count, const char* what, const uint32_t*& order_out, const uint64_t*& sorted_out) {
	MarkdupState& state = ctx->markdup;
	hipStream_t s = ctx->stream;
	DeviceBuffer& gathered = state.buffer("markdup.sort_in"); DeviceBuffer& sorted = state.buffer("markdup.sort_out"); DeviceBuffer& temporary_storage = state.buffer("markdup.rocprim");
	DeviceBuffer* order[2] = { &state.buffer("markdup.order0"), &state.buffer("markdup.order1") };
	ALLOC(gathered, count * 8); ALLOC(sorted, count * 8); ALLOC(*order[0], count * 4); ALLOC(*order[1], count * 4);
	markdup_identity_kernel<<<grid_for(count), BLOCK, 0, s>>>(order[0]->as<uint32_t>(), count);
	for (int w = 0; w < n_words; ++w) {
		{ KernelTimer timer(ctx, "markdup_gather_kernel", count * 20);
		  markdup_gather_kernel<<<grid_for(count), BLOCK, 0, s>>>(words[w].words, order[w & 1]->as<uint32_t>(), count, gathered.as<uint64_t>()); }
		size_t temporary = 0;
		HIP_CHECK(rocprim::radix_sort_pairs(nullptr, temporary, gathered.as<uint64_t>(), sorted.as<uint64_t>(), order[w & 1]->as<uint32_t>(), order[(w + 1) & 1]->as<uint32_t>(), (size_t) count, 0u, words[w].end_bit, s));
		if (temporary > temporary_storage.capacity) { HIP_CHECK(hipStreamSynchronize(s)); ALLOC(temporary_storage, temporary); }
		{ KernelTimer timer(ctx, what, count * 24);
		  HIP_CHECK(rocprim::radix_sort_pairs(temporary_storage.ptr, temporary, gathered.as<uint64_t>(), sorted.as<uint64_t>(), order[w & 1]->as<uint32_t>(), order[(w + 1) & 1]->as<uint32_t>(), (size_t) count, 0u, words[w].end_bit, s)); }
	}
	order_out = order[n_words & 1]->as<uint32_t>(); sorted_out = sorted.as<uint64_t>();
	return AGPU_OK;
}

int find(agpu_ctx* ctx, const ResidentStream& resident, hipEvent_t* events) {
	MarkdupState& state = ctx->markdup;
	hipStream_t s = ctx->stream;
	const uint64_t size = resident.stream_size, n = resident.records;
	const uint8_t* stream = resident.stream;
	const uint64_t* record_offset = resident.record_offset;
	uint64_t peak = 0;
	DeviceBuffer& flag = state.buffer("markdup.flag");
	ALLOC(flag, std::max<uint64_t>(n, 1));
	HIP_CHECK(hipEventRecord(events[0], s));
	if (n == 0) { for (int k = 1; k < 4; ++k) HIP_CHECK(hipEventRecord(events[k], s)); state.counts.peak_bytes = state.allocated(); return AGPU_OK; }
	DeviceBuffer& counters = state.buffer("markdup.counters"); DeviceBuffer& name_id = state.buffer("markdup.name_id"); DeviceBuffer& slot_first = state.buffer("markdup.slot_first");
	ALLOC(counters, COUNT_WORDS * 8); ALLOC(name_id, n * 4); ALLOC(slot_first, n * 8);
	HIP_CHECK(hipMemsetAsync(counters.ptr, 0, COUNT_WORDS * 8, s));
	HIP_CHECK(hipMemsetAsync(slot_first.ptr, 0xFF, n * 8, s));
	{ // name ids and claims
		DeviceBuffer& table = state.buffer("markdup.table");
		const uint64_t slots = support_table_slots(n);
		ALLOC(table, slots * 8);
		HIP_CHECK(hipMemsetAsync(table.ptr, 0, slots * 8, s));
		peak = std::max(peak, state.allocated());
		{ KernelTimer timer(ctx, "markdup_name_kernel", n * 64 + slots * 8);
		  markdup_name_kernel<<<grid_for(n), BLOCK, 0, s>>>(stream, size, record_offset, n, table.as<unsigned long long>(), slots, hash_bits_knob("ARRIBA_MARKDUP_HASH_BITS"), name_id.as<uint32_t>(), slot_first.as<uint32_t>(), flag.as<uint8_t>()); }
		HIP_CHECK(hipEventRecord(events[1], s));
		HIP_CHECK(hipStreamSynchronize(s));
		table.release();
	}
	DeviceBuffer& end_key = state.buffer("markdup.end_key"); DeviceBuffer& end_score = state.buffer("markdup.end_score");
	ALLOC(end_key, n * 16); ALLOC(end_score, n * 8);
	{ KernelTimer timer(ctx, "markdup_end_kernel", n * 24 + size / 2);
	  for_each_launch_piece(2 * n, [&](uint64_t first, unsigned int grid) { // (one lane per slot: two slots per record)
		markdup_end_kernel<<<grid, BLOCK, 0, s>>>(stream, size, record_offset, slot_first.as<uint32_t>(), 2 * n, first, end_key.as<uint64_t>(), end_score.as<uint32_t>()); }); }
	HIP_CHECK(hipEventRecord(events[2], s));
	// pairs and fragments: a pair has two records of its own and a fragment one, so there are at most n / 2 pairs and n entries
	const uint64_t pair_room = n / 2 + 1, entry_room = n + 1;
	DeviceBuffer& pair_low = state.buffer("markdup.pair_low"); DeviceBuffer& pair_high = state.buffer("markdup.pair_high"); DeviceBuffer& pair_tie = state.buffer("markdup.pair_tie"); DeviceBuffer& pair_template = state.buffer("markdup.pair_template");
	DeviceBuffer& entry_key = state.buffer("markdup.entry_key"); DeviceBuffer& entry_mark = state.buffer("markdup.entry_mark"); DeviceBuffer& entry_tie = state.buffer("markdup.entry_tie"); DeviceBuffer& entry_template = state.buffer("markdup.entry_template");
	ALLOC(pair_low, pair_room * 8); ALLOC(pair_high, pair_room * 8); ALLOC(pair_tie, pair_room * 8); ALLOC(pair_template, pair_room * 4);
	ALLOC(entry_key, entry_room * 8); ALLOC(entry_mark, entry_room * 8); ALLOC(entry_tie, entry_room * 8); ALLOC(entry_template, entry_room * 4);
	peak = std::max(peak, state.allocated());
	const PairArrays pairs = { pair_low.as<uint64_t>(), pair_high.as<uint64_t>(), pair_tie.as<uint64_t>(), pair_template.as<uint32_t>() };
	const EntryArrays entries = { entry_key.as<uint64_t>(), entry_mark.as<uint64_t>(), entry_tie.as<uint64_t>(), entry_template.as<uint32_t>() };
	{ KernelTimer timer(ctx, "markdup_template_kernel", n * 40);
	  markdup_template_kernel<<<grid_for(n), BLOCK, 0, s>>>(name_id.as<uint32_t>(), slot_first.as<uint32_t>(), end_key.as<uint64_t>(), end_score.as<uint32_t>(), n, pairs, entries, counters.as<unsigned long long>()); }
	unsigned long long host_counters[COUNT_WORDS];
	HIP_CHECK(hipMemcpyAsync(host_counters, counters.ptr, sizeof(host_counters), hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	const uint64_t n_pairs = host_counters[COUNT_PAIRS], n_entries = host_counters[COUNT_ENTRIES];
	if (n_pairs >= pair_room || n_entries >= entry_room || n_entries < 2 * n_pairs) { set_last_error("--mark-duplicates: more pairs or fragments than the records of the stream allow"); return AGPU_ERR_DEVICE; }
	end_key.release(); end_score.release(); slot_first.release();
	DeviceBuffer& duplicate_template = state.buffer("markdup.duplicate_template");
	ALLOC(duplicate_template, n);
	HIP_CHECK(hipMemsetAsync(duplicate_template.ptr, 0, n, s));
	const uint32_t* order = nullptr; const uint64_t* sorted = nullptr;
	if (n_pairs > 0) {
		const SortWord words[3] = { { pairs.tie, 64 }, { pairs.key_high, 64 }, { pairs.key_low, 64 } };
		TRY(sort_by_words(ctx, words, 3, n_pairs, "markdup rocprim::radix_sort_pairs(pairs)", order, sorted));
		peak = std::max(peak, state.allocated());
		KernelTimer timer(ctx, "markdup_pair_kernel", n_pairs * 32);
		markdup_pair_kernel<<<grid_for(n_pairs), BLOCK, 0, s>>>(sorted, pairs.key_high, order, pairs.template_of, n_pairs, duplicate_template.as<uint8_t>(), counters.as<unsigned long long>());
	}
	if (n_entries > 0) {
		const SortWord words[3] = { { entries.tie, 64 }, { entries.mark, 1 }, { entries.key, 64 } };
		TRY(sort_by_words(ctx, words, 3, n_entries, "markdup rocprim::radix_sort_pairs(ends)", order, sorted));
		peak = std::max(peak, state.allocated());
		KernelTimer timer(ctx, "markdup_entry_kernel", n_entries * 32);
		markdup_entry_kernel<<<grid_for(n_entries), BLOCK, 0, s>>>(sorted, entries.mark, order, entries.template_of, n_entries, duplicate_template.as<uint8_t>(), counters.as<unsigned long long>());
	}
	{ KernelTimer timer(ctx, "markdup_flag_kernel", n * 7);
	  markdup_flag_kernel<<<grid_for(n), BLOCK, 0, s>>>(name_id.as<uint32_t>(), duplicate_template.as<uint8_t>(), n, flag.as<uint8_t>(), counters.as<unsigned long long>()); }
	HIP_CHECK(hipEventRecord(events[3], s));
	HIP_CHECK(hipMemcpyAsync(host_counters, counters.ptr, sizeof(host_counters), hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	agpu_markdup_counts& counts = state.counts;
	counts.templates = host_counters[COUNT_TEMPLATES]; counts.pairs = n_pairs; counts.fragments = n_entries - 2 * n_pairs;
	counts.duplicate_pairs = host_counters[COUNT_DUPLICATE_PAIRS]; counts.duplicate_fragments = host_counters[COUNT_DUPLICATE_FRAGMENTS];
	counts.records_flagged = host_counters[COUNT_FLAGGED]; counts.records_changed = host_counters[COUNT_CHANGED];
	counts.peak_bytes = peak;
	for (int k = 0; k < 3; ++k) { float ms = 0; if (hipEventElapsedTime(&ms, events[k], events[k + 1]) == hipSuccess) counts.seconds[k] = ms / 1000.0; }
	return AGPU_OK;
}

}

namespace agpu {

int markdup_find(agpu_ctx* ctx, const ResidentStream& stream) {
	MarkdupState& state = ctx->markdup;
	memset(&state.counts, 0, sizeof(state.counts));
	hipEvent_t events[4] = { nullptr, nullptr, nullptr, nullptr };
	for (int k = 0; k < 4; ++k) if (hipEventCreate(&events[k]) != hipSuccess) { for (int j = 0; j < k; ++j) (void) hipEventDestroy(events[j]); set_last_error("--mark-duplicates: hipEventCreate failed"); return AGPU_ERR_DEVICE; }
	const int status = find(ctx, stream, events);
	if (status != AGPU_OK) (void) hipStreamSynchronize(ctx->stream); // (nothing of a failed search is in flight when its buffers go)
	for (int k = 0; k < 4; ++k) (void) hipEventDestroy(events[k]);
	if (status == AGPU_OK) state.release_all_but("markdup.flag"); else state.release_all();
	collect_kernel_samples(ctx);
	return status;
}

}

extern "C" {

int agpu_sorted_bam_set_mark_duplicates(agpu_ctx* ctx, int on) {
	if (!ctx) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	if (ctx->sorted_bam_active) { set_last_error("agpu_sorted_bam_set_mark_duplicates: it comes before agpu_sorted_bam_begin"); return AGPU_ERR_INVALID; }
	ctx->markdup.next = on != 0;
	return AGPU_OK;
}

int agpu_markdup_stats(agpu_ctx* ctx, agpu_markdup_counts* counts) {
	if (!ctx || !counts) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	*counts = ctx->markdup.counts;
	return AGPU_OK;
}

int agpu_markdup_allocated_bytes(agpu_ctx* ctx, uint64_t* bytes) {
	if (!ctx || !bytes) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	*bytes = ctx->markdup.allocated();
	return AGPU_OK;
}

}
