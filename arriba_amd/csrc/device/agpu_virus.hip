// arriba_amd/csrc/device/agpu_virus.hip -- --virus-expression on the MI355X: the counters of the reference's scripts/quantify_virus_expression.sh from the record stream of the
// last ingest (include/arriba_gpu.h: agpu_virus_expression).  What decides a number is virus_core.hpp, which the host steps as well (arriba_amd/csrc/host/virus.cpp); here are
//   virus_scan_kernel        one lane per record through ingest.record_offset (the access pattern of sorted_bam_key_kernel): flag and refID, `total` from ballots with one add
//                            per workgroup, refID -> virus slot through a table, the CIGAR test, the candidates compacted with one cursor bump per workgroup
//   virus_candidate_kernel   THE HOT PATH of a virus-rich sample, one lane per candidate: the tandem test on the packed SEQ (three positions of history in registers), reads[slot]
//                            (one add per wavefront when its lanes agree on the slot), coverage as atomicOr of word masks into the bitmap of the slot, the number of its 12-mers
//   virus_kmer_emit_kernel   one lane per 12-mer of a window of the emission: its candidate by binary search in the scanned counts, 48 bits of nibbles above 16 bits of slot
//   rocPRIM radix sort of the set so far with the window behind it, virus_head_kernel + exclusive scan + virus_compact_kernel: the set without duplicates, in the order k-mer, slot
//   virus_kmer_count_kernel, virus_shared_kernel   per key of the final set: the histogram by slot; every other slot of its run of equal k-mers adds one to the matrix
//   virus_covered_kernel     one wavefront per slot: the bits of its bitmap
// Integer and byte work: the scan is bound by the latency of the two dependent loads in front of a record's words, the rest by atomics and the sort; no MFMA, no LDS beyond a few words.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <rocprim/rocprim.hpp>
#define AGPU_OPTION "--virus-expression"
#include "resident_stream.hpp"
#include "device_utils.hpp"
#include "virus_core.hpp"

using namespace agpu;

namespace {

const uint64_t DEFAULT_KMER_WINDOW = 1ull << 25; // keys of one emission: 256 MiB

enum { COUNTER_TOTAL = 0, COUNTER_CANDIDATES = 1, COUNTER_WORDS = 2 }; // 64-bit words; the cursor of the candidates is the low half of its word

// table[slot] += 1 for the lanes that are `on`: one add for those that agree with the first of them.  Every lane of the wavefront calls it.
__device__ __forceinline__ void wave_count(unsigned long long* table, uint32_t slot, bool on) {
	const unsigned long long mask = __ballot(on);
	if (mask == 0) return;
	const int leader = __ffsll(mask) - 1;
	const uint32_t first = (uint32_t) __shfl((int) slot, leader);
	const unsigned long long same = __ballot(on && slot == first);
	if (!on) return;
	if (slot != first) atomicAdd(&table[slot], 1ull);
	else if ((int) (threadIdx.x & 63) == leader) atomicAdd(&table[first], (unsigned long long) __popcll(same));
}

__global__ void __launch_bounds__(BLOCK) virus_scan_kernel(const uint8_t* __restrict__ stream, uint64_t stream_size, const uint64_t* __restrict__ record_offset, uint64_t n, const uint32_t* __restrict__ slot_of_ref, uint32_t n_ref,
		unsigned long long* counters, uint32_t* candidates) {
	__shared__ uint32_t wave_offset[BLOCK / 64], block_base, mapped_records;
	const uint64_t r = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (threadIdx.x == 0) mapped_records = 0;
	bool mapped = false, candidate = false;
	if (r < n) {
		const uint64_t at = record_offset[r];
		if (at < stream_size) {
			const VirusRecord record = virus_parse(stream, at, stream_size);
			mapped = virus_mapped(record.flag) && at + 36 <= stream_size;
			if (mapped && virus_flag_ok(record.flag) && record.whole && record.ref >= 0 && (uint32_t) record.ref < n_ref && slot_of_ref[record.ref] != VIRUS_NO_SLOT)
				candidate = virus_cigar_ok(stream, record.cigar_at, record.n_cigar);
		}
	}
	__syncthreads();
	const unsigned long long ballot = __ballot(mapped);
	if ((threadIdx.x & 63) == 0 && ballot != 0) atomicAdd(&mapped_records, (uint32_t) __popcll(ballot));
	const uint32_t place = block_append<BLOCK>(candidate ? 1u : 0u, (uint32_t*) &counters[COUNTER_CANDIDATES], wave_offset, &block_base); // (its barriers order mapped_records as well)
	if (candidate) candidates[place] = (uint32_t) r;
	if (threadIdx.x == 0 && mapped_records != 0) atomicAdd(&counters[COUNTER_TOTAL], (unsigned long long) mapped_records);
}

struct BitmapOr { uint32_t* words; __device__ __forceinline__ void operator()(uint32_t word, uint32_t mask) const { atomicOr(&words[word], mask); } };

// One lane per candidate; lane m writes the 0 that ends the counts.  seq_at / slot: kept for the emission, which then has no need of the record's head.
__global__ void __launch_bounds__(BLOCK) virus_candidate_kernel(const uint8_t* __restrict__ stream, uint64_t stream_size, const uint64_t* __restrict__ record_offset, const uint32_t* __restrict__ candidates, uint64_t m,
		const uint32_t* __restrict__ slot_of_ref, const uint32_t* __restrict__ viral_length, const uint64_t* __restrict__ bitmap_offset, uint32_t* bitmap, unsigned long long* reads,
		uint32_t* kmers, uint64_t* candidate_seq, uint32_t* candidate_slot) {
	const uint64_t c = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	bool passes = false; uint32_t slot = 0;
	if (c < m) {
		const uint64_t at = record_offset[candidates[c]];
		const VirusRecord record = virus_parse(stream, at, stream_size); // (a candidate: whole, on a viral reference, with a CIGAR of M, N and X)
		slot = slot_of_ref[record.ref];
		passes = !virus_tandem(stream + record.seq_at, record.l_seq);
		if (passes) {
			const BitmapOr mark = { bitmap + bitmap_offset[slot] };
			virus_cover(stream, record.cigar_at, record.n_cigar, record.pos, viral_length[slot], mark);
		}
		kmers[c] = passes ? virus_kmer_count(record.l_seq) : 0;
		candidate_seq[c] = record.seq_at; candidate_slot[c] = slot;
	} else if (c == m) kmers[c] = 0;
	wave_count(reads, slot, passes);
}

// key first + j of the emission, j < count: the candidate c with kmer_offset[c] <= key < kmer_offset[c + 1] (kmer_offset[m] = all keys)
__global__ void __launch_bounds__(BLOCK) virus_kmer_emit_kernel(const uint8_t* __restrict__ stream, const uint64_t* __restrict__ kmer_offset, uint64_t m, const uint64_t* __restrict__ candidate_seq, const uint32_t* __restrict__ candidate_slot,
		uint64_t first, uint64_t count, uint64_t* out) {
	const uint64_t j = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (j >= count) return;
	const uint64_t key = first + j;
	uint64_t low = 0, high = m; // kmer_offset[low] <= key < kmer_offset[high]
	while (high - low > 1) { const uint64_t middle = low + (high - low) / 2; if (kmer_offset[middle] <= key) low = middle; else high = middle; }
	out[j] = virus_kmer_key(stream + candidate_seq[low], (uint32_t) (key - kmer_offset[low]), candidate_slot[low]);
}

// heads[i] = 1 if sorted[i] is the first of its value; one entry more (0) for the scan that gives the number of distinct keys
__global__ void __launch_bounds__(BLOCK) virus_head_kernel(const uint64_t* __restrict__ sorted, uint64_t n, uint32_t* heads) {
	const uint64_t i = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (i > n) return;
	heads[i] = i < n && (i == 0 || sorted[i] != sorted[i - 1]) ? 1u : 0u;
}
__global__ void __launch_bounds__(BLOCK) virus_compact_kernel(const uint64_t* __restrict__ sorted, const uint32_t* __restrict__ heads, const uint64_t* __restrict__ place, uint64_t n, uint64_t* out) {
	const uint64_t i = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (i < n && heads[i] != 0) out[place[i]] = sorted[i];
}

__global__ void __launch_bounds__(BLOCK) virus_kmer_count_kernel(const uint64_t* __restrict__ set, uint64_t n, unsigned long long* kmer_count) {
	const uint64_t i = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	const bool live = i < n;
	wave_count(kmer_count, live ? (uint32_t) (set[i] & 0xFFFFu) : 0u, live);
}

// One lane per key of the set: the other keys of its run of equal k-mers are the other viruses that have the k-mer.  dense_of_slot: the rank of a slot among those with reads
// (every slot of the set has reads).  A run is as long as there are related strains, so a lane walks a few keys; nearly all runs have one key and add nothing.
__global__ void __launch_bounds__(BLOCK) virus_shared_kernel(const uint64_t* __restrict__ set, uint64_t n, const uint32_t* __restrict__ dense_of_slot, uint32_t n_active, unsigned long long* shared) {
	const uint64_t i = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (i >= n) return;
	const uint64_t key = set[i], kmer = key >> 16;
	const uint64_t row = (uint64_t) dense_of_slot[key & 0xFFFFu] * n_active;
	for (uint64_t j = i; j-- > 0; ) { const uint64_t other = set[j]; if (other >> 16 != kmer) break; atomicAdd(&shared[row + dense_of_slot[other & 0xFFFFu]], 1ull); }
	for (uint64_t j = i + 1; j < n; ++j) { const uint64_t other = set[j]; if (other >> 16 != kmer) break; atomicAdd(&shared[row + dense_of_slot[other & 0xFFFFu]], 1ull); }
}

// One wavefront per slot (launched in chunks: `first` is the slot of the first wavefront)
__global__ void __launch_bounds__(BLOCK) virus_covered_kernel(const uint32_t* __restrict__ bitmap, const uint64_t* __restrict__ bitmap_offset, uint32_t n_viruses, unsigned long long* covered, uint32_t first) {
	const uint64_t v = first + ((uint64_t) blockIdx.x * BLOCK + threadIdx.x) / 64;
	if (v >= n_viruses) return;
	const uint32_t lane = threadIdx.x & 63;
	uint32_t bits = 0; // (a contig has fewer than 2^32 positions)
	for (uint64_t w = bitmap_offset[v] + lane; w < bitmap_offset[v + 1]; w += 64) bits += (uint32_t) __popc(bitmap[w]);
	for (int offset = 32; offset > 0; offset >>= 1) bits += __shfl_down(bits, offset);
	if (lane == 0) covered[v] = bits;
}

int run(agpu_ctx* ctx, const ResidentStream& resident, const int32_t* viral_ref, const uint32_t* viral_length, uint32_t n_viruses, uint32_t n_ref, agpu_virus_counters* out, hipEvent_t* marks, uint64_t& peak) {
	hipStream_t s = ctx->stream;
	VirusState& state = ctx->virus;
	const uint64_t size = resident.stream_size, n = resident.records;
	const uint8_t* stream = resident.stream;
	const uint64_t* record_offset = resident.record_offset;
	uint64_t window = DEFAULT_KMER_WINDOW;
	{ const char* knob = getenv("ARRIBA_VIRUS_KMER_WINDOW"); if (knob != nullptr && knob[0] != 0) window = std::max<uint64_t>(strtoull(knob, nullptr, 10), 1); }
	window = std::min<uint64_t>(window, 1ull << 31);
	struct Peak { VirusState& state; uint64_t& peak; void operator()() { peak = std::max(peak, state.allocated()); } } note = { state, peak };

	// the tables of the call
	std::vector<uint32_t> host_slot_of_ref(std::max<uint32_t>(n_ref, 1), VIRUS_NO_SLOT);
	std::vector<uint64_t> host_bitmap_offset((size_t) n_viruses + 1, 0);
	for (uint32_t v = 0; v < n_viruses; ++v) { host_slot_of_ref[viral_ref[v]] = v; host_bitmap_offset[v + 1] = host_bitmap_offset[v] + virus_bitmap_words(viral_length[v]); }
	const uint64_t bitmap_words = host_bitmap_offset[n_viruses];
	DeviceBuffer& slot_of_ref = state.buffer("virus.slot_of_ref"); DeviceBuffer& lengths = state.buffer("virus.length"); DeviceBuffer& bitmap_offset = state.buffer("virus.bitmap_offset"); DeviceBuffer& bitmap = state.buffer("virus.bitmap");
	DeviceBuffer& counters = state.buffer("virus.counters"); DeviceBuffer& per_virus = state.buffer("virus.per_virus"); DeviceBuffer& candidates = state.buffer("virus.candidates");
	const size_t slots = std::max<uint32_t>(n_viruses, 1);
	ALLOC(slot_of_ref, host_slot_of_ref.size() * 4); ALLOC(lengths, slots * 4); ALLOC(bitmap_offset, ((size_t) n_viruses + 1) * 8); ALLOC(bitmap, std::max<uint64_t>(bitmap_words, 1) * 4);
	ALLOC(counters, COUNTER_WORDS * 8); ALLOC(per_virus, 3 * slots * 8); ALLOC(candidates, std::max<uint64_t>(n, 1) * 4);
	note();
	unsigned long long* const reads = per_virus.as<unsigned long long>(), * const covered = reads + slots, * const kmer_count = covered + slots;
	HIP_CHECK(hipMemcpyAsync(slot_of_ref.ptr, host_slot_of_ref.data(), host_slot_of_ref.size() * 4, hipMemcpyHostToDevice, s));
	if (n_viruses > 0) HIP_CHECK(hipMemcpyAsync(lengths.ptr, viral_length, (size_t) n_viruses * 4, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(bitmap_offset.ptr, host_bitmap_offset.data(), host_bitmap_offset.size() * 8, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipStreamSynchronize(s)); // (the sources are pageable memory of this call)
	HIP_CHECK(hipMemsetAsync(bitmap.ptr, 0, std::max<uint64_t>(bitmap_words, 1) * 4, s));
	HIP_CHECK(hipMemsetAsync(counters.ptr, 0, COUNTER_WORDS * 8, s));
	HIP_CHECK(hipMemsetAsync(per_virus.ptr, 0, 3 * slots * 8, s));

	// 1. the scan
	HIP_CHECK(hipEventRecord(marks[0], s));
	if (n > 0) { KernelTimer timer(ctx, "virus_scan_kernel", n * 8 + n * 64);
	  virus_scan_kernel<<<grid_for(n), BLOCK, 0, s>>>(stream, size, record_offset, n, slot_of_ref.as<uint32_t>(), n_ref, counters.as<unsigned long long>(), candidates.as<uint32_t>()); }
	unsigned long long host_counters[COUNTER_WORDS] = { 0, 0 };
	HIP_CHECK(hipMemcpyAsync(host_counters, counters.ptr, sizeof(host_counters), hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipEventRecord(marks[1], s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	const uint64_t m = host_counters[COUNTER_CANDIDATES] & 0xFFFFFFFFull;
	if (m > n) { set_last_error("agpu_virus_expression: more candidates than records"); return AGPU_ERR_DEVICE; }

	// 2. per candidate
	uint64_t all_keys = 0;
	DeviceBuffer& kmers = state.buffer("virus.kmers"); DeviceBuffer& kmer_offset = state.buffer("virus.kmer_offset"); DeviceBuffer& candidate_seq = state.buffer("virus.candidate_seq"); DeviceBuffer& candidate_slot = state.buffer("virus.candidate_slot");
	if (m > 0) {
		ALLOC(kmers, (m + 1) * 4); ALLOC(kmer_offset, (m + 1) * 8); ALLOC(candidate_seq, m * 8); ALLOC(candidate_slot, m * 4);
		note();
		{ KernelTimer timer(ctx, "virus_candidate_kernel", m * 128);
		  virus_candidate_kernel<<<grid_for(m + 1), BLOCK, 0, s>>>(stream, size, record_offset, candidates.as<uint32_t>(), m, slot_of_ref.as<uint32_t>(), lengths.as<uint32_t>(), bitmap_offset.as<uint64_t>(), bitmap.as<uint32_t>(), reads,
			kmers.as<uint32_t>(), candidate_seq.as<uint64_t>(), candidate_slot.as<uint32_t>()); }
		TRY(with_temporary(ctx, state.buffer("virus.rocprim"), "virus rocprim::exclusive_scan(k-mers)", m * 12, [&](void* t, size_t& b) { return rocprim::exclusive_scan(t, b, kmers.as<uint32_t>(), kmer_offset.as<uint64_t>(), (uint64_t) 0, (size_t) m + 1, rocprim::plus<uint64_t>(), s); }));
		HIP_CHECK(hipMemcpyAsync(&all_keys, kmer_offset.as<uint64_t>() + m, 8, hipMemcpyDeviceToHost, s));
	}
	state.reads.assign(n_viruses, 0);
	if (n_viruses > 0) HIP_CHECK(hipMemcpyAsync(state.reads.data(), reads, (size_t) n_viruses * 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipEventRecord(marks[2], s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	state.active_slots.clear();
	std::vector<uint32_t> host_dense(slots, VIRUS_NO_SLOT);
	for (uint32_t v = 0; v < n_viruses; ++v) if (state.reads[v] > 0) { host_dense[v] = (uint32_t) state.active_slots.size(); state.active_slots.push_back(v); }
	const uint32_t n_active = (uint32_t) state.active_slots.size();

	// 3. the set of (k-mer, slot): the set so far at the front of `work`, a window of keys behind it, sorted, the first of every value kept
	uint64_t distinct = 0, rounds = 0;
	DeviceBuffer& work = state.buffer("virus.keys"); DeviceBuffer& sorted = state.buffer("virus.keys_sorted"); DeviceBuffer& heads = state.buffer("virus.heads"); DeviceBuffer& place = state.buffer("virus.place");
	for (uint64_t first = 0; first < all_keys; first += window, ++rounds) {
		const uint64_t count = std::min(window, all_keys - first), held = distinct + count;
		if (work.capacity < held * 8) { // the set moves to a larger buffer through `sorted`, whose keys nobody needs any more
			const uint64_t room = std::max(held, std::min(all_keys, distinct + 2 * window));
			if (distinct > 0) HIP_CHECK(hipMemcpyAsync(sorted.ptr, work.ptr, distinct * 8, hipMemcpyDeviceToDevice, s));
			HIP_CHECK(hipStreamSynchronize(s));
			ALLOC(work, room * 8);
			if (distinct > 0) HIP_CHECK(hipMemcpyAsync(work.ptr, sorted.ptr, distinct * 8, hipMemcpyDeviceToDevice, s));
			HIP_CHECK(hipStreamSynchronize(s));
			ALLOC(sorted, room * 8); ALLOC(heads, (room + 1) * 4); ALLOC(place, (room + 1) * 8);
			note();
		}
		{ KernelTimer timer(ctx, "virus_kmer_emit_kernel", count * 24);
		  virus_kmer_emit_kernel<<<grid_for(count), BLOCK, 0, s>>>(stream, kmer_offset.as<uint64_t>(), m, candidate_seq.as<uint64_t>(), candidate_slot.as<uint32_t>(), first, count, work.as<uint64_t>() + distinct); }
		TRY(with_temporary(ctx, state.buffer("virus.rocprim"), "virus rocprim::radix_sort_keys(k-mers)", held * 16, [&](void* t, size_t& b) { return rocprim::radix_sort_keys(t, b, work.as<uint64_t>(), sorted.as<uint64_t>(), (size_t) held, 0, 64, s); }));
		note();
		{ KernelTimer timer(ctx, "virus_head_kernel", held * 12);
		  virus_head_kernel<<<grid_for(held + 1), BLOCK, 0, s>>>(sorted.as<uint64_t>(), held, heads.as<uint32_t>()); }
		TRY(with_temporary(ctx, state.buffer("virus.rocprim"), "virus rocprim::exclusive_scan(heads)", held * 12, [&](void* t, size_t& b) { return rocprim::exclusive_scan(t, b, heads.as<uint32_t>(), place.as<uint64_t>(), (uint64_t) 0, (size_t) held + 1, rocprim::plus<uint64_t>(), s); }));
		{ KernelTimer timer(ctx, "virus_compact_kernel", held * 28);
		  virus_compact_kernel<<<grid_for(held), BLOCK, 0, s>>>(sorted.as<uint64_t>(), heads.as<uint32_t>(), place.as<uint64_t>(), held, work.as<uint64_t>()); }
		HIP_CHECK(hipMemcpyAsync(&distinct, place.as<uint64_t>() + held, 8, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		HIP_CHECK(hipGetLastError());
		if (distinct > held) { set_last_error("agpu_virus_expression: more distinct keys than keys"); return AGPU_ERR_DEVICE; }
	}
	DeviceBuffer& dense_of_slot = state.buffer("virus.dense_of_slot"); DeviceBuffer& shared = state.buffer("virus.shared");
	const uint64_t cells = (uint64_t) n_active * n_active;
	state.shared.assign(cells, 0);
	if (distinct > 0) {
		ALLOC(dense_of_slot, slots * 4); ALLOC(shared, std::max<uint64_t>(cells, 1) * 8);
		note();
		HIP_CHECK(hipMemcpyAsync(dense_of_slot.ptr, host_dense.data(), slots * 4, hipMemcpyHostToDevice, s));
		HIP_CHECK(hipStreamSynchronize(s));
		HIP_CHECK(hipMemsetAsync(shared.ptr, 0, std::max<uint64_t>(cells, 1) * 8, s));
		{ KernelTimer timer(ctx, "virus_kmer_count_kernel", distinct * 8);
		  virus_kmer_count_kernel<<<grid_for(distinct), BLOCK, 0, s>>>(work.as<uint64_t>(), distinct, kmer_count); }
		{ KernelTimer timer(ctx, "virus_shared_kernel", distinct * 8);
		  virus_shared_kernel<<<grid_for(distinct), BLOCK, 0, s>>>(work.as<uint64_t>(), distinct, dense_of_slot.as<uint32_t>(), n_active, shared.as<unsigned long long>()); }
		if (cells > 0) HIP_CHECK(hipMemcpyAsync(state.shared.data(), shared.ptr, cells * 8, hipMemcpyDeviceToHost, s));
	}
	HIP_CHECK(hipEventRecord(marks[3], s));

	// 4. the covered positions, and what the host gets
	if (n_viruses > 0) { KernelTimer timer(ctx, "virus_covered_kernel", bitmap_words * 4);
	  for_each_wave_chunk(n_viruses, [&](uint64_t first, uint64_t count) { virus_covered_kernel<<<grid_for(count * 64), BLOCK, 0, s>>>(bitmap.as<uint32_t>(), bitmap_offset.as<uint64_t>(), n_viruses, covered, (uint32_t) first); }); }
	state.covered.assign(n_viruses, 0); state.kmer_count.assign(n_viruses, 0);
	if (n_viruses > 0) { HIP_CHECK(hipMemcpyAsync(state.covered.data(), covered, (size_t) n_viruses * 8, hipMemcpyDeviceToHost, s)); HIP_CHECK(hipMemcpyAsync(state.kmer_count.data(), kmer_count, (size_t) n_viruses * 8, hipMemcpyDeviceToHost, s)); }
	HIP_CHECK(hipEventRecord(marks[4], s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	{ std::lock_guard<std::mutex> lock(ctx->profile_mutex); if (!ctx->failed_launch.empty()) { set_last_error("agpu_virus_expression: " + ctx->failed_launch); return AGPU_ERR_DEVICE; } }

	memset(out, 0, sizeof(*out));
	out->total = host_counters[COUNTER_TOTAL]; out->n_viruses = n_viruses; out->n_active = n_active;
	out->reads = state.reads.data(); out->covered = state.covered.data(); out->kmer_count = state.kmer_count.data(); out->active = state.active_slots.data(); out->shared = state.shared.data();
	out->candidates = m; out->kmer_keys = all_keys; out->kmer_rounds = rounds;
	for (int k = 0; k < 4; ++k) { float ms = 0; if (hipEventElapsedTime(&ms, marks[k], marks[k + 1]) == hipSuccess) out->seconds[k] = ms / 1000.0; }
	return AGPU_OK;
}

}

extern "C" {

int agpu_virus_expression(agpu_ctx* ctx, const int32_t* viral_ref, const uint32_t* viral_length, uint32_t n_viruses, uint32_t n_ref, agpu_virus_counters* counters) {
	if (!ctx || !counters || (n_viruses > 0 && (!viral_ref || !viral_length))) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	if (n_viruses > VIRUS_MAX_SLOTS) { set_last_error("--virus-expression: " + std::to_string(n_viruses) + " viral contigs, more than the 65535 that a k-mer key can name"); return AGPU_ERR_INVALID; }
	for (uint32_t v = 0; v < n_viruses; ++v)
		if (viral_ref[v] < 0 || (uint32_t) viral_ref[v] >= n_ref || (v > 0 && viral_ref[v] <= viral_ref[v - 1])) { set_last_error("agpu_virus_expression: the viral refIDs must ascend and lie below n_ref"); return AGPU_ERR_INVALID; }
	ResidentStream resident;
	TRY(resident_stream(ctx, "agpu_virus_expression", "a virus expression table of one sample over several GPUs is not supported", ctx->virus.active ? "a call is under way on this context" : nullptr, resident));
	HIP_CHECK(hipSetDevice(ctx->device));
	ctx->virus.active = true; // (the stream is read from here on: nothing of this context is given back when an allocation fails)
	hipEvent_t marks[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };
	struct Guard { agpu_ctx* ctx; hipEvent_t* marks; ~Guard() { (void) hipStreamSynchronize(ctx->stream); for (int k = 0; k < 5; ++k) if (marks[k]) (void) hipEventDestroy(marks[k]); ctx->virus.release_all(); ctx->virus.active = false; } } guard = { ctx, marks };
	for (int k = 0; k < 5; ++k) HIP_CHECK(hipEventCreate(&marks[k]));
	uint64_t peak = 0;
	const int status = run(ctx, resident, viral_ref, viral_length, n_viruses, n_ref, counters, marks, peak);
	if (status == AGPU_OK) counters->peak_bytes = peak;
	collect_kernel_samples(ctx);
	return status;
}

int agpu_virus_allocated_bytes(agpu_ctx* ctx, uint64_t* bytes) {
	if (!ctx || !bytes) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	*bytes = ctx->virus.allocated();
	return AGPU_OK;
}

}
