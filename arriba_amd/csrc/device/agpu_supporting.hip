// arriba_amd/csrc/device/agpu_supporting.hip -- --supporting-alignments on the MI355X: one sorted, indexed BAM file of stored BGZF blocks per row of fusions.tsv, with the records
// of the row's read_identifiers that lie near its breakpoints (include/arriba_gpu.h: agpu_support_pool_*, agpu_supporting_*; what the reference's
// scripts/extract_fusion-supporting_alignments.sh does with samtools).  What decides a byte is supporting_core.hpp and sorted_bam_core.hpp, which the host steps as well
// (arriba_amd/csrc/host/supporting.cpp).  Phase 1, behind the ingest, while the stream is in HBM:
//   support_name_insert_kernel   one lane per listed name: hash, open-addressing table, 64-bit atomicCAS, a hit confirmed by the bytes
//   support_mark_kernel          THE HOT PATH, one lane per record of the stream (the access pattern of sorted_bam_key_kernel: a 36-byte head and a short name per lane, ~225 bytes
//                                apart): sbam_parse's key, size and end, the QNAME hashed and looked up, name id or none
//   rocPRIM scan of the marks, support_compact_kernel, stable radix sort of (key, record), support_meta_kernel, scan of the sizes
//   support_pool_copy_kernel     one wavefront per marked record: the record into the pool, in coordinate order (the copy of sorted_bam_device.hpp)
// Phase 2, when the rows are known:
//   support_pair_kernel + radix sort        (name id, row) grouped by name id
//   support_join_kernel<count / emit>       one lane per pooled record: the rows of its name, the two windows of each; (row, pool rank) emitted
//   radix sort of the emissions             every row's records next to each other, in file order; scan of their sizes
//   support_row_kernel, support_block_table_kernel   where a row begins; per output block its row and the record its first payload byte belongs to
//   supporting_gather_kernel                one workgroup per output block: the records through the emission list into an LDS image, framed as sorted_bam_gather_kernel frames
//   supporting_index_kernel                 per record of a file its coordinates, bin and virtual offsets (the host assembles the BAI files: they are small)
// Integer and byte work, bound by HBM and by the latency of the dependent loads in front of a record's bytes; no MFMA.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <rocprim/rocprim.hpp>
#define AGPU_OPTION "--supporting-alignments"
#define AGPU_ALLOC_MESSAGE(buffer) "hipMalloc failed (" buffer "): the pool of " AGPU_OPTION " does not fit the device"
#include "resident_stream.hpp"
#include "crc32_core.hpp"
#include "supporting_core.hpp"
#include "sorted_bam_device.hpp"

using namespace agpu;

namespace {

const int GATHER_THREADS = SBAM_GATHER_THREADS;
const uint32_t GATHER_BATCH = 512;        // records whose source and destination are looked up together
const uint64_t DEFAULT_WINDOW_BYTES = 64ull << 20;

// ---- phase 1: the pool ----

__global__ void __launch_bounds__(BLOCK) support_name_insert_kernel(SupportNames names, unsigned long long* table, uint64_t slots, uint32_t hash_bits, uint32_t* name_id) {
	const uint64_t i = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (i >= names.n) return;
	name_id[i] = support_insert(table, slots, names, (uint32_t) i, hash_bits);
}

// end_flag: the end coordinate, bit 31: the record is unmapped (flag 0x4); record_name: the name id, SUPPORT_NONE for a record that is not pooled
__global__ void __launch_bounds__(BLOCK) support_mark_kernel(const uint8_t* __restrict__ stream, uint64_t stream_size, const uint64_t* __restrict__ record_offset, uint64_t n, SupportNames names,
		const unsigned long long* __restrict__ table, uint64_t slots, uint32_t hash_bits, uint64_t* keys, uint32_t* sizes, uint32_t* end_flag, uint32_t* record_name, uint32_t* marked) {
	const uint64_t r = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (r > n) return;
	if (r == n) { marked[n] = 0; return; } // (one entry more for the scan)
	const uint64_t at = record_offset[r];
	uint32_t id = SUPPORT_NONE;
	SbamRecord record; record.key = sbam_key(-1, -1, 4); record.size = 0; record.end = 0; record.flag = 4; record.ref = -1; record.pos = -1;
	if (at < stream_size) {
		record = sbam_parse(stream, at, stream_size);
		const uint8_t* name; uint32_t length;
		if (record.ref >= 0 && support_qname(stream, at, record.size, name, length)) id = support_lookup(table, slots, names, name, length, hash_bits); // (records without a reference are never selected)
	}
	keys[r] = record.key; sizes[r] = record.size; end_flag[r] = (uint32_t) record.end | ((record.flag & 4u) ? 0x80000000u : 0u);
	record_name[r] = id; marked[r] = id != SUPPORT_NONE ? 1u : 0u;
}

__global__ void __launch_bounds__(BLOCK) support_compact_kernel(const uint32_t* marked, const uint32_t* compact_index, const uint64_t* keys, uint64_t n, uint64_t* compact_keys, uint32_t* compact_record) {
	const uint64_t r = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (r >= n || !marked[r]) return;
	const uint32_t c = compact_index[r];
	compact_keys[c] = keys[r]; compact_record[c] = (uint32_t) r;
}

// the metadata of the pool in coordinate order (m + 1 entries of sizes for the scan)
__global__ void __launch_bounds__(BLOCK) support_meta_kernel(const uint64_t* keys_sorted, const uint32_t* record_sorted, uint64_t m, const uint64_t* record_offset, const uint32_t* sizes, const uint32_t* end_flag, const uint32_t* record_name,
		uint32_t* pool_size, uint64_t* pool_source, int32_t* pool_ref, int32_t* pool_pos, uint32_t* pool_end_flag, uint32_t* pool_name) {
	const uint64_t i = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (i > m) return;
	if (i == m) { pool_size[m] = 0; return; }
	const uint32_t r = record_sorted[i]; const uint64_t key = keys_sorted[i];
	pool_size[i] = sizes[r]; pool_source[i] = record_offset[r];
	pool_ref[i] = (int32_t) (uint32_t) (key >> 32); pool_pos[i] = (int32_t) ((uint32_t) (key >> 1) & 0x7FFFFFFFu) - 1;
	pool_end_flag[i] = end_flag[r]; pool_name[i] = record_name[r];
}

// one wavefront per pooled record: stream[source ..) -> pool[pool_offset[i] .. pool_offset[i + 1])
__global__ void __launch_bounds__(BLOCK) support_pool_copy_kernel(const uint8_t* __restrict__ stream, const uint64_t* __restrict__ pool_source, const uint64_t* __restrict__ pool_offset, uint64_t m, uint8_t* pool) {
	const uint64_t i = (uint64_t) blockIdx.x * (BLOCK / 64) + threadIdx.x / 64;
	if (i >= m) return;
	sbam_wave_copy<uint64_t>(pool, pool_offset[i], pool_offset[i + 1], stream, pool_source[i], threadIdx.x % 64);
}

// ---- phase 2: the files ----

__global__ void __launch_bounds__(BLOCK) support_pair_kernel(const uint32_t* entry_name, const uint32_t* entry_row, uint64_t n_entries, const uint32_t* name_id, uint64_t* pairs) {
	const uint64_t k = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (k >= n_entries) return;
	pairs[k] = support_pair_key(name_id[entry_name[k]], entry_row[k]);
}

// the first index of sorted[0 .. n) whose value is >= target
__device__ __forceinline__ uint64_t lower_bound(const uint64_t* sorted, uint64_t n, uint64_t target) {
	uint64_t low = 0, high = n;
	while (low < high) { const uint64_t middle = low + (high - low) / 2; if (sorted[middle] < target) low = middle + 1; else high = middle; }
	return low;
}

// One lane per pooled record: the rows that list its name (a row that lists a name twice counts once: equal pairs lie next to each other), the two windows of each.
// EMIT false: counts[i] (and counts[m] = 0 for the scan); true: (row, i) at emissions[offset[i] ..)
template <bool EMIT> __global__ void __launch_bounds__(BLOCK) support_join_kernel(const uint64_t* __restrict__ pairs, uint64_t n_pairs, const int32_t* __restrict__ row_ref, const int32_t* __restrict__ row_breakpoint, int64_t window,
		const int32_t* __restrict__ pool_ref, const int32_t* __restrict__ pool_pos, const uint32_t* __restrict__ pool_end_flag, const uint32_t* __restrict__ pool_name, uint64_t m, uint32_t* counts, const uint64_t* offset, uint64_t* emissions) {
	const uint64_t i = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (i > m) return;
	if (i == m) { if (!EMIT) counts[m] = 0; return; }
	const uint32_t name = pool_name[i];
	const int32_t ref = pool_ref[i], pos = pool_pos[i], end = (int32_t) (pool_end_flag[i] & 0x7FFFFFFFu);
	uint32_t count = 0;
	const uint64_t out = EMIT ? offset[i] : 0;
	const uint64_t first = lower_bound(pairs, n_pairs, support_pair_key(name, 0));
	for (uint64_t k = first; k < n_pairs; ++k) {
		const uint64_t pair = pairs[k];
		if ((uint32_t) (pair >> 32) != name) break;
		if (k > first && pairs[k - 1] == pair) continue;
		const uint32_t row = (uint32_t) pair;
		if (support_overlaps(ref, pos, end, row_ref[2 * (uint64_t) row], row_breakpoint[2 * (uint64_t) row], window) || support_overlaps(ref, pos, end, row_ref[2 * (uint64_t) row + 1], row_breakpoint[2 * (uint64_t) row + 1], window)) {
			if (EMIT) emissions[out + count] = (uint64_t) row << 32 | i;
			++count;
		}
	}
	if (!EMIT) counts[i] = count;
}

__global__ void __launch_bounds__(BLOCK) support_emission_size_kernel(const uint64_t* emissions, uint64_t n, const uint32_t* pool_size, uint32_t* sizes) {
	const uint64_t e = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (e > n) return;
	sizes[e] = e < n ? pool_size[(uint32_t) emissions[e]] : 0;
}

// row_first[r]: the first emission of row r (n_rows + 1 entries); row_byte[r]: the uncompressed offset of that record among the records of all rows
__global__ void __launch_bounds__(BLOCK) support_row_kernel(const uint64_t* emissions, uint64_t n, const uint64_t* emission_offset, uint32_t n_rows, uint64_t* row_first, uint64_t* row_byte) {
	const uint64_t r = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (r > n_rows) return;
	const uint64_t first = r == n_rows ? n : lower_bound(emissions, n, r << 32);
	row_first[r] = first; row_byte[r] = emission_offset[first];
}

// One lane per output block: its row (the last row whose first block is not behind it: rows without records have no block), and the record its first payload byte belongs to
__global__ void __launch_bounds__(BLOCK) support_block_table_kernel(const uint64_t* row_block_begin, const uint64_t* row_first, const uint64_t* row_byte, uint32_t n_rows, const uint64_t* emission_offset, uint64_t n_blocks, uint32_t* block_row, uint32_t* block_first) {
	const uint64_t b = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (b >= n_blocks) return;
	uint32_t low = 0, high = n_rows; // row_block_begin[low] <= b < row_block_begin[high] (= n_blocks)
	while (high - low > 1) { const uint32_t middle = low + (high - low) / 2; if (row_block_begin[middle] <= b) low = middle; else high = middle; }
	const uint32_t row = low;
	const uint64_t target = row_byte[row] + (b - row_block_begin[row]) * SBAM_PAYLOAD;
	uint64_t first = row_first[row], behind = row_first[row + 1]; // emission_offset[first] <= target < emission_offset[behind]
	while (behind - first > 1) { const uint64_t middle = first + (behind - first) / 2; if (emission_offset[middle] <= target) first = middle; else behind = middle; }
	block_row[b] = row; block_first[b] = (uint32_t) first;
}

struct GatherShared {
	SbamFrameShared frame;
	uint64_t source[GATHER_BATCH];           // where the record begins in the pool
	uint64_t destination[GATHER_BATCH + 1];  // ... and among the records of all rows; (the CRCs of the lanes lie over `source` later)
};
static_assert(sizeof(uint64_t) * GATHER_BATCH >= sizeof(uint32_t) * GATHER_THREADS, "the CRCs of the lanes fit where the sources were");
static_assert(sizeof(GatherShared) * 2 <= 160 * 1024, "two workgroups per CU");

// One workgroup per output block: block first_block + blockIdx.x of the blocks of all rows.  The framed blocks of a row lie next to each other and the rows behind each other:
// block k of row r begins at row_out_offset[r] + k * SBAM_BLOCK, and goes to out + that - window_base.
__global__ void __launch_bounds__(GATHER_THREADS) supporting_gather_kernel(const uint8_t* __restrict__ pool, const uint64_t* __restrict__ pool_offset, const uint64_t* __restrict__ emissions, const uint64_t* __restrict__ emission_offset,
		const uint32_t* __restrict__ block_row, const uint32_t* __restrict__ block_first, const uint64_t* __restrict__ row_first, const uint64_t* __restrict__ row_byte, const uint64_t* __restrict__ row_block_begin,
		const uint64_t* __restrict__ row_out_offset, uint64_t n_blocks, uint64_t first_block, uint64_t window_base, const Crc32Tables* __restrict__ tables, uint8_t* out) {
	__shared__ GatherShared shared;
	const uint32_t t = threadIdx.x, lane = t % 64, wave = t / 64;
	const uint64_t b = first_block + blockIdx.x;
	if (b >= n_blocks) return;
	const uint32_t row = block_row[b];
	const uint64_t in_row = b - row_block_begin[row];
	const uint64_t begin = row_byte[row] + in_row * SBAM_PAYLOAD, row_end = row_byte[row + 1];
	const uint32_t length = (uint32_t) (row_end - begin < SBAM_PAYLOAD ? row_end - begin : SBAM_PAYLOAD);
	uint8_t* const block_out = out + (row_out_offset[row] + in_row * SBAM_BLOCK - window_base);
	const uint32_t pad = (uint32_t) ((uint64_t) block_out & 15u);
	uint8_t* const image = (uint8_t*) shared.frame.image;
	const uint32_t payload_at = pad + SBAM_HEAD;
	sbam_frame_begin(shared.frame, tables, pad, length, t);

	const uint64_t first_record = block_first[b], last_record = (b + 1 < n_blocks && block_row[b + 1] == row) ? block_first[b + 1] : row_first[row + 1] - 1;
	for (uint64_t batch = first_record; batch <= last_record; batch += GATHER_BATCH) {
		const uint32_t count = (uint32_t) (last_record - batch + 1 < GATHER_BATCH ? last_record - batch + 1 : GATHER_BATCH);
		__syncthreads(); // (the batch before has been copied)
		for (uint32_t j = t; j <= count; j += GATHER_THREADS) {
			shared.destination[j] = emission_offset[batch + j]; // (emission_offset has one entry more than there are emissions)
			if (j < count) shared.source[j] = pool_offset[(uint32_t) emissions[batch + j]];
		}
		__syncthreads();
		for (uint32_t j = wave; j < count; j += GATHER_THREADS / 64) {
			const uint64_t record_begin = shared.destination[j], record_end = shared.destination[j + 1];
			const uint64_t from = record_begin > begin ? record_begin : begin, to = record_end < begin + length ? record_end : begin + length;
			if (from >= to) continue;
			sbam_wave_copy<uint32_t>(image, payload_at + (uint32_t) (from - begin), payload_at + (uint32_t) (to - begin), pool, shared.source[j] + (from - record_begin), lane);
		}
	}
	__syncthreads();
	sbam_frame_finish(shared.frame, (uint32_t*) shared.source, pad, length, block_out, t);
}

__global__ void __launch_bounds__(BLOCK) supporting_index_kernel(const uint64_t* emissions, const uint64_t* emission_offset, uint64_t n, const uint64_t* row_byte, const int32_t* pool_ref, const int32_t* pool_pos, const uint32_t* pool_end_flag,
		uint64_t first_block_file_offset, int32_t* ref, int32_t* pos, uint32_t* end_flag, uint32_t* bin, uint64_t* begin, uint64_t* end) {
	const uint64_t e = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (e >= n) return;
	const uint64_t emission = emissions[e]; const uint32_t row = (uint32_t) (emission >> 32), rank = (uint32_t) emission;
	const int32_t p = pool_pos[rank]; const uint32_t word = pool_end_flag[rank];
	ref[e] = pool_ref[rank]; pos[e] = p; end_flag[e] = word;
	bin[e] = (p >= 0 && p < SBAM_MAX_REFERENCE) ? sbam_reg2bin(p, (int32_t) (word & 0x7FFFFFFFu)) : SUPPORT_NONE;
	begin[e] = sbam_voffset(first_block_file_offset, emission_offset[e] - row_byte[row]); end[e] = sbam_voffset(first_block_file_offset, emission_offset[e + 1] - row_byte[row]);
}

uint32_t hash_bits_knob() {
	const char* knob = getenv("ARRIBA_SUPPORT_HASH_BITS");
	if (knob == nullptr || knob[0] == 0) return 64;
	const long bits = strtol(knob, nullptr, 10);
	return bits >= 1 && bits < 64 ? (uint32_t) bits : 64;
}

// the framed blocks of all rows lie behind each other: where block b begins (b == blocks: where they end)
uint64_t out_offset_of_block(const SupportState& state, uint64_t b) {
	if (b >= state.blocks) return state.row_out_offset[state.n_rows];
	const size_t row = (size_t) (std::upper_bound(state.row_block_begin.begin(), state.row_block_begin.begin() + state.n_rows, b) - state.row_block_begin.begin()) - 1; // (the last row that begins at or in front of b)
	return state.row_out_offset[row] + (b - state.row_block_begin[row]) * SBAM_BLOCK;
}

int launch_gather(agpu_ctx* ctx, uint64_t first_block) {
	SupportState& state = ctx->support;
	const uint64_t blocks = std::min<uint64_t>(state.window_blocks, state.blocks - first_block);
	const uint64_t base = out_offset_of_block(state, first_block), bytes = out_offset_of_block(state, first_block + blocks) - base;
	{ KernelTimer timer(ctx, "supporting_gather_kernel", 2 * bytes);
	  supporting_gather_kernel<<<(unsigned int) blocks, GATHER_THREADS, 0, ctx->stream>>>(state.buffer("support.pool").as<uint8_t>(), state.buffer("support.pool_offset").as<uint64_t>(), state.buffer("support.files.emissions").as<uint64_t>(),
		state.buffer("support.files.emission_offset").as<uint64_t>(), state.buffer("support.files.block_row").as<uint32_t>(), state.buffer("support.files.block_first").as<uint32_t>(), state.buffer("support.files.row_first").as<uint64_t>(),
		state.buffer("support.files.row_byte").as<uint64_t>(), state.buffer("support.files.row_block_begin").as<uint64_t>(), state.buffer("support.files.row_out_offset").as<uint64_t>(), state.blocks, first_block, base,
		state.buffer("support.crc_tables").as<Crc32Tables>(), state.buffer("support.files.staging").as<uint8_t>()); }
	state.gathered_block = first_block;
	return AGPU_OK;
}

}

extern "C" {

int agpu_support_pool_build(agpu_ctx* ctx, const char* names, const uint64_t* name_offset, uint64_t n_names, agpu_support_pool_info* info) {
	if (!ctx || !info || (names != nullptr && n_names > 0 && !name_offset)) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	ResidentStream resident;
	TRY(resident_stream(ctx, "agpu_support_pool_build", "supporting alignments of one sample over several GPUs are not supported", ctx->support.active ? "agpu_supporting_end must run first" : nullptr, resident));
	const uint64_t size = resident.stream_size, base = resident.first_record, n = resident.records;
	const bool of_batch = names == nullptr;
	if (of_batch) { if (!ctx->have_batch) { set_last_error("agpu_support_pool_build: no batch whose names could be taken"); return AGPU_ERR_INVALID; } n_names = ctx->n; }
	if (n_names >= SUPPORT_MAX_NAMES) { set_last_error("agpu_support_pool_build: too many names"); return AGPU_ERR_INVALID; }
	if (!of_batch) for (uint64_t k = 0; k < n_names; ++k) if (name_offset[k + 1] < name_offset[k]) { set_last_error("agpu_support_pool_build: name_offset must not fall"); return AGPU_ERR_INVALID; }
	HIP_CHECK(hipSetDevice(ctx->device));
	hipStream_t s = ctx->stream;
	SupportState& state = ctx->support;
	state.built = false;
	state.active = true; // (the stream is read from here on: nothing of this context is given back when an allocation fails)
	struct Guard { SupportState& state; ~Guard() { state.active = false; state.release_prefix("support.tmp."); } } guard = { state };
	state.hash_bits = hash_bits_knob(); state.strip_hit_index = of_batch; state.n_names = n_names; state.table_slots = support_table_slots(n_names);
	DeviceBuffer& name_id = state.buffer("support.name_id"); DeviceBuffer& table = state.buffer("support.tmp.table");
	ALLOC(name_id, std::max<uint64_t>(n_names, 1) * 4); ALLOC(table, state.table_slots * 8);
	SupportNames view; view.n = n_names; view.strip_hit_index = of_batch;
	if (of_batch) { view.bytes = ctx->names.as<uint8_t>(); view.offset = ctx->name_offset.as<uint64_t>(); }
	else {
		DeviceBuffer& bytes = state.buffer("support.tmp.names"); DeviceBuffer& offsets = state.buffer("support.tmp.name_offset");
		const uint64_t total = n_names > 0 ? name_offset[n_names] : 0;
		ALLOC(bytes, std::max<uint64_t>(total, 1)); ALLOC(offsets, (n_names + 1) * 8);
		if (n_names > 0) { if (total > 0) HIP_CHECK(hipMemcpyAsync(bytes.ptr, names, total, hipMemcpyHostToDevice, s)); HIP_CHECK(hipMemcpyAsync(offsets.ptr, name_offset, (n_names + 1) * 8, hipMemcpyHostToDevice, s)); HIP_CHECK(hipStreamSynchronize(s)); }
		else HIP_CHECK(hipMemsetAsync(offsets.ptr, 0, 8, s));
		view.bytes = bytes.as<uint8_t>(); view.offset = offsets.as<uint64_t>();
	}
	HIP_CHECK(hipMemsetAsync(table.ptr, 0, state.table_slots * 8, s));
	if (n_names > 0) { KernelTimer timer(ctx, "support_name_insert_kernel", n_names * 48);
	  support_name_insert_kernel<<<grid_for(n_names), BLOCK, 0, s>>>(view, table.as<unsigned long long>(), state.table_slots, state.hash_bits, name_id.as<uint32_t>()); }
	// the marks
	const size_t room = std::max<uint64_t>(n, 1);
	DeviceBuffer& keys = state.buffer("support.tmp.keys"); DeviceBuffer& sizes = state.buffer("support.tmp.sizes"); DeviceBuffer& end_flag = state.buffer("support.tmp.end_flag"); DeviceBuffer& record_name = state.buffer("support.tmp.record_name");
	DeviceBuffer& marked = state.buffer("support.tmp.marked"); DeviceBuffer& compact_index = state.buffer("support.tmp.compact_index");
	ALLOC(keys, room * 8); ALLOC(sizes, room * 4); ALLOC(end_flag, room * 4); ALLOC(record_name, room * 4); ALLOC(marked, (room + 1) * 4); ALLOC(compact_index, (room + 1) * 4);
	{ KernelTimer timer(ctx, "support_mark_kernel", n * 28 + (size - base) / 4);
	  support_mark_kernel<<<grid_for(n + 1), BLOCK, 0, s>>>(resident.stream, size, resident.record_offset, n, view, table.as<unsigned long long>(), state.table_slots, state.hash_bits,
		keys.as<uint64_t>(), sizes.as<uint32_t>(), end_flag.as<uint32_t>(), record_name.as<uint32_t>(), marked.as<uint32_t>()); }
	TRY(with_temporary(ctx, state.buffer("support.tmp.rocprim"), "support rocprim::exclusive_scan(marks)", n * 8, [&](void* t, size_t& b) { return rocprim::exclusive_scan(t, b, marked.as<uint32_t>(), compact_index.as<uint32_t>(), 0u, (size_t) n + 1, rocprim::plus<uint32_t>(), s); }));
	uint32_t m32 = 0;
	HIP_CHECK(hipMemcpyAsync(&m32, compact_index.as<uint32_t>() + n, 4, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	const uint64_t m = m32;
	// compact, sort, metadata, offsets
	const size_t pool_room = std::max<uint64_t>(m, 1);
	DeviceBuffer& compact_keys = state.buffer("support.tmp.compact_keys"); DeviceBuffer& compact_record = state.buffer("support.tmp.compact_record"); DeviceBuffer& keys_sorted = state.buffer("support.tmp.keys_sorted");
	DeviceBuffer& record_sorted = state.buffer("support.tmp.record_sorted"); DeviceBuffer& pool_source = state.buffer("support.tmp.pool_source");
	DeviceBuffer& pool_size = state.buffer("support.pool_size"); DeviceBuffer& pool_offset = state.buffer("support.pool_offset"); DeviceBuffer& pool_ref = state.buffer("support.pool_ref"); DeviceBuffer& pool_pos = state.buffer("support.pool_pos");
	DeviceBuffer& pool_end_flag = state.buffer("support.pool_end_flag"); DeviceBuffer& pool_name = state.buffer("support.pool_name"); DeviceBuffer& pool = state.buffer("support.pool");
	ALLOC(compact_keys, pool_room * 8); ALLOC(compact_record, pool_room * 4); ALLOC(keys_sorted, pool_room * 8); ALLOC(record_sorted, pool_room * 4); ALLOC(pool_source, pool_room * 8);
	ALLOC(pool_size, (pool_room + 1) * 4); ALLOC(pool_offset, (pool_room + 1) * 8); ALLOC(pool_ref, pool_room * 4); ALLOC(pool_pos, pool_room * 4); ALLOC(pool_end_flag, pool_room * 4); ALLOC(pool_name, pool_room * 4);
	uint64_t total = 0;
	if (m > 0) {
		{ KernelTimer timer(ctx, "support_compact_kernel", n * 8 + m * 12);
		  support_compact_kernel<<<grid_for(n), BLOCK, 0, s>>>(marked.as<uint32_t>(), compact_index.as<uint32_t>(), keys.as<uint64_t>(), n, compact_keys.as<uint64_t>(), compact_record.as<uint32_t>()); }
		TRY(with_temporary(ctx, state.buffer("support.tmp.rocprim"), "support rocprim::radix_sort_pairs(pool)", m * 24, [&](void* t, size_t& b) { return rocprim::radix_sort_pairs(t, b, compact_keys.as<uint64_t>(), keys_sorted.as<uint64_t>(), compact_record.as<uint32_t>(), record_sorted.as<uint32_t>(), (size_t) m, 0, 64, s); }));
		{ KernelTimer timer(ctx, "support_meta_kernel", m * 48);
		  support_meta_kernel<<<grid_for(m + 1), BLOCK, 0, s>>>(keys_sorted.as<uint64_t>(), record_sorted.as<uint32_t>(), m, resident.record_offset, sizes.as<uint32_t>(), end_flag.as<uint32_t>(), record_name.as<uint32_t>(),
			pool_size.as<uint32_t>(), pool_source.as<uint64_t>(), pool_ref.as<int32_t>(), pool_pos.as<int32_t>(), pool_end_flag.as<uint32_t>(), pool_name.as<uint32_t>()); }
		TRY(with_temporary(ctx, state.buffer("support.tmp.rocprim"), "support rocprim::exclusive_scan(pool sizes)", m * 12, [&](void* t, size_t& b) { return rocprim::exclusive_scan(t, b, pool_size.as<uint32_t>(), pool_offset.as<uint64_t>(), (uint64_t) 0, (size_t) m + 1, rocprim::plus<uint64_t>(), s); }));
		HIP_CHECK(hipMemcpyAsync(&total, pool_offset.as<uint64_t>() + m, 8, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		if (total > size - base) { set_last_error("agpu_support_pool_build: the pooled records are larger than the stream"); return AGPU_ERR_INVALID; }
	} else { HIP_CHECK(hipMemsetAsync(pool_offset.ptr, 0, 8, s)); HIP_CHECK(hipMemsetAsync(pool_size.ptr, 0, 4, s)); }
	ALLOC(pool, (total + 3) / 4 * 4 + 16);
	if (m > 0) { KernelTimer timer(ctx, "support_pool_copy_kernel", 2 * total + m * 24);
	  support_pool_copy_kernel<<<(unsigned int) ((m + BLOCK / 64 - 1) / (BLOCK / 64)), BLOCK, 0, s>>>(resident.stream, pool_source.as<uint64_t>(), pool_offset.as<uint64_t>(), m, pool.as<uint8_t>()); }
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	state.records = m; state.bytes = total; state.built = true;
	memset(info, 0, sizeof(*info));
	info->names = n_names; info->stream_records = n; info->pooled_records = m; info->pool_bytes = total;
	collect_kernel_samples(ctx);
	return AGPU_OK;
}

int agpu_supporting_begin(agpu_ctx* ctx, const agpu_supporting_rows* rows, int64_t window, agpu_supporting_info* info) {
	if (!ctx || !rows || !info) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	SupportState& state = ctx->support;
	if (!state.built) { set_last_error("agpu_supporting_begin: there is no pool of supporting alignments on this context (agpu_support_pool_build comes first, behind the ingest of the sample)"); return AGPU_ERR_INVALID; }
	if (state.active) { set_last_error("agpu_supporting_begin: agpu_supporting_end must run first"); return AGPU_ERR_INVALID; }
	if (window < 0 || window > 0x7FFFFFFF) { set_last_error("agpu_supporting_begin: the window must lie in 0 .. 2^31-1"); return AGPU_ERR_INVALID; }
	const uint32_t n_rows = rows->n_rows;
	if (n_rows >= 0x7FFFFFF0u) { set_last_error("agpu_supporting_begin: too many rows"); return AGPU_ERR_INVALID; }
	if (n_rows > 0 && (!rows->ref || !rows->breakpoint || !rows->name_begin)) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	const uint64_t n_entries = n_rows > 0 ? rows->name_begin[n_rows] : 0;
	if (n_entries > 0 && !rows->names) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	std::vector<uint32_t> entry_row((size_t) n_entries);
	for (uint32_t r = 0; r < n_rows; ++r) {
		if (rows->name_begin[r + 1] < rows->name_begin[r] || rows->name_begin[r + 1] > n_entries) { set_last_error("agpu_supporting_begin: name_begin must not fall"); return AGPU_ERR_INVALID; }
		for (uint64_t k = rows->name_begin[r]; k < rows->name_begin[r + 1]; ++k) {
			if (rows->names[k] >= state.n_names) { set_last_error("agpu_supporting_begin: a row lists a name the pool was not built from"); return AGPU_ERR_INVALID; }
			entry_row[(size_t) k] = r;
		}
	}
	HIP_CHECK(hipSetDevice(ctx->device));
	hipStream_t s = ctx->stream;
	state.active = true;
	struct Guard { SupportState& state; bool keep; ~Guard() { if (!keep) { state.active = false; state.release_prefix("support.files."); state.release_prefix("support.tmp."); } } } guard = { state, false };
	const uint64_t m = state.records;
	uint64_t window_bytes = DEFAULT_WINDOW_BYTES;
	{ const char* knob = getenv("ARRIBA_SUPPORTING_WINDOW"); if (knob != nullptr && knob[0] != 0) window_bytes = strtoull(knob, nullptr, 10); }
	const uint64_t window_blocks = std::max<uint64_t>(std::min<uint64_t>(window_bytes / SBAM_BLOCK, 1u << 20), 1);
	DeviceBuffer& crc_tables = state.buffer("support.crc_tables");
	if (crc_tables.ptr == nullptr) {
		ALLOC(crc_tables, sizeof(Crc32Tables));
		static Crc32Tables tables; static bool made = false; static std::mutex mutex;
		{ std::lock_guard<std::mutex> lock(mutex); if (!made) { crc32_make_tables(tables); made = true; } }
		HIP_CHECK(hipMemcpy(crc_tables.ptr, &tables, sizeof(tables), hipMemcpyHostToDevice));
	}
	// the rows on the device; (name id, row) grouped by name id
	DeviceBuffer& row_ref = state.buffer("support.files.row_ref"); DeviceBuffer& row_breakpoint = state.buffer("support.files.row_breakpoint"); DeviceBuffer& entry_name_d = state.buffer("support.tmp.entry_name");
	DeviceBuffer& entry_row_d = state.buffer("support.tmp.entry_row"); DeviceBuffer& pairs = state.buffer("support.tmp.pairs"); DeviceBuffer& pairs_sorted = state.buffer("support.tmp.pairs_sorted");
	const size_t row_room = std::max<uint32_t>(n_rows, 1), entry_room = std::max<uint64_t>(n_entries, 1), pool_room = std::max<uint64_t>(m, 1);
	ALLOC(row_ref, row_room * 8); ALLOC(row_breakpoint, row_room * 8); ALLOC(entry_name_d, entry_room * 4); ALLOC(entry_row_d, entry_room * 4); ALLOC(pairs, entry_room * 8); ALLOC(pairs_sorted, entry_room * 8);
	if (n_rows > 0) { HIP_CHECK(hipMemcpyAsync(row_ref.ptr, rows->ref, (size_t) n_rows * 8, hipMemcpyHostToDevice, s)); HIP_CHECK(hipMemcpyAsync(row_breakpoint.ptr, rows->breakpoint, (size_t) n_rows * 8, hipMemcpyHostToDevice, s)); }
	if (n_entries > 0) { HIP_CHECK(hipMemcpyAsync(entry_name_d.ptr, rows->names, n_entries * 4, hipMemcpyHostToDevice, s)); HIP_CHECK(hipMemcpyAsync(entry_row_d.ptr, entry_row.data(), n_entries * 4, hipMemcpyHostToDevice, s)); }
	HIP_CHECK(hipStreamSynchronize(s)); // (the sources are pageable memory of the caller and of this call)
	uint64_t n_emissions = 0, total = 0;
	DeviceBuffer& counts = state.buffer("support.tmp.counts"); DeviceBuffer& offsets = state.buffer("support.tmp.offsets");
	DeviceBuffer& emissions = state.buffer("support.files.emissions"); DeviceBuffer& emission_offset = state.buffer("support.files.emission_offset");
	const int32_t* pool_ref = state.buffer("support.pool_ref").as<int32_t>(); const int32_t* pool_pos = state.buffer("support.pool_pos").as<int32_t>();
	const uint32_t* pool_end_flag = state.buffer("support.pool_end_flag").as<uint32_t>(); const uint32_t* pool_name = state.buffer("support.pool_name").as<uint32_t>();
	if (n_entries > 0 && m > 0) {
		{ KernelTimer timer(ctx, "support_pair_kernel", n_entries * 20);
		  support_pair_kernel<<<grid_for(n_entries), BLOCK, 0, s>>>(entry_name_d.as<uint32_t>(), entry_row_d.as<uint32_t>(), n_entries, state.buffer("support.name_id").as<uint32_t>(), pairs.as<uint64_t>()); }
		TRY(with_temporary(ctx, state.buffer("support.tmp.rocprim"), "support rocprim::radix_sort_keys(pairs)", n_entries * 16, [&](void* t, size_t& b) { return rocprim::radix_sort_keys(t, b, pairs.as<uint64_t>(), pairs_sorted.as<uint64_t>(), (size_t) n_entries, 0, 64, s); }));
		ALLOC(counts, (pool_room + 1) * 4); ALLOC(offsets, (pool_room + 1) * 8);
		{ KernelTimer timer(ctx, "support_join_kernel(count)", m * 20);
		  support_join_kernel<false><<<grid_for(m + 1), BLOCK, 0, s>>>(pairs_sorted.as<uint64_t>(), n_entries, row_ref.as<int32_t>(), row_breakpoint.as<int32_t>(), window, pool_ref, pool_pos, pool_end_flag, pool_name, m, counts.as<uint32_t>(), nullptr, nullptr); }
		TRY(with_temporary(ctx, state.buffer("support.tmp.rocprim"), "support rocprim::exclusive_scan(emissions)", m * 12, [&](void* t, size_t& b) { return rocprim::exclusive_scan(t, b, counts.as<uint32_t>(), offsets.as<uint64_t>(), (uint64_t) 0, (size_t) m + 1, rocprim::plus<uint64_t>(), s); }));
		HIP_CHECK(hipMemcpyAsync(&n_emissions, offsets.as<uint64_t>() + m, 8, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		if (n_emissions >= 0xFFFFFFF0ull) { set_last_error("agpu_supporting_begin: more than 2^32-16 records in the files of the rows"); return AGPU_ERR_INVALID; }
	}
	const size_t emission_room = std::max<uint64_t>(n_emissions, 1);
	ALLOC(emissions, emission_room * 8); ALLOC(emission_offset, (emission_room + 1) * 8);
	if (n_emissions > 0) {
		DeviceBuffer& unsorted = state.buffer("support.tmp.emissions"); DeviceBuffer& sizes = state.buffer("support.tmp.emission_sizes");
		ALLOC(unsorted, emission_room * 8); ALLOC(sizes, (emission_room + 1) * 4);
		{ KernelTimer timer(ctx, "support_join_kernel(emit)", m * 28 + n_emissions * 8);
		  support_join_kernel<true><<<grid_for(m + 1), BLOCK, 0, s>>>(pairs_sorted.as<uint64_t>(), n_entries, row_ref.as<int32_t>(), row_breakpoint.as<int32_t>(), window, pool_ref, pool_pos, pool_end_flag, pool_name, m, nullptr, offsets.as<uint64_t>(), unsorted.as<uint64_t>()); }
		TRY(with_temporary(ctx, state.buffer("support.tmp.rocprim"), "support rocprim::radix_sort_keys(emissions)", n_emissions * 16, [&](void* t, size_t& b) { return rocprim::radix_sort_keys(t, b, unsorted.as<uint64_t>(), emissions.as<uint64_t>(), (size_t) n_emissions, 0, 64, s); }));
		{ KernelTimer timer(ctx, "support_emission_size_kernel", n_emissions * 16);
		  support_emission_size_kernel<<<grid_for(n_emissions + 1), BLOCK, 0, s>>>(emissions.as<uint64_t>(), n_emissions, state.buffer("support.pool_size").as<uint32_t>(), sizes.as<uint32_t>()); }
		TRY(with_temporary(ctx, state.buffer("support.tmp.rocprim"), "support rocprim::exclusive_scan(emission sizes)", n_emissions * 12, [&](void* t, size_t& b) { return rocprim::exclusive_scan(t, b, sizes.as<uint32_t>(), emission_offset.as<uint64_t>(), (uint64_t) 0, (size_t) n_emissions + 1, rocprim::plus<uint64_t>(), s); }));
	} else HIP_CHECK(hipMemsetAsync(emission_offset.ptr, 0, 8, s));
	// where the rows begin: records, bytes, blocks, framed bytes
	DeviceBuffer& row_first = state.buffer("support.files.row_first"); DeviceBuffer& row_byte = state.buffer("support.files.row_byte"); DeviceBuffer& row_block_begin = state.buffer("support.files.row_block_begin"); DeviceBuffer& row_out_offset = state.buffer("support.files.row_out_offset");
	ALLOC(row_first, (row_room + 1) * 8); ALLOC(row_byte, (row_room + 1) * 8); ALLOC(row_block_begin, (row_room + 1) * 8); ALLOC(row_out_offset, (row_room + 1) * 8);
	{ KernelTimer timer(ctx, "support_row_kernel", (uint64_t) n_rows * 16);
	  support_row_kernel<<<grid_for((uint64_t) n_rows + 1), BLOCK, 0, s>>>(emissions.as<uint64_t>(), n_emissions, emission_offset.as<uint64_t>(), n_rows, row_first.as<uint64_t>(), row_byte.as<uint64_t>()); }
	std::vector<uint64_t> host_row_byte((size_t) n_rows + 1);
	state.row_first.assign((size_t) n_rows + 1, 0); state.row_bytes.assign((size_t) n_rows + 1, 0); state.row_block_begin.assign((size_t) n_rows + 1, 0); state.row_out_offset.assign((size_t) n_rows + 1, 0);
	HIP_CHECK(hipMemcpyAsync(state.row_first.data(), row_first.ptr, ((size_t) n_rows + 1) * 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipMemcpyAsync(host_row_byte.data(), row_byte.ptr, ((size_t) n_rows + 1) * 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	for (uint32_t r = 0; r < n_rows; ++r) {
		if (host_row_byte[r + 1] < host_row_byte[r] || state.row_first[r + 1] < state.row_first[r]) { set_last_error("agpu_supporting_begin: the rows of the emission list are out of order"); return AGPU_ERR_DEVICE; }
		state.row_bytes[r] = host_row_byte[r + 1] - host_row_byte[r];
		const uint64_t blocks = sbam_block_count(state.row_bytes[r]);
		state.row_block_begin[r + 1] = state.row_block_begin[r] + blocks;
		state.row_out_offset[r + 1] = state.row_out_offset[r] + state.row_bytes[r] + blocks * (SBAM_HEAD + SBAM_TAIL);
	}
	total = host_row_byte[n_rows];
	const uint64_t n_blocks = state.row_block_begin[n_rows];
	HIP_CHECK(hipMemcpyAsync(row_block_begin.ptr, state.row_block_begin.data(), ((size_t) n_rows + 1) * 8, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(row_out_offset.ptr, state.row_out_offset.data(), ((size_t) n_rows + 1) * 8, hipMemcpyHostToDevice, s));
	DeviceBuffer& block_row = state.buffer("support.files.block_row"); DeviceBuffer& block_first = state.buffer("support.files.block_first"); DeviceBuffer& staging = state.buffer("support.files.staging");
	ALLOC(block_row, std::max<uint64_t>(n_blocks, 1) * 4); ALLOC(block_first, std::max<uint64_t>(n_blocks, 1) * 4); ALLOC(staging, std::max<uint64_t>(std::min(window_blocks, n_blocks), 1) * SBAM_BLOCK + 16);
	if (n_blocks > 0) { KernelTimer timer(ctx, "support_block_table_kernel", n_blocks * 8);
	  support_block_table_kernel<<<grid_for(n_blocks), BLOCK, 0, s>>>(row_block_begin.as<uint64_t>(), row_first.as<uint64_t>(), row_byte.as<uint64_t>(), n_rows, emission_offset.as<uint64_t>(), n_blocks, block_row.as<uint32_t>(), block_first.as<uint32_t>()); }
	HIP_CHECK(hipStreamSynchronize(s)); // (the two tables came from the vectors of the state)
	HIP_CHECK(hipGetLastError());
	state.release_prefix("support.tmp.");
	state.n_rows = n_rows; state.emissions = n_emissions; state.blocks = n_blocks; state.window_blocks = window_blocks; state.next_block = 0; state.gathered_block = ~0ull; state.index_ready = false;
	memset(info, 0, sizeof(*info));
	info->rows = n_rows; info->records = n_emissions; info->uncompressed_bytes = total; info->file_bytes = state.row_out_offset[n_rows]; info->blocks = n_blocks;
	info->windows = (n_blocks + window_blocks - 1) / window_blocks; info->window_bytes = std::max<uint64_t>(std::min(window_blocks, n_blocks), 1) * SBAM_BLOCK;
	collect_kernel_samples(ctx);
	guard.keep = true;
	return AGPU_OK;
}

int agpu_supporting_row_bytes(agpu_ctx* ctx, uint64_t* row_file_bytes) {
	if (!ctx || (!row_file_bytes && ctx->support.n_rows > 0)) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	if (!ctx->support.active || !ctx->support.built) { set_last_error("agpu_supporting_begin must run first"); return AGPU_ERR_INVALID; }
	for (uint32_t r = 0; r < ctx->support.n_rows; ++r) row_file_bytes[r] = ctx->support.row_out_offset[r + 1] - ctx->support.row_out_offset[r];
	return AGPU_OK;
}

int agpu_supporting_next(agpu_ctx* ctx, void* pinned, uint64_t capacity, uint64_t* bytes) {
	if (!ctx || !bytes) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	SupportState& state = ctx->support;
	if (!state.active || !state.built) { set_last_error("agpu_supporting_begin must run first"); return AGPU_ERR_INVALID; }
	*bytes = 0;
	if (state.next_block >= state.blocks) return AGPU_OK;
	HIP_CHECK(hipSetDevice(ctx->device));
	hipStream_t s = ctx->stream;
	const uint64_t first = state.next_block, blocks = std::min<uint64_t>(state.window_blocks, state.blocks - first);
	const uint64_t window = out_offset_of_block(state, first + blocks) - out_offset_of_block(state, first);
	if (!pinned || capacity < window) { set_last_error("agpu_supporting_next: the buffer is smaller than a window (agpu_supporting_info.window_bytes)"); return AGPU_ERR_INVALID; }
	if (state.gathered_block != first) TRY(launch_gather(ctx, first));
	{ KernelTimer timer(ctx, "supporting copy back", window);
	  HIP_CHECK(hipMemcpyAsync(pinned, state.buffer("support.files.staging").ptr, window, hipMemcpyDeviceToHost, s)); }
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	state.next_block = first + blocks;
	if (state.next_block < state.blocks) TRY(launch_gather(ctx, state.next_block)); // (gathered while the caller writes this window)
	*bytes = window;
	collect_kernel_samples(ctx);
	return AGPU_OK;
}

int agpu_supporting_index(agpu_ctx* ctx, uint64_t first_block_file_offset, agpu_supporting_index_arrays* index) {
	if (!ctx || !index) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	SupportState& state = ctx->support;
	if (!state.active || !state.built) { set_last_error("agpu_supporting_begin must run first"); return AGPU_ERR_INVALID; }
	HIP_CHECK(hipSetDevice(ctx->device));
	hipStream_t s = ctx->stream;
	const uint64_t n = state.emissions;
	index->n_rows = state.n_rows; index->n_records = n;
	if (!index->row_first && !index->ref && !index->pos && !index->end_flag && !index->bin && !index->begin && !index->end) return AGPU_OK; // the sizes
	if (!index->row_first || !index->ref || !index->pos || !index->end_flag || !index->bin || !index->begin || !index->end) { set_last_error("agpu_supporting_index: all arrays or none"); return AGPU_ERR_INVALID; }
	for (uint32_t r = 0; r <= state.n_rows; ++r) index->row_first[r] = state.row_first[r];
	if (n == 0) return AGPU_OK;
	DeviceBuffer& ref = state.buffer("support.files.index_ref"); DeviceBuffer& pos = state.buffer("support.files.index_pos"); DeviceBuffer& end_flag = state.buffer("support.files.index_end_flag");
	DeviceBuffer& bin = state.buffer("support.files.index_bin"); DeviceBuffer& begin = state.buffer("support.files.index_begin"); DeviceBuffer& end = state.buffer("support.files.index_end");
	if (!state.index_ready || state.index_first != first_block_file_offset) {
		ALLOC(ref, n * 4); ALLOC(pos, n * 4); ALLOC(end_flag, n * 4); ALLOC(bin, n * 4); ALLOC(begin, n * 8); ALLOC(end, n * 8);
		{ KernelTimer timer(ctx, "supporting_index_kernel", n * 56);
		  supporting_index_kernel<<<grid_for(n), BLOCK, 0, s>>>(state.buffer("support.files.emissions").as<uint64_t>(), state.buffer("support.files.emission_offset").as<uint64_t>(), n, state.buffer("support.files.row_byte").as<uint64_t>(),
			state.buffer("support.pool_ref").as<int32_t>(), state.buffer("support.pool_pos").as<int32_t>(), state.buffer("support.pool_end_flag").as<uint32_t>(), first_block_file_offset,
			ref.as<int32_t>(), pos.as<int32_t>(), end_flag.as<uint32_t>(), bin.as<uint32_t>(), begin.as<uint64_t>(), end.as<uint64_t>()); }
		state.index_ready = true; state.index_first = first_block_file_offset;
	}
	HIP_CHECK(hipMemcpyAsync(index->ref, ref.ptr, n * 4, hipMemcpyDeviceToHost, s)); HIP_CHECK(hipMemcpyAsync(index->pos, pos.ptr, n * 4, hipMemcpyDeviceToHost, s)); HIP_CHECK(hipMemcpyAsync(index->end_flag, end_flag.ptr, n * 4, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipMemcpyAsync(index->bin, bin.ptr, n * 4, hipMemcpyDeviceToHost, s)); HIP_CHECK(hipMemcpyAsync(index->begin, begin.ptr, n * 8, hipMemcpyDeviceToHost, s)); HIP_CHECK(hipMemcpyAsync(index->end, end.ptr, n * 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	collect_kernel_samples(ctx);
	return AGPU_OK;
}

int agpu_supporting_end(agpu_ctx* ctx) {
	if (!ctx) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	SupportState& state = ctx->support;
	if (!state.active) return AGPU_OK;
	(void) hipSetDevice(ctx->device);
	const hipError_t status = hipStreamSynchronize(ctx->stream); // (a window gathered ahead that nobody asked for)
	state.active = false; state.index_ready = false; state.gathered_block = ~0ull;
	state.release_prefix("support.files.");
	collect_kernel_samples(ctx);
	if (status != hipSuccess) { set_last_error(std::string("agpu_supporting_end: ") + hipGetErrorString(status)); return AGPU_ERR_DEVICE; }
	return AGPU_OK;
}

int agpu_support_pool_release(agpu_ctx* ctx) {
	if (!ctx) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	if (ctx->support.active) { set_last_error("agpu_support_pool_release: agpu_supporting_end must run first"); return AGPU_ERR_INVALID; }
	(void) hipSetDevice(ctx->device);
	(void) hipStreamSynchronize(ctx->stream);
	ctx->support.release_all();
	return AGPU_OK;
}

int agpu_support_allocated_bytes(agpu_ctx* ctx, uint64_t* bytes) {
	if (!ctx || !bytes) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	*bytes = ctx->support.allocated();
	return AGPU_OK;
}

}
