// arriba_amd/csrc/device/agpu_sorted_bam.hip -- --sorted-bam on the MI355X: the records of the last ingest in coordinate order as stored BGZF blocks, and the arrays of the BAI
// index (include/arriba_gpu.h: agpu_sorted_bam_*).  What decides a byte is sorted_bam_core.hpp, which the host steps as well (arriba_amd/csrc/host/sorted_bam.cpp); here are
//   sorted_bam_key_kernel          one lane per record: key, size, end coordinate (through ingest.record_offset; the stream is const)
//   rocPRIM radix sort of (64-bit key, 32-bit record number) -- stable --, sorted_bam_sizes_kernel + exclusive scan: the uncompressed offset of every record of the output
//   sorted_bam_block_first_kernel  one lane per BGZF block: the record its first payload byte belongs to (binary search, once, so that the gather does not chase it block by block)
//   sorted_bam_gather_kernel       THE HOT PATH, one workgroup per block: the parts of the records that fall into its 0xff00 bytes gathered into an LDS image of the block (source
//                                  read with aligned words and shifts, one wavefront per record), the CRC-32 of the payload taken from LDS (64 bytes per lane, joined pairwise with
//                                  the operators of crc32_core.hpp), header, payload and trailer stored with 16-byte stores.  Source bytes are read once, output bytes written once.
//   sorted_bam_deflate_kernel      --sorted-bam-compression 1: the gather with a compressor behind it (deflate_out_core.hpp: LZ77 tokens by 16 wavefronts with a hash table each,
//                                  histograms, Huffman codes, the bits OR-ed into the LDS image), a block of its real size into its staging slot and the size into a table;
//   sorted_bam_compact_kernel      one wavefront per block packs a window of such blocks.  Neither runs at level 0, and none of their buffers exists then.
//   sorted_bam_index_*_kernel      per record of the file: bin, virtual offsets, run heads of (reference, bin), 64-bit atomicMin into the 16 kb windows, the pseudo-bin's counts
// Integer and byte work, bound by HBM and by the latency of the three dependent loads in front of a record's bytes; no MFMA.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <rocprim/rocprim.hpp>
#define AGPU_OPTION "--sorted-bam"
#define AGPU_ALLOC_MESSAGE(buffer) "hipMalloc failed (" buffer ")"
#include "resident_stream.hpp"
#include "crc32_core.hpp"
#include "deflate_out_core.hpp"
#include "markdup_core.hpp"
#include "device_utils.hpp"
#include "sorted_bam_core.hpp"
#include "sorted_bam_device.hpp"

using namespace agpu;

namespace {

const int GATHER_THREADS = SBAM_GATHER_THREADS; // (the frame of a block and the copy of a record: sorted_bam_device.hpp, shared with agpu_supporting.hip)
const uint32_t GATHER_BATCH = 512;        // records whose source and destination are looked up together
const uint64_t DEFAULT_WINDOW_BYTES = 256ull << 20;

// end_flag: the end coordinate (0 .. 2^29), bit 31: the record is unmapped (flag 0x4)
__global__ void __launch_bounds__(BLOCK) sorted_bam_key_kernel(const uint8_t* stream, uint64_t stream_size, const uint64_t* record_offset, uint64_t n, uint64_t* keys, uint32_t* sizes, uint32_t* end_flag) {
	const uint64_t r = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (r >= n) return;
	const uint64_t at = record_offset[r];
	if (at >= stream_size) { keys[r] = sbam_key(-1, -1, 4); sizes[r] = 0; end_flag[r] = 0x80000000u; return; } // (not what the ingest leaves behind; nothing is read there)
	const SbamRecord record = sbam_parse(stream, at, stream_size);
	keys[r] = record.key; sizes[r] = record.size; end_flag[r] = (uint32_t) record.end | ((record.flag & 4u) ? 0x80000000u : 0u);
}

// sizes in the order of the file, one entry more (0) for the scan that gives out_offset[n] = all bytes
__global__ void __launch_bounds__(BLOCK) sorted_bam_sizes_kernel(const uint32_t* sizes, const uint32_t* order, uint64_t n, uint32_t* sizes_sorted) {
	const uint64_t i = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (i > n) return;
	sizes_sorted[i] = i < n ? sizes[order[i]] : 0;
}

// block_first[b]: the last record i with out_offset[i] <= b * SBAM_PAYLOAD (n > 0, out_offset[0] = 0)
__global__ void __launch_bounds__(BLOCK) sorted_bam_block_first_kernel(const uint64_t* out_offset, uint64_t n, uint64_t n_blocks, uint32_t* block_first) {
	const uint64_t b = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (b >= n_blocks) return;
	const uint64_t target = b * SBAM_PAYLOAD;
	uint64_t low = 0, high = n; // out_offset[low] <= target < out_offset[high]
	while (high - low > 1) { const uint64_t middle = low + (high - low) / 2; if (out_offset[middle] <= target) low = middle; else high = middle; }
	block_first[b] = (uint32_t) low;
}

struct GatherShared {
	SbamFrameShared frame;
	uint64_t source[GATHER_BATCH];           // where the record begins in the stream
	uint64_t destination[GATHER_BATCH + 1];  // ... and in the uncompressed output; (the CRCs of the lanes lie over `source` later)
};
static_assert(sizeof(uint64_t) * GATHER_BATCH >= sizeof(uint32_t) * GATHER_THREADS, "the CRCs of the lanes fit where the sources were");
static_assert(sizeof(GatherShared) * 2 <= 160 * 1024, "two workgroups per CU");

// The parts of the records that fall into block b (payload bytes begin .. begin + length of the output) into image[payload_at ..): one wavefront per record, the batches of
// sources and destinations through LDS.  Shared: GatherShared, or a struct that begins like it.  No barrier behind the last copy.
// duplicate (--mark-duplicates; may be null: the bytes of the stream as they are): one byte per record of the stream, not 0 if it leaves with bit 0x400.  The bit travels in bit 63 of
// the record's source; behind the copy of the record one lane sets or clears MDUP_FLAG_MASK in byte MDUP_FLAG_BYTE of the record in the image, if that byte lies in this block -- a
// byte store: the words around it may hold bytes of the neighbouring records, which other wavefronts copy.
const uint64_t GATHER_DUPLICATE_BIT = 1ull << 63;
template <class Shared> __device__ __forceinline__ void gather_payload(Shared& shared, const uint8_t* __restrict__ stream, const uint64_t* __restrict__ record_offset, const uint32_t* __restrict__ order,
		const uint64_t* __restrict__ out_offset, const uint32_t* __restrict__ block_first, uint64_t n, uint64_t n_blocks, uint64_t b, uint64_t begin, uint32_t length, uint8_t* image, uint32_t payload_at, uint32_t t, const uint8_t* __restrict__ duplicate) {
	const uint32_t lane = t % 64, wave = t / 64;
	const uint64_t first_record = block_first[b], last_record = b + 1 < n_blocks ? block_first[b + 1] : n - 1;
	for (uint64_t batch = first_record; batch <= last_record; batch += GATHER_BATCH) {
		const uint32_t count = (uint32_t) (last_record - batch + 1 < GATHER_BATCH ? last_record - batch + 1 : GATHER_BATCH);
		__syncthreads(); // (the batch before has been copied)
		for (uint32_t j = t; j <= count; j += GATHER_THREADS) {
			shared.destination[j] = out_offset[batch + j]; // (batch + count <= n: out_offset has n + 1 entries)
			if (j < count) {
				const uint32_t record = order[batch + j];
				uint64_t source = record_offset[record];
				if (duplicate != nullptr && duplicate[record] != 0) source |= GATHER_DUPLICATE_BIT;
				shared.source[j] = source;
			}
		}
		__syncthreads();
		for (uint32_t j = wave; j < count; j += GATHER_THREADS / 64) {
			const uint64_t record_begin = shared.destination[j], record_end = shared.destination[j + 1];
			const uint64_t from = record_begin > begin ? record_begin : begin, to = record_end < begin + length ? record_end : begin + length;
			if (from >= to) continue;
			const uint64_t source = shared.source[j];
			sbam_wave_copy<uint32_t>(image, payload_at + (uint32_t) (from - begin), payload_at + (uint32_t) (to - begin), stream, (source & ~GATHER_DUPLICATE_BIT) + (from - record_begin), lane);
			if (duplicate != nullptr) {
				const uint64_t flag_byte = record_begin + MDUP_FLAG_BYTE;
				__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); // (the byte was written by a lane of this wavefront)
				if (lane == 0 && flag_byte >= from && flag_byte < to) {
					uint8_t* const byte = image + payload_at + (uint32_t) (flag_byte - begin);
					*byte = (uint8_t) ((*byte & ~MDUP_FLAG_MASK) | ((source & GATHER_DUPLICATE_BIT) ? MDUP_FLAG_MASK : 0u));
				}
			}
		}
	}
}

// One workgroup per BGZF block: block first_block + blockIdx.x of the file goes to out + blockIdx.x * SBAM_BLOCK.  n > 0.
__global__ void __launch_bounds__(GATHER_THREADS) sorted_bam_gather_kernel(const uint8_t* __restrict__ stream, const uint64_t* __restrict__ record_offset, const uint32_t* __restrict__ order,
		const uint64_t* __restrict__ out_offset, const uint32_t* __restrict__ block_first, uint64_t n, uint64_t total_bytes, uint64_t n_blocks, uint64_t first_block, const Crc32Tables* __restrict__ tables, uint8_t* out, const uint8_t* __restrict__ duplicate) {
	__shared__ GatherShared shared;
	const uint32_t t = threadIdx.x;
	const uint64_t b = first_block + blockIdx.x;
	if (b >= n_blocks) return;
	const uint64_t begin = b * SBAM_PAYLOAD;
	const uint32_t length = (uint32_t) (total_bytes - begin < SBAM_PAYLOAD ? total_bytes - begin : SBAM_PAYLOAD);
	uint8_t* const block_out = out + (uint64_t) blockIdx.x * SBAM_BLOCK;
	const uint32_t pad = (uint32_t) ((uint64_t) block_out & 15u); // image byte pad + i is byte i of the block: 16-byte chunks of the image are 16-byte chunks of memory
	uint8_t* const image = (uint8_t*) shared.frame.image;
	const uint32_t payload_at = pad + SBAM_HEAD;
	sbam_frame_begin(shared.frame, tables, pad, length, t);

	gather_payload(shared, stream, record_offset, order, out_offset, block_first, n, n_blocks, b, begin, length, image, payload_at, t, duplicate);
	__syncthreads();
	sbam_frame_finish(shared.frame, (uint32_t*) shared.source, pad, length, block_out, t);
}


// ---- --sorted-bam-compression 1 ----

const uint32_t DEFLATE_GRID = 512;                       // blocks of one launch: two rounds over the CUs (the LDS of a CU holds one workgroup)
const uint32_t DEFLATE_TOKEN_WORDS = DFO_ROUND * GATHER_THREADS; // the token words of one workgroup in "sortedbam.tokens": position p at (p % 64) * 1024 + p / 64, so that a wavefront
                                                         // stores a round to 64 lines once and the lanes, each with 64 positions in a row of its own, read whole lines twice
static_assert(DFO_ROUND == 64 && SBAM_PAYLOAD <= DFO_ROUND * GATHER_THREADS && SBAM_PAYLOAD <= DFO_MAX_SEGMENTS * DFO_SEGMENT && DFO_MAX_SEGMENTS == GATHER_THREADS / 64, "a wavefront per segment, a round per wavefront, 64 positions per lane");

struct DeflateShared {
	SbamFrameShared frame;
	uint64_t source[GATHER_BATCH];
	uint64_t destination[GATHER_BATCH + 1];
	uint32_t partial[GATHER_THREADS];                    // the CRCs of the lanes; then the scan of the bits of the lanes
	uint32_t table[DFO_MAX_SEGMENTS][DFO_HASH_SLOTS];    // position + 1 of the last occurrence of a hash in the segment of the wavefront
	DfoState state;
};
static_assert(sizeof(DeflateShared) <= 160 * 1024, "one workgroup per CU");

struct LdsOr { uint32_t* words; __device__ __forceinline__ void operator()(uint32_t word, uint32_t bits) const { if (bits != 0) atomicOr(&words[word], bits); } };

// One workgroup per BGZF block: block k = window_block + blockIdx.x of the window that begins at first_block -- gather, CRC-32 of the payload, tokens, codes, bits; it goes to
// out + k * SBAM_BLOCK with the size it really has, and that size to block_bytes[first_block + k].  tokens: gridDim.x * DEFLATE_TOKEN_WORDS words (a window is launched in
// pieces of DEFLATE_GRID blocks, one behind the other on the stream, over the same token words).  n > 0.
__global__ void __launch_bounds__(GATHER_THREADS) sorted_bam_deflate_kernel(const uint8_t* __restrict__ stream, const uint64_t* __restrict__ record_offset, const uint32_t* __restrict__ order,
		const uint64_t* __restrict__ out_offset, const uint32_t* __restrict__ block_first, uint64_t n, uint64_t total_bytes, uint64_t n_blocks, uint64_t first_block, uint32_t window_block,
		const Crc32Tables* __restrict__ tables, uint8_t* out, uint32_t* tokens, uint32_t* block_bytes, const uint8_t* __restrict__ duplicate) {
	__shared__ DeflateShared shared;
	const uint32_t t = threadIdx.x, lane = t % 64, wave = (uint32_t) __builtin_amdgcn_readfirstlane((int) (t / 64));
	uint32_t* const token = tokens + (uint64_t) blockIdx.x * DEFLATE_TOKEN_WORDS;
	uint8_t* const image = (uint8_t*) shared.frame.image;
	DfoState& state = shared.state;
	{
		const uint32_t k = window_block + blockIdx.x;
		const uint64_t b = first_block + k;
		if (b >= n_blocks) return;
		const uint64_t begin = b * SBAM_PAYLOAD;
		const uint32_t length = (uint32_t) (total_bytes - begin < SBAM_PAYLOAD ? total_bytes - begin : SBAM_PAYLOAD);
		uint8_t* const block_out = out + (uint64_t) k * SBAM_BLOCK;
		const uint32_t pad = (uint32_t) ((uint64_t) block_out & 15u);
		const uint32_t payload_at = pad + SBAM_HEAD;
		sbam_frame_begin(shared.frame, tables, pad, length, t);
		gather_payload(shared, stream, record_offset, order, out_offset, block_first, n, n_blocks, b, begin, length, image, payload_at, t, duplicate);
		for (uint32_t i = t; i < DFO_MAX_SEGMENTS * DFO_HASH_SLOTS; i += GATHER_THREADS) (&shared.table[0][0])[i] = 0;
		for (uint32_t i = t; i < sizeof(DfoState) / 4; i += GATHER_THREADS) ((uint32_t*) &state)[i] = 0;
		__syncthreads();
		const uint32_t crc = sbam_frame_crc(shared.frame, shared.partial, payload_at, length, t);

		// tokens: wavefront w walks segment w in rounds of 64 positions; no barrier in here, the table is the wavefront's own
		const uint8_t* const payload = image + payload_at;
		const uint32_t segment_begin = wave * DFO_SEGMENT;
		if (segment_begin < length) {
			const uint32_t segment_end = dfo_segment_end(segment_begin, length);
			uint32_t* const table = shared.table[wave];
			uint32_t next = segment_begin; // the first position that no token covers yet (the same in all lanes)
			#pragma unroll 1
			for (uint32_t base = segment_begin; base < segment_end; base += DFO_ROUND) {
				const uint32_t count = segment_end - base < DFO_ROUND ? segment_end - base : DFO_ROUND;
				const bool covered = next >= base + count;
				const uint32_t p = base + lane;
				const bool live = lane < count, hashable = live && dfo_hashable(p, segment_end);
				const uint32_t value = hashable ? dfo_load32(payload, p) : 0, slot = dfo_hash(value);
				const uint32_t candidate = hashable && !covered ? table[slot] : 0; // all loads of the round ...
				uint32_t found = 0;
				if (!covered && live && p >= next) found = dfo_find(payload, p, segment_end, candidate, value);
				if (hashable) atomicMax(&table[slot], p + 1);                     // ... before its stores; the maximum does not depend on the order of the lanes
				uint32_t mine = 0;
				if (!covered) { // the greedy parse of the round: a walk from token start to token start
					const uint32_t span = found != 0 ? dfo_token_span(found) : 1;
					uint32_t at = next > base ? next : base;
					while (at < base + count) {
						const uint32_t step = (uint32_t) __builtin_amdgcn_readfirstlane((int) __shfl((int) span, (int) (at - base)));
						if (lane == at - base) mine = found;
						at += step;
					}
					next = at;
				}
				if (live) token[lane * GATHER_THREADS + base / DFO_ROUND] = mine;
			}
		}
		__syncthreads(); // (the token words were written to memory by this workgroup and are read by it: the barrier orders them)

		// histograms: sums, in any order
		{
			uint32_t extra_sum = 0;
			#pragma unroll 1
			for (uint32_t j = 0; j < DFO_ROUND; ++j) {
				const uint32_t p = t * DFO_ROUND + j;
				if (p >= length) break;
				const uint32_t word = token[j * GATHER_THREADS + t];
				if (word == 0) continue;
				uint32_t ll, d, extra;
				dfo_token_symbols(word, ll, d, extra);
				atomicAdd(&state.ll_count[ll], 1u);
				if (d < DFO_D) atomicAdd(&state.d_count[d], 1u);
				extra_sum += extra;
			}
			if (extra_sum != 0) atomicAdd(&state.extra_bits, extra_sum);
			if (t == 0) atomicAdd(&state.ll_count[DFO_END], 1u);
		}
		__syncthreads();
		if (t < DFO_LL) { if (state.ll_count[t] != 0) { state.ll_sorted[dfo_rank(state.ll_count, DFO_LL, t)] = (uint16_t) t; atomicAdd(&state.ll_used, 1u); } }
		else if (t >= 512 && t < 512 + DFO_D) { const uint32_t u = t - 512; if (state.d_count[u] != 0) { state.d_sorted[dfo_rank(state.d_count, DFO_D, u)] = (uint16_t) u; atomicAdd(&state.d_used, 1u); } }
		__syncthreads();
		if (t == 0) dfo_plan_lengths(state);
		__syncthreads();
		if (t < DFO_CL && state.cl_count[t] != 0) { state.cl_sorted[dfo_rank(state.cl_count, DFO_CL, t)] = (uint16_t) t; atomicAdd(&state.cl_used, 1u); }
		__syncthreads();
		if (t == 0) dfo_plan(state, length);
		__syncthreads();

		uint32_t size;
		if (state.btype == DFO_STORED) { // (the same for all lanes) today's bytes
			size = length + SBAM_HEAD + SBAM_TAIL;
			if (t < SBAM_TAIL) image[payload_at + length + t] = sbam_tail_byte(t, crc, length);
			__syncthreads();
		} else {
			if (t < DFO_LL) state.ll_code[t] = (uint16_t) dfo_code_of(state.ll_length, state.ll_first, t);
			else if (t >= 512 && t < 512 + DFO_D) state.d_code[t - 512] = (uint16_t) dfo_code_of(state.d_length, state.d_first, t - 512);
			else if (t >= 640 && t < 640 + DFO_CL) state.cl_code[t - 640] = (uint16_t) dfo_code_of(state.cl_length, state.cl_first, t - 640);
			// the bits of the 64 positions of the lane, and where they begin: an inclusive scan over the lanes
			uint32_t bits = 0;
			#pragma unroll 1
			for (uint32_t j = 0; j < DFO_ROUND; ++j) { const uint32_t p = t * DFO_ROUND + j; if (p >= length) break; bits += dfo_token_bits(state, token[j * GATHER_THREADS + t]); }
			shared.partial[t] = bits;
			for (uint32_t i = t; i < SBAM_IMAGE_BYTES / 16; i += GATHER_THREADS) shared.frame.image[i] = make_uint4(0, 0, 0, 0); // (nobody reads the payload any more: the tokens hold the literals)
			__syncthreads();
			for (uint32_t stride = 1; stride < GATHER_THREADS; stride *= 2) {
				const uint32_t before = t >= stride ? shared.partial[t - stride] : 0;
				__syncthreads();
				shared.partial[t] += before;
				__syncthreads();
			}
			const LdsOr or_word = { (uint32_t*) shared.frame.image };
			const uint32_t data_bytes = (state.total_bits + 7) / 8;
			size = dfo_block_bytes(state.total_bits);
			if (t < 18) { const uint32_t byte = t < 16 ? sbam_head_byte(t, length) : (uint8_t) ((size - 1) >> (8 * (t - 16))); or_word((pad + t) / 4, byte << (8 * ((pad + t) & 3u))); }
			else if (t < 18 + SBAM_TAIL) { const uint32_t i = t - 18, at = pad + 18 + data_bytes + i; or_word(at / 4, (uint32_t) sbam_tail_byte(i, crc, length) << (8 * (at & 3u))); }
			const uint32_t data_bit = (pad + 18) * 8;
			if (t == 64) dfo_put_header(state, data_bit, or_word);
			if (t == 128) dfo_put(data_bit + state.header_bits + shared.partial[GATHER_THREADS - 1], dfo_end_value(state), dfo_end_bits(state), or_word);
			uint32_t at = data_bit + state.header_bits + (shared.partial[t] - bits);
			#pragma unroll 1
			for (uint32_t j = 0; j < DFO_ROUND; ++j) {
				const uint32_t p = t * DFO_ROUND + j;
				if (p >= length) break;
				const uint32_t word = token[j * GATHER_THREADS + t];
				if (word == 0) continue;
				dfo_put_token(state, at, word, or_word);
				at += dfo_token_bits(state, word);
			}
			__syncthreads();
		}
		sbam_frame_store(shared.frame, pad, size, block_out, t);
		if (t == 0) block_bytes[b] = size;
	}
}

// One wavefront per block of the window: its bytes from its staging slot to their packed place.  window_offset: exclusive scan of the sizes (blocks + 1 entries).  Launched in
// chunks (for_each_wave_chunk): `first` is the block of the first wavefront.
__global__ void __launch_bounds__(BLOCK) sorted_bam_compact_kernel(const uint8_t* __restrict__ staging, const uint64_t* __restrict__ window_offset, uint64_t blocks, uint8_t* packed, uint64_t first) {
	const uint64_t k = first + ((uint64_t) blockIdx.x * BLOCK + threadIdx.x) / 64;
	if (k >= blocks) return;
	sbam_wave_copy<uint64_t>(packed, window_offset[k], window_offset[k + 1], staging, k * SBAM_BLOCK, threadIdx.x % 64);
}

// ---- the index ----

struct RefStats { unsigned long long begin, end, mapped, unmapped; };
enum { STAT_NO_COOR = 0, STAT_COUNT = 2 };

__device__ __forceinline__ void file_record(const uint64_t* keys_sorted, const uint32_t* order, const uint32_t* end_flag, uint64_t i, int32_t& ref, int32_t& pos, int32_t& end, bool& unmapped) {
	const uint64_t key = keys_sorted[i];
	ref = (int32_t) (uint32_t) (key >> 32); pos = (int32_t) ((uint32_t) (key >> 1) & 0x7FFFFFFFu) - 1;
	const uint32_t word = end_flag[order[i]];
	end = (int32_t) (word & 0x7FFFFFFFu); unmapped = (word >> 31) != 0;
}

// One lane per record of the file: the pseudo-bin's numbers, the run heads of (reference, bin), the windows of the linear index
__global__ void __launch_bounds__(BLOCK) sorted_bam_index_record_kernel(const uint64_t* keys_sorted, const uint32_t* order, const uint32_t* end_flag, const uint64_t* out_offset, uint64_t n, uint64_t first_block_file_offset,
		const uint64_t* block_file_offset /* compressed blocks: where every block begins in the file; nullptr: stored blocks */, const uint32_t* ref_length, uint32_t n_ref, const uint64_t* interval_offset, unsigned long long* intervals, RefStats* stats, unsigned long long* counters, uint32_t* heads) {
	const uint64_t i = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	const bool live = i < n;
	int32_t ref = -1, pos = -1, end = 0; bool unmapped = true;
	if (live) file_record(keys_sorted, order, end_flag, i, ref, pos, end, unmapped);
	// counts: the records of a workgroup are nearly always of one reference (the file is sorted): one atomic per workgroup then
	const uint64_t block_begin = (uint64_t) blockIdx.x * BLOCK, block_last = (block_begin + BLOCK <= n ? block_begin + BLOCK : n) - 1;
	const uint32_t first_ref = (uint32_t) (keys_sorted[block_begin] >> 32), last_ref = (uint32_t) (keys_sorted[block_last] >> 32);
	if (first_ref == last_ref) {
		const int n_unmapped = __syncthreads_count(live && unmapped), n_live = (int) (block_last - block_begin + 1);
		if (threadIdx.x == 0) {
			if ((int32_t) first_ref < 0) atomicAdd(&counters[STAT_NO_COOR], (unsigned long long) n_live);
			else if (first_ref < n_ref) { if (n_unmapped > 0) atomicAdd(&stats[first_ref].unmapped, (unsigned long long) n_unmapped); if (n_live > n_unmapped) atomicAdd(&stats[first_ref].mapped, (unsigned long long) (n_live - n_unmapped)); }
		}
	} else if (live) {
		if (ref < 0) atomicAdd(&counters[STAT_NO_COOR], 1ull);
		else if ((uint32_t) ref < n_ref) atomicAdd(unmapped ? &stats[ref].unmapped : &stats[ref].mapped, 1ull);
	}
	if (!live) return;
	const uint64_t begin_offset = block_file_offset ? sbam_voffset(block_file_offset, out_offset[i]) : sbam_voffset(first_block_file_offset, out_offset[i]);
	const uint64_t end_offset = block_file_offset ? sbam_voffset(block_file_offset, out_offset[i + 1]) : sbam_voffset(first_block_file_offset, out_offset[i + 1]);
	const uint64_t key_before = i > 0 ? keys_sorted[i - 1] : 0, key_behind = i + 1 < n ? keys_sorted[i + 1] : 0;
	if (ref >= 0 && (uint32_t) ref < n_ref) { // the records of a reference lie next to each other: its first and its last one write its range
		if (i == 0 || (uint32_t) (key_before >> 32) != (uint32_t) ref) stats[ref].begin = begin_offset;
		if (i + 1 == n || (uint32_t) (key_behind >> 32) != (uint32_t) ref) stats[ref].end = end_offset;
	}
	uint32_t head = 0;
	if (sbam_indexed(ref, pos, n_ref)) {
		head = 1;
		if (i > 0) {
			int32_t ref_before, pos_before, end_before; bool unmapped_before;
			file_record(keys_sorted, order, end_flag, i - 1, ref_before, pos_before, end_before, unmapped_before);
			if (sbam_indexed(ref_before, pos_before, n_ref) && sbam_chunk_key(ref_before, sbam_reg2bin(pos_before, end_before)) == sbam_chunk_key(ref, sbam_reg2bin(pos, end))) head = 0;
		}
		uint64_t first, last;
		if (sbam_window_range(pos, end, sbam_windows_of(ref_length[ref]), first, last))
			for (uint64_t w = first; w <= last; ++w) {
				unsigned long long* slot = &intervals[interval_offset[ref] + w];
				if (*(volatile unsigned long long*) slot > begin_offset) atomicMin(slot, (unsigned long long) begin_offset); // (the value only ever falls: a stale read costs one atomic more)
			}
	}
	heads[i] = head;
}

// chunk_id: exclusive scan of heads (n + 1 entries).  The head of a run writes key and begin of its chunk, the last record of the run its end.
__global__ void __launch_bounds__(BLOCK) sorted_bam_index_chunk_kernel(const uint64_t* keys_sorted, const uint32_t* order, const uint32_t* end_flag, const uint64_t* out_offset, uint64_t n, uint64_t first_block_file_offset,
		const uint64_t* block_file_offset, uint32_t n_ref, const uint32_t* heads, const uint32_t* chunk_id, uint64_t* chunk_key, uint64_t* chunk_begin, uint64_t* chunk_end) {
	const uint64_t i = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (i >= n) return;
	int32_t ref, pos, end; bool unmapped;
	file_record(keys_sorted, order, end_flag, i, ref, pos, end, unmapped);
	if (!sbam_indexed(ref, pos, n_ref)) return;
	const uint32_t chunk = chunk_id[i + 1] - 1;
	if (heads[i]) { chunk_key[chunk] = sbam_chunk_key(ref, sbam_reg2bin(pos, end)); chunk_begin[chunk] = block_file_offset ? sbam_voffset(block_file_offset, out_offset[i]) : sbam_voffset(first_block_file_offset, out_offset[i]); }
	bool last = i + 1 == n || heads[i + 1] != 0;
	if (!last) { const uint64_t key = keys_sorted[i + 1]; last = !sbam_indexed((int32_t) (uint32_t) (key >> 32), (int32_t) ((uint32_t) (key >> 1) & 0x7FFFFFFFu) - 1, n_ref); }
	if (last) chunk_end[chunk] = block_file_offset ? sbam_voffset(block_file_offset, out_offset[i + 1]) : sbam_voffset(first_block_file_offset, out_offset[i + 1]);
}

// One lane per reference: empty windows take the offset of the next window that has one, 0 if there is none (the offsets of a reference rise with the window)
__global__ void __launch_bounds__(BLOCK) sorted_bam_index_fill_kernel(const uint64_t* interval_offset, uint32_t n_ref, unsigned long long* intervals, RefStats* stats) {
	const uint32_t ref = blockIdx.x * BLOCK + threadIdx.x;
	if (ref >= n_ref) return;
	if (stats[ref].begin == SBAM_NO_OFFSET) stats[ref].begin = 0;
	unsigned long long next = 0;
	for (uint64_t w = interval_offset[ref + 1]; w-- > interval_offset[ref]; ) { const unsigned long long value = intervals[w]; if (value == SBAM_NO_OFFSET) intervals[w] = next; else next = value; }
}

__global__ void __launch_bounds__(BLOCK) sorted_bam_index_order_kernel(const uint32_t* chunk_order, uint64_t n_chunks, const uint64_t* chunk_begin, const uint64_t* chunk_end, uint64_t* out /* [2 * n_chunks]: begins, ends */) {
	const uint64_t c = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (c >= n_chunks) return;
	out[c] = chunk_begin[chunk_order[c]]; out[n_chunks + c] = chunk_end[chunk_order[c]];
}

const char* const COMPRESSION_BUFFERS[] = { "sortedbam.tokens", "sortedbam.block_bytes", "sortedbam.window_offset", "sortedbam.packed", "sortedbam.block_offset" }; // what level 1 adds

int launch_gather(agpu_ctx* ctx, uint64_t first_block) {
	const uint64_t blocks = std::min<uint64_t>(ctx->sorted_bam_window_blocks, ctx->sorted_bam_blocks - first_block);
	const uint64_t bytes = std::min<uint64_t>(blocks * SBAM_PAYLOAD, ctx->sorted_bam_bytes - first_block * SBAM_PAYLOAD);
	const uint8_t* const duplicate = ctx->markdup.on ? ctx->markdup.buffer("markdup.flag").as<uint8_t>() : nullptr; // (--mark-duplicates off: the kernels do what they did without it)
	if (ctx->sorted_bam_level == 0) {
		KernelTimer timer(ctx, "sorted_bam_gather_kernel", 2 * bytes + blocks * (SBAM_HEAD + SBAM_TAIL));
		sorted_bam_gather_kernel<<<(unsigned int) blocks, GATHER_THREADS, 0, ctx->stream>>>(ctx->sorted_bam_stream.stream, ctx->sorted_bam_stream.record_offset, ctx->scratch("sortedbam.order").as<uint32_t>(),
			ctx->scratch("sortedbam.out_offset").as<uint64_t>(), ctx->scratch("sortedbam.block_first").as<uint32_t>(), ctx->sorted_bam_records, ctx->sorted_bam_bytes, ctx->sorted_bam_blocks, first_block,
			ctx->scratch("sortedbam.crc_tables").as<Crc32Tables>(), ctx->scratch("sortedbam.staging").as<uint8_t>(), duplicate);
	} else { // compressed blocks into their staging slots, their sizes scanned, the blocks packed
		hipStream_t s = ctx->stream;
		DeviceBuffer& block_bytes = ctx->scratch("sortedbam.block_bytes"); DeviceBuffer& window_offset = ctx->scratch("sortedbam.window_offset"); DeviceBuffer& rocprim_scratch = ctx->scratch("sortedbam.rocprim");
		{ KernelTimer timer(ctx, "sorted_bam_deflate_kernel", 2 * bytes);
		  for (uint64_t done = 0; done < blocks; done += DEFLATE_GRID)
		  sorted_bam_deflate_kernel<<<(unsigned int) std::min<uint64_t>(blocks - done, DEFLATE_GRID), GATHER_THREADS, 0, s>>>(ctx->sorted_bam_stream.stream, ctx->sorted_bam_stream.record_offset, ctx->scratch("sortedbam.order").as<uint32_t>(),
			ctx->scratch("sortedbam.out_offset").as<uint64_t>(), ctx->scratch("sortedbam.block_first").as<uint32_t>(), ctx->sorted_bam_records, ctx->sorted_bam_bytes, ctx->sorted_bam_blocks, first_block, (uint32_t) done,
			ctx->scratch("sortedbam.crc_tables").as<Crc32Tables>(), ctx->scratch("sortedbam.staging").as<uint8_t>(), ctx->scratch("sortedbam.tokens").as<uint32_t>(), block_bytes.as<uint32_t>(), duplicate); }
		size_t temporary = 0;
		HIP_CHECK(rocprim::exclusive_scan(nullptr, temporary, block_bytes.as<uint32_t>() + first_block, window_offset.as<uint64_t>(), (uint64_t) 0, (size_t) blocks + 1, rocprim::plus<uint64_t>(), s));
		if (temporary > rocprim_scratch.capacity) { HIP_CHECK(hipStreamSynchronize(s)); ALLOC(rocprim_scratch, temporary); }
		{ KernelTimer timer(ctx, "sorted_bam rocprim::exclusive_scan(blocks)", blocks * 12);
		  HIP_CHECK(rocprim::exclusive_scan(rocprim_scratch.ptr, temporary, block_bytes.as<uint32_t>() + first_block, window_offset.as<uint64_t>(), (uint64_t) 0, (size_t) blocks + 1, rocprim::plus<uint64_t>(), s)); }
		{ KernelTimer timer(ctx, "sorted_bam_compact_kernel", 2 * bytes);
		  uint8_t* const staging = ctx->scratch("sortedbam.staging").as<uint8_t>(); uint8_t* const packed = ctx->scratch("sortedbam.packed").as<uint8_t>();
		  for_each_wave_chunk(blocks, [&](uint64_t first, uint64_t count) { sorted_bam_compact_kernel<<<(unsigned int) ((count * 64 + BLOCK - 1) / BLOCK), BLOCK, 0, s>>>(staging, window_offset.as<uint64_t>(), blocks, packed, first); }); }
	}
	ctx->sorted_bam_gathered_block = first_block;
	return AGPU_OK;
}

int build_index(agpu_ctx* ctx, uint64_t first_block_file_offset, const uint32_t* ref_length, uint32_t n_ref) {
	hipStream_t s = ctx->stream;
	const uint64_t n = ctx->sorted_bam_records;
	DeviceBuffer& lengths = ctx->scratch("sortedbam.ref_length"); DeviceBuffer& interval_offset = ctx->scratch("sortedbam.interval_offset"); DeviceBuffer& intervals = ctx->scratch("sortedbam.intervals");
	DeviceBuffer& stats = ctx->scratch("sortedbam.ref_stats"); DeviceBuffer& heads = ctx->scratch("sortedbam.heads"); DeviceBuffer& chunk_id = ctx->scratch("sortedbam.chunk_id"); DeviceBuffer& rocprim_scratch = ctx->scratch("sortedbam.rocprim");
	std::vector<uint64_t> host_interval_offset((size_t) n_ref + 1, 0);
	for (uint32_t t = 0; t < n_ref; ++t) host_interval_offset[t + 1] = host_interval_offset[t] + sbam_windows_of(ref_length[t]);
	const uint64_t n_intervals = host_interval_offset[n_ref];
	ALLOC(lengths, std::max<size_t>(n_ref, 1) * 4); ALLOC(interval_offset, ((size_t) n_ref + 1) * 8); ALLOC(intervals, std::max<uint64_t>(n_intervals, 1) * 8);
	ALLOC(stats, ((size_t) n_ref + 1) * sizeof(RefStats)); ALLOC(heads, (n + 1) * 4); ALLOC(chunk_id, (n + 1) * 4);
	static_assert(sizeof(RefStats) >= STAT_COUNT * 8, "the counters fit an entry");
	unsigned long long* const counters = (unsigned long long*) stats.ptr; // entry 0: the counters; the references behind it
	RefStats* const device_stats = stats.as<RefStats>() + 1;
	std::vector<RefStats> initial((size_t) n_ref + 1);
	memset(initial.data(), 0, initial.size() * sizeof(RefStats));
	for (uint32_t t = 0; t < n_ref; ++t) initial[t + 1].begin = SBAM_NO_OFFSET;
	if (n_ref > 0) HIP_CHECK(hipMemcpyAsync(lengths.ptr, ref_length, (size_t) n_ref * 4, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(interval_offset.ptr, host_interval_offset.data(), ((size_t) n_ref + 1) * 8, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(stats.ptr, initial.data(), initial.size() * sizeof(RefStats), hipMemcpyHostToDevice, s));
	HIP_CHECK(hipStreamSynchronize(s)); // (the three sources are pageable memory of this call)
	HIP_CHECK(hipMemsetAsync(intervals.ptr, 0xFF, std::max<uint64_t>(n_intervals, 1) * 8, s));
	uint32_t n_chunks = 0;
	const uint64_t* block_file_offset = nullptr;
	if (n > 0 && ctx->sorted_bam_level != 0) { // where every block begins in the file: the sizes the blocks really have, scanned from first_block_file_offset on
		DeviceBuffer& block_offset = ctx->scratch("sortedbam.block_offset");
		const size_t entries = (size_t) ctx->sorted_bam_blocks + 1;
		size_t temporary = 0;
		HIP_CHECK(rocprim::exclusive_scan(nullptr, temporary, ctx->scratch("sortedbam.block_bytes").as<uint32_t>(), block_offset.as<uint64_t>(), first_block_file_offset, entries, rocprim::plus<uint64_t>(), s));
		if (temporary > rocprim_scratch.capacity) ALLOC(rocprim_scratch, temporary);
		{ KernelTimer timer(ctx, "sorted_bam rocprim::exclusive_scan(offsets)", entries * 12);
		  HIP_CHECK(rocprim::exclusive_scan(rocprim_scratch.ptr, temporary, ctx->scratch("sortedbam.block_bytes").as<uint32_t>(), block_offset.as<uint64_t>(), first_block_file_offset, entries, rocprim::plus<uint64_t>(), s)); }
		block_file_offset = block_offset.as<uint64_t>();
	}
	if (n > 0) {
		const uint64_t* keys_sorted = ctx->scratch("sortedbam.keys_sorted").as<uint64_t>(); const uint32_t* order = ctx->scratch("sortedbam.order").as<uint32_t>();
		const uint32_t* end_flag = ctx->scratch("sortedbam.end_flag").as<uint32_t>(); const uint64_t* out_offset = ctx->scratch("sortedbam.out_offset").as<uint64_t>();
		{ KernelTimer timer(ctx, "sorted_bam_index_record_kernel", n * 40);
		  sorted_bam_index_record_kernel<<<grid_for(n), BLOCK, 0, s>>>(keys_sorted, order, end_flag, out_offset, n, first_block_file_offset, block_file_offset, lengths.as<uint32_t>(), n_ref, interval_offset.as<uint64_t>(),
			intervals.as<unsigned long long>(), device_stats, counters, heads.as<uint32_t>()); }
		HIP_CHECK(hipMemsetAsync(heads.as<uint32_t>() + n, 0, 4, s));
		size_t temporary = 0;
		HIP_CHECK(rocprim::exclusive_scan(nullptr, temporary, heads.as<uint32_t>(), chunk_id.as<uint32_t>(), 0u, (size_t) n + 1, rocprim::plus<uint32_t>(), s));
		if (temporary > rocprim_scratch.capacity) ALLOC(rocprim_scratch, temporary);
		{ KernelTimer timer(ctx, "sorted_bam rocprim::exclusive_scan(run heads)", n * 8);
		  HIP_CHECK(rocprim::exclusive_scan(rocprim_scratch.ptr, temporary, heads.as<uint32_t>(), chunk_id.as<uint32_t>(), 0u, (size_t) n + 1, rocprim::plus<uint32_t>(), s)); }
		HIP_CHECK(hipMemcpyAsync(&n_chunks, chunk_id.as<uint32_t>() + n, 4, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		DeviceBuffer& chunk_key = ctx->scratch("sortedbam.chunk_key"); DeviceBuffer& chunk_begin = ctx->scratch("sortedbam.chunk_begin"); DeviceBuffer& chunk_end = ctx->scratch("sortedbam.chunk_end");
		DeviceBuffer& chunk_key_sorted = ctx->scratch("sortedbam.chunk_key_sorted"); DeviceBuffer& chunk_order = ctx->scratch("sortedbam.chunk_order"); DeviceBuffer& chunk_out = ctx->scratch("sortedbam.chunk_out");
		const size_t room = std::max<size_t>(n_chunks, 1);
		ALLOC(chunk_key, room * 8); ALLOC(chunk_begin, room * 8); ALLOC(chunk_end, room * 8); ALLOC(chunk_key_sorted, room * 8); ALLOC(chunk_order, room * 4); ALLOC(chunk_out, room * 16);
		if (n_chunks > 0) {
			{ KernelTimer timer(ctx, "sorted_bam_index_chunk_kernel", n * 24);
			  sorted_bam_index_chunk_kernel<<<grid_for(n), BLOCK, 0, s>>>(keys_sorted, order, end_flag, out_offset, n, first_block_file_offset, block_file_offset, n_ref, heads.as<uint32_t>(), chunk_id.as<uint32_t>(),
				chunk_key.as<uint64_t>(), chunk_begin.as<uint64_t>(), chunk_end.as<uint64_t>()); }
			temporary = 0;
			HIP_CHECK(rocprim::radix_sort_pairs(nullptr, temporary, chunk_key.as<uint64_t>(), chunk_key_sorted.as<uint64_t>(), rocprim::counting_iterator<uint32_t>(0), chunk_order.as<uint32_t>(), (size_t) n_chunks, 0, 64, s));
			if (temporary > rocprim_scratch.capacity) ALLOC(rocprim_scratch, temporary);
			{ KernelTimer timer(ctx, "sorted_bam rocprim::radix_sort_pairs(chunks)", (uint64_t) n_chunks * 24);
			  HIP_CHECK(rocprim::radix_sort_pairs(rocprim_scratch.ptr, temporary, chunk_key.as<uint64_t>(), chunk_key_sorted.as<uint64_t>(), rocprim::counting_iterator<uint32_t>(0), chunk_order.as<uint32_t>(), (size_t) n_chunks, 0, 64, s)); }
			sorted_bam_index_order_kernel<<<grid_for(n_chunks), BLOCK, 0, s>>>(chunk_order.as<uint32_t>(), n_chunks, chunk_begin.as<uint64_t>(), chunk_end.as<uint64_t>(), chunk_out.as<uint64_t>());
		}
	}
	if (n_ref > 0) { KernelTimer timer(ctx, "sorted_bam_index_fill_kernel", n_intervals * 16);
	  sorted_bam_index_fill_kernel<<<grid_for(n_ref), BLOCK, 0, s>>>(interval_offset.as<uint64_t>(), n_ref, intervals.as<unsigned long long>(), device_stats); }
	unsigned long long host_counters[STAT_COUNT] = { 0, 0 };
	HIP_CHECK(hipMemcpyAsync(host_counters, counters, sizeof(host_counters), hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	ctx->sorted_bam_chunks = n_chunks; ctx->sorted_bam_intervals = n_intervals; ctx->sorted_bam_no_coor = host_counters[STAT_NO_COOR]; ctx->sorted_bam_n_ref = n_ref;
	ctx->sorted_bam_index_first = first_block_file_offset; ctx->sorted_bam_index_ready = true;
	collect_kernel_samples(ctx);
	return AGPU_OK;
}

}

extern "C" {

int agpu_sorted_bam_begin(agpu_ctx* ctx, agpu_sorted_bam_info* info) {
	if (!ctx || !info) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	ResidentStream& resident = ctx->sorted_bam_stream;
	TRY(resident_stream(ctx, "agpu_sorted_bam_begin", "a sorted BAM file of one sample over several GPUs is not supported", ctx->sorted_bam_active ? "agpu_sorted_bam_end must run first" : nullptr, resident));
	const uint64_t size = resident.stream_size, base = resident.first_record, n = resident.records;
	HIP_CHECK(hipSetDevice(ctx->device));
	hipStream_t s = ctx->stream;
	ctx->sorted_bam_active = true; // (from here on nothing of this context is given back when an allocation fails: DeviceBuffer::release_idle_buffers)
	struct Guard { agpu_ctx* ctx; bool keep; ~Guard() { if (!keep) { ctx->sorted_bam_active = false; ctx->markdup.on = false; ctx->markdup.release_all(); } } } guard = { ctx, false };
	// --mark-duplicates: one byte per record, found now -- its working buffers are gone before those of the file are allocated, so the two peaks do not add
	const bool mark_duplicates = ctx->markdup.next;
	if (mark_duplicates) TRY(markdup_find(ctx, resident));
	const uint64_t bytes = size - base, n_blocks = sbam_block_count(bytes);
	uint64_t window_bytes = DEFAULT_WINDOW_BYTES;
	{ const char* knob = getenv("ARRIBA_SORTED_BAM_WINDOW"); if (knob != nullptr && knob[0] != 0) window_bytes = strtoull(knob, nullptr, 10); }
	const uint64_t window_blocks = std::max<uint64_t>(std::min<uint64_t>(window_bytes / SBAM_BLOCK, 1u << 20), 1);
	DeviceBuffer& keys = ctx->scratch("sortedbam.keys"); DeviceBuffer& keys_sorted = ctx->scratch("sortedbam.keys_sorted"); DeviceBuffer& order = ctx->scratch("sortedbam.order"); DeviceBuffer& sizes = ctx->scratch("sortedbam.sizes");
	DeviceBuffer& sizes_sorted = ctx->scratch("sortedbam.sizes_sorted"); DeviceBuffer& end_flag = ctx->scratch("sortedbam.end_flag"); DeviceBuffer& out_offset = ctx->scratch("sortedbam.out_offset");
	DeviceBuffer& block_first = ctx->scratch("sortedbam.block_first"); DeviceBuffer& staging = ctx->scratch("sortedbam.staging"); DeviceBuffer& rocprim_scratch = ctx->scratch("sortedbam.rocprim"); DeviceBuffer& crc_tables = ctx->scratch("sortedbam.crc_tables");
	const size_t room = std::max<uint64_t>(n, 1);
	ALLOC(keys, room * 8); ALLOC(keys_sorted, room * 8); ALLOC(order, room * 4); ALLOC(sizes, room * 4); ALLOC(sizes_sorted, (room + 1) * 4); ALLOC(end_flag, room * 4); ALLOC(out_offset, (room + 1) * 8);
	ALLOC(block_first, std::max<uint64_t>(n_blocks, 1) * 4); ALLOC(staging, std::max<uint64_t>(std::min(window_blocks, n_blocks), 1) * SBAM_BLOCK);
	if (crc_tables.ptr == nullptr) {
		ALLOC(crc_tables, sizeof(Crc32Tables));
		static Crc32Tables tables; static bool made = false; static std::mutex mutex;
		{ std::lock_guard<std::mutex> lock(mutex); if (!made) { crc32_make_tables(tables); made = true; } }
		HIP_CHECK(hipMemcpy(crc_tables.ptr, &tables, sizeof(tables), hipMemcpyHostToDevice));
	}
	const int level = ctx->sorted_bam_level_next;
	if (level != 0) { // (at level 0 none of these exists)
		DeviceBuffer& tokens = ctx->scratch("sortedbam.tokens"); DeviceBuffer& block_bytes = ctx->scratch("sortedbam.block_bytes"); DeviceBuffer& window_offset = ctx->scratch("sortedbam.window_offset");
		DeviceBuffer& packed = ctx->scratch("sortedbam.packed"); DeviceBuffer& block_offset = ctx->scratch("sortedbam.block_offset");
		const uint64_t held = std::max<uint64_t>(std::min(window_blocks, n_blocks), 1);
		ALLOC(tokens, std::min<uint64_t>(held, DEFLATE_GRID) * DEFLATE_TOKEN_WORDS * 4); ALLOC(block_bytes, (n_blocks + 1) * 4); ALLOC(window_offset, (held + 1) * 8); ALLOC(packed, held * SBAM_BLOCK); ALLOC(block_offset, (n_blocks + 1) * 8);
		HIP_CHECK(hipMemsetAsync(block_bytes.ptr, 0, (n_blocks + 1) * 4, s));
	}
	uint64_t total = 0;
	if (n > 0) {
		{ KernelTimer timer(ctx, "sorted_bam_key_kernel", n * 24 + bytes / 4);
		  sorted_bam_key_kernel<<<grid_for(n), BLOCK, 0, s>>>(resident.stream, size, resident.record_offset, n, keys.as<uint64_t>(), sizes.as<uint32_t>(), end_flag.as<uint32_t>()); }
		size_t temporary = 0;
		HIP_CHECK(rocprim::radix_sort_pairs(nullptr, temporary, keys.as<uint64_t>(), keys_sorted.as<uint64_t>(), rocprim::counting_iterator<uint32_t>(0), order.as<uint32_t>(), (size_t) n, 0, 64, s));
		if (temporary > rocprim_scratch.capacity) ALLOC(rocprim_scratch, temporary);
		{ KernelTimer timer(ctx, "sorted_bam rocprim::radix_sort_pairs(records)", n * 24);
		  HIP_CHECK(rocprim::radix_sort_pairs(rocprim_scratch.ptr, temporary, keys.as<uint64_t>(), keys_sorted.as<uint64_t>(), rocprim::counting_iterator<uint32_t>(0), order.as<uint32_t>(), (size_t) n, 0, 64, s)); }
		sorted_bam_sizes_kernel<<<grid_for(n + 1), BLOCK, 0, s>>>(sizes.as<uint32_t>(), order.as<uint32_t>(), n, sizes_sorted.as<uint32_t>());
		temporary = 0;
		HIP_CHECK(rocprim::exclusive_scan(nullptr, temporary, sizes_sorted.as<uint32_t>(), out_offset.as<uint64_t>(), (uint64_t) 0, (size_t) n + 1, rocprim::plus<uint64_t>(), s));
		if (temporary > rocprim_scratch.capacity) ALLOC(rocprim_scratch, temporary);
		{ KernelTimer timer(ctx, "sorted_bam rocprim::exclusive_scan(sizes)", n * 12);
		  HIP_CHECK(rocprim::exclusive_scan(rocprim_scratch.ptr, temporary, sizes_sorted.as<uint32_t>(), out_offset.as<uint64_t>(), (uint64_t) 0, (size_t) n + 1, rocprim::plus<uint64_t>(), s)); }
		HIP_CHECK(hipMemcpyAsync(&total, out_offset.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		if (total != bytes) { set_last_error("agpu_sorted_bam_begin: the records of the stream do not add up to its size"); return AGPU_ERR_INVALID; } // (then the blocks would not be what `info` says: nothing is gathered)
		{ KernelTimer timer(ctx, "sorted_bam_block_first_kernel", n_blocks * 4);
		  sorted_bam_block_first_kernel<<<grid_for(n_blocks), BLOCK, 0, s>>>(out_offset.as<uint64_t>(), n, n_blocks, block_first.as<uint32_t>()); }
		HIP_CHECK(hipStreamSynchronize(s));
		HIP_CHECK(hipGetLastError());
	} else if (bytes != 0) { set_last_error("agpu_sorted_bam_begin: the records of the stream do not add up to its size"); return AGPU_ERR_INVALID; }
	ctx->sorted_bam_records = n; ctx->sorted_bam_bytes = bytes; ctx->sorted_bam_blocks = n_blocks; ctx->sorted_bam_window_blocks = window_blocks; ctx->sorted_bam_next_block = 0; ctx->sorted_bam_gathered_block = ~0ull;
	ctx->sorted_bam_index_ready = false; ctx->sorted_bam_level = level; ctx->sorted_bam_level_next = 0; ctx->sorted_bam_compressed_bytes = 0;
	ctx->markdup.on = mark_duplicates; ctx->markdup.next = false;
	memset(info, 0, sizeof(*info));
	info->records = n; info->uncompressed_bytes = bytes; info->file_bytes = bytes + n_blocks * (SBAM_HEAD + SBAM_TAIL); info->windows = (n_blocks + window_blocks - 1) / window_blocks;
	info->window_bytes = std::max<uint64_t>(std::min(window_blocks, n_blocks), 1) * SBAM_BLOCK;
	collect_kernel_samples(ctx);
	guard.keep = true;
	return AGPU_OK;
}

int agpu_sorted_bam_set_compression(agpu_ctx* ctx, int level) {
	if (!ctx) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	if (level != 0 && level != 1) { set_last_error("agpu_sorted_bam_set_compression: the level is 0 (stored blocks) or 1, not " + std::to_string(level)); return AGPU_ERR_INVALID; }
	if (ctx->sorted_bam_active) { set_last_error("agpu_sorted_bam_set_compression: it comes before agpu_sorted_bam_begin"); return AGPU_ERR_INVALID; }
	ctx->sorted_bam_level_next = level;
	return AGPU_OK;
}

int agpu_sorted_bam_compressed_bytes(agpu_ctx* ctx, uint64_t* bytes) {
	if (!ctx || !bytes) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	if (!ctx->sorted_bam_active || ctx->sorted_bam_next_block < ctx->sorted_bam_blocks) { set_last_error("agpu_sorted_bam_compressed_bytes: valid between the agpu_sorted_bam_next that fetched the last window and agpu_sorted_bam_end"); return AGPU_ERR_INVALID; }
	*bytes = ctx->sorted_bam_compressed_bytes;
	return AGPU_OK;
}

int agpu_sorted_bam_compression_allocated_bytes(agpu_ctx* ctx, uint64_t* bytes) {
	if (!ctx || !bytes) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	uint64_t sum = 0;
	for (const char* name : COMPRESSION_BUFFERS) sum += ctx->scratch(name).capacity;
	*bytes = sum;
	return AGPU_OK;
}

int agpu_sorted_bam_next(agpu_ctx* ctx, void* pinned, uint64_t capacity, uint64_t* bytes) {
	if (!ctx || !bytes) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	if (!ctx->sorted_bam_active) { set_last_error("agpu_sorted_bam_begin must run first"); return AGPU_ERR_INVALID; }
	*bytes = 0;
	if (ctx->sorted_bam_next_block >= ctx->sorted_bam_blocks) return AGPU_OK;
	HIP_CHECK(hipSetDevice(ctx->device));
	hipStream_t s = ctx->stream;
	const uint64_t first = ctx->sorted_bam_next_block, blocks = std::min<uint64_t>(ctx->sorted_bam_window_blocks, ctx->sorted_bam_blocks - first);
	const uint64_t payload = std::min<uint64_t>(blocks * SBAM_PAYLOAD, ctx->sorted_bam_bytes - first * SBAM_PAYLOAD), window = payload + blocks * (SBAM_HEAD + SBAM_TAIL);
	if (!pinned || capacity < window) { set_last_error("agpu_sorted_bam_next: the buffer is smaller than a window (agpu_sorted_bam_info.window_bytes)"); return AGPU_ERR_INVALID; }
	if (ctx->sorted_bam_gathered_block != first) TRY(launch_gather(ctx, first));
	const void* from = ctx->scratch("sortedbam.staging").ptr;
	uint64_t fetched = window;
	if (ctx->sorted_bam_level != 0) { // the packed blocks: as many bytes as their sizes add up to
		from = ctx->scratch("sortedbam.packed").ptr;
		HIP_CHECK(hipMemcpyAsync(&fetched, ctx->scratch("sortedbam.window_offset").as<uint64_t>() + blocks, 8, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		if (fetched > window) { set_last_error("agpu_sorted_bam_next: the compressed blocks of a window are larger than its stored blocks"); return AGPU_ERR_DEVICE; }
	}
	{ KernelTimer timer(ctx, "sorted_bam copy back", fetched);
	  HIP_CHECK(hipMemcpyAsync(pinned, from, fetched, hipMemcpyDeviceToHost, s)); }
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	ctx->sorted_bam_compressed_bytes += fetched;
	ctx->sorted_bam_next_block = first + blocks;
	if (ctx->sorted_bam_next_block < ctx->sorted_bam_blocks) TRY(launch_gather(ctx, ctx->sorted_bam_next_block)); // (gathered while the caller writes this window)
	*bytes = fetched;
	collect_kernel_samples(ctx);
	return AGPU_OK;
}

int agpu_sorted_bam_index(agpu_ctx* ctx, uint64_t first_block_file_offset, const uint32_t* ref_length, uint32_t n_ref, agpu_sorted_bam_index_arrays* index) {
	if (!ctx || !index || (!ref_length && n_ref > 0)) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	if (!ctx->sorted_bam_active) { set_last_error("agpu_sorted_bam_begin must run first"); return AGPU_ERR_INVALID; }
	if (n_ref >= 0x7FFFFFFFu) { set_last_error("agpu_sorted_bam_index: too many references"); return AGPU_ERR_INVALID; }
	if (ctx->sorted_bam_level != 0 && ctx->sorted_bam_next_block < ctx->sorted_bam_blocks) {
		set_last_error("agpu_sorted_bam_index: with compression on the virtual offsets need the sizes of all blocks: call it behind the agpu_sorted_bam_next that fetched the last window"); return AGPU_ERR_INVALID;
	}
	for (uint32_t t = 0; t < n_ref; ++t) if (ref_length[t] > (uint32_t) SBAM_MAX_REFERENCE) { set_last_error("a reference is longer than 2^29 bases: a BAI index cannot address it"); return AGPU_ERR_INVALID; }
	HIP_CHECK(hipSetDevice(ctx->device));
	hipStream_t s = ctx->stream;
	if (!ctx->sorted_bam_index_ready || ctx->sorted_bam_index_first != first_block_file_offset || ctx->sorted_bam_n_ref != n_ref) TRY(build_index(ctx, first_block_file_offset, ref_length, n_ref));
	index->n_ref = n_ref; index->n_chunks = ctx->sorted_bam_chunks; index->n_intervals = ctx->sorted_bam_intervals; index->n_no_coor = ctx->sorted_bam_no_coor;
	if (!index->chunk_key && !index->chunk_begin && !index->chunk_end && !index->interval_offset && !index->intervals && !index->ref_begin && !index->ref_end && !index->ref_mapped && !index->ref_unmapped) return AGPU_OK; // the sizes
	if (!index->chunk_key || !index->chunk_begin || !index->chunk_end || !index->interval_offset || !index->intervals || !index->ref_begin || !index->ref_end || !index->ref_mapped || !index->ref_unmapped) {
		set_last_error("agpu_sorted_bam_index: all arrays or none"); return AGPU_ERR_INVALID;
	}
	const uint64_t n_chunks = ctx->sorted_bam_chunks;
	if (n_chunks > 0) {
		HIP_CHECK(hipMemcpyAsync(index->chunk_key, ctx->scratch("sortedbam.chunk_key_sorted").ptr, n_chunks * 8, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipMemcpyAsync(index->chunk_begin, ctx->scratch("sortedbam.chunk_out").ptr, n_chunks * 8, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipMemcpyAsync(index->chunk_end, ctx->scratch("sortedbam.chunk_out").as<uint64_t>() + n_chunks, n_chunks * 8, hipMemcpyDeviceToHost, s));
	}
	HIP_CHECK(hipMemcpyAsync(index->interval_offset, ctx->scratch("sortedbam.interval_offset").ptr, ((size_t) n_ref + 1) * 8, hipMemcpyDeviceToHost, s));
	if (ctx->sorted_bam_intervals > 0) HIP_CHECK(hipMemcpyAsync(index->intervals, ctx->scratch("sortedbam.intervals").ptr, ctx->sorted_bam_intervals * 8, hipMemcpyDeviceToHost, s));
	std::vector<RefStats> stats((size_t) n_ref + 1);
	HIP_CHECK(hipMemcpyAsync(stats.data(), ctx->scratch("sortedbam.ref_stats").ptr, stats.size() * sizeof(RefStats), hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	for (uint32_t t = 0; t < n_ref; ++t) { index->ref_begin[t] = stats[t + 1].begin; index->ref_end[t] = stats[t + 1].end; index->ref_mapped[t] = stats[t + 1].mapped; index->ref_unmapped[t] = stats[t + 1].unmapped; }
	return AGPU_OK;
}

int agpu_sorted_bam_end(agpu_ctx* ctx) {
	if (!ctx) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	if (!ctx->sorted_bam_active) return AGPU_OK;
	(void) hipSetDevice(ctx->device);
	const hipError_t status = hipStreamSynchronize(ctx->stream); // (a window gathered ahead that nobody asked for)
	ctx->sorted_bam_active = false; ctx->sorted_bam_index_ready = false; ctx->sorted_bam_gathered_block = ~0ull; ctx->sorted_bam_level = 0;
	ctx->markdup.on = false; ctx->markdup.release_all(); // (behind the synchronisation: no gather reads "markdup.flag" any more)
	collect_kernel_samples(ctx);
	if (status != hipSuccess) { set_last_error(std::string("agpu_sorted_bam_end: ") + hipGetErrorString(status)); return AGPU_ERR_DEVICE; }
	return AGPU_OK;
}

}
