// arriba_amd/csrc/device/agpu_sam.hip -- SAM text -> BAM records on the MI355X, in front of the ingest of agpu_ingest.hip (the reference opens -x with sam_open, which
// reads SAM text as well as BAM: source/read_chimeric_alignments.cpp:563).  The per-line logic is sam_core.hpp; here are the three passes over a piece of text in HBM:
//   sam_newline_count_kernel / sam_line_start_kernel   16 bytes per lane compared against "\n", popcount per lane, sum and prefix over the wavefront; a rocPRIM scan over the
//                                                     wavefronts' sums gives every line its index, the second kernel writes the line starts
//   sam_size_kernel     one lane per line: validation and the size of the record (0: malformed -- the smallest line number and its reason are kept on the device);
//                       a rocPRIM exclusive scan over the sizes gives the offsets of the records
//   sam_emit_kernel     one lane per line again: the record is written
// Both per-line kernels follow record_parse_kernel (agpu_ingest.hip): one wavefront per workgroup stages the text of its 64 lines into LDS, 16 bytes per lane and turn, and
// the lanes parse there; the records are staged in LDS, too, and leave in whole words, lane after lane.  What does not fit a window (reads of some kilobases) is read from
// and written to HBM directly.  Integer and byte work, bound by the latency of dependent LDS loads; no MFMA.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>
#include <rocprim/rocprim.hpp>
#include "agpu_context.hpp"
#include "sam_core.hpp"

using namespace agpu;

namespace {

const int BLOCK = 256;
const uint32_t SAM_TEXT_WINDOW = 32768;   // 64 lines of 2 x 150 bases with their qualities and tags
const uint32_t SAM_RECORD_WINDOW = 24576; // their records (the bases take a quarter of their text)
const uint64_t SAM_NO_BAD_LINE = ~0ull;
const uint32_t SAM_GRID_LIMIT = 1u << 20; // workgroups of one wavefront per launch; a wavefront goes on with the lines one grid further
enum { SAM_STATE_BAD = 0 /* (line number << 8 | reason) of the first malformed line, SAM_NO_BAD_LINE if none */, SAM_STATE_RECORDS = 1, SAM_STATE_WORDS = 2 };

#define HIP_CHECK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { set_last_error(std::string(#call) + ": " + hipGetErrorString(e_)); return AGPU_ERR_DEVICE; } } while (0)
#define ALLOC(buffer, bytes) do { if (!(buffer).allocate(bytes)) { set_last_error("hipMalloc failed (" #buffer ")"); return AGPU_ERR_NO_MEMORY; } } while (0)
#define TRY(call) do { int s_ = (call); if (s_ != AGPU_OK) return s_; } while (0)

// bit k: byte at + k of the text is "\n" (the text is padded behind its end: the 16 bytes are there, those behind `size` do not count)
__device__ __forceinline__ uint32_t newline_mask(const uint8_t* text, uint32_t at, uint32_t size) {
	if (at >= size) return 0;
	const uint4 v = *(const uint4*) (text + at);
	const uint32_t words[4] = { v.x, v.y, v.z, v.w };
	uint32_t mask = 0;
	AGPU_UNROLL
	for (int k = 0; k < 4; ++k) {
		const uint32_t x = words[k] ^ 0x0A0A0A0Au;
		const uint32_t zero = ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu); // 0x80 in every byte of x that is zero
		mask |= (((zero >> 7) & 1) | ((zero >> 14) & 2) | ((zero >> 21) & 4) | ((zero >> 28) & 8)) << (4 * k);
	}
	if (size - at < 16) mask &= (1u << (size - at)) - 1;
	return mask;
}

__global__ void __launch_bounds__(BLOCK) sam_newline_count_kernel(const uint8_t* text, uint32_t size, uint32_t* wave_count) {
	const uint32_t chunk = blockIdx.x * BLOCK + threadIdx.x;
	uint32_t count = __popc(newline_mask(text, chunk * 16, size));
	for (int step = 32; step > 0; step >>= 1) count += __shfl_xor(count, step, 64);
	if (threadIdx.x % 64 == 0) wave_count[chunk / 64] = count;
}

// line_start[i]: where line i begins; line_start[n_lines] = size.  A "\n" that is the last byte of the text starts no line.
__global__ void __launch_bounds__(BLOCK) sam_line_start_kernel(const uint8_t* text, uint32_t size, const uint32_t* wave_base, uint32_t* line_start, uint32_t n_lines) {
	const uint32_t chunk = blockIdx.x * BLOCK + threadIdx.x, lane = threadIdx.x % 64;
	uint32_t mask = newline_mask(text, chunk * 16, size);
	const uint32_t count = __popc(mask);
	uint32_t before = count;
	for (int step = 1; step < 64; step <<= 1) { const uint32_t other = __shfl_up(before, step, 64); if (lane >= step) before += other; }
	uint32_t index = 1 + wave_base[chunk / 64] + before - count;
	while (mask != 0) {
		const uint32_t position = chunk * 16 + (uint32_t) __ffs(mask) - 1;
		mask &= mask - 1;
		if (position + 1 < size && index < n_lines) line_start[index] = position + 1;
		++index;
	}
	if (chunk == 0) { line_start[0] = 0; line_start[n_lines] = size; }
}

// what a lane of the per-line kernels works on: its line without the line feed and without one carriage return in front of it
struct SamLane { uint32_t begin, end; };
__device__ __forceinline__ SamLane lane_line(const uint8_t* text, const uint32_t* line_start, uint32_t line) {
	SamLane l = { line_start[line], line_start[line + 1] };
	if (l.end > l.begin && text[l.end - 1] == '\n') --l.end;
	if (l.end > l.begin && text[l.end - 1] == '\r') --l.end;
	return l;
}
// the text of the 64 lines from `first` on -> the window of the wavefront; returns the end of what was staged (lines that end behind it are parsed from HBM)
__device__ __forceinline__ uint32_t stage_text(const uint8_t* text, const uint32_t* line_start, uint32_t first, uint32_t n_lines, uint8_t* window, uint32_t lane, uint32_t& staged_begin) {
	const uint32_t span_end = line_start[first + 64 < n_lines ? first + 64 : n_lines];
	staged_begin = line_start[first] & ~15u;
	const uint32_t staged_end = span_end - staged_begin <= SAM_TEXT_WINDOW ? span_end : staged_begin + SAM_TEXT_WINDOW;
	for (uint32_t at = staged_begin + 16 * lane; at < staged_end; at += 16 * 64) *(uint4*) (window + (at - staged_begin)) = *(const uint4*) (text + at); // (the text is padded behind its end)
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
	return staged_end;
}

__global__ void __launch_bounds__(64) sam_size_kernel(const uint8_t* text, const uint32_t* line_start, uint32_t n_lines, SamTargets targets, uint64_t first_line_number, uint32_t* record_size, unsigned long long* state) {
	__shared__ __attribute__((aligned(16))) uint8_t window[SAM_TEXT_WINDOW + 64];
	const uint32_t lane = threadIdx.x;
	for (uint64_t first64 = (uint64_t) blockIdx.x * 64; first64 < n_lines; first64 += (uint64_t) gridDim.x * 64) { // (the same for the lanes of the wavefront; the grid is bounded)
		const uint32_t first = (uint32_t) first64, line = first + lane;
		uint32_t staged_begin;
		const uint32_t staged_end = stage_text(text, line_start, first, n_lines, window, lane, staged_begin);
		uint32_t bytes = 0;
		if (line < n_lines) {
			const SamLane l = lane_line(text, line_start, line);
			const uint8_t* p = line_start[line + 1] <= staged_end ? window + (l.begin - staged_begin) : text + l.begin;
			uint32_t reason;
			bytes = sam_line<false>(p, l.end - l.begin, targets, nullptr, reason);
			record_size[line] = bytes;
			if (bytes == 0) atomicMin(&state[SAM_STATE_BAD], (unsigned long long) ((first_line_number + line) << 8 | reason));
		}
		const unsigned long long good = __ballot(bytes != 0);
		if (lane == 0 && good != 0) atomicAdd(&state[SAM_STATE_RECORDS], (unsigned long long) __popcll(good));
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); // (the window is overwritten by the next turn)
	}
}

// out + record_offset[line]: where the record of the line goes (record_offset: the exclusive scan of record_size, one entry more than there are lines)
__global__ void __launch_bounds__(64) sam_emit_kernel(const uint8_t* text, const uint32_t* line_start, uint32_t n_lines, SamTargets targets, const uint32_t* record_size, const uint64_t* record_offset, uint8_t* out, uint64_t out_base) {
	__shared__ __attribute__((aligned(16))) uint8_t window[SAM_TEXT_WINDOW + 64];
	__shared__ __attribute__((aligned(16))) uint8_t records[SAM_RECORD_WINDOW + 8];
	const uint32_t lane = threadIdx.x;
	for (uint64_t first64 = (uint64_t) blockIdx.x * 64; first64 < n_lines; first64 += (uint64_t) gridDim.x * 64) { // (the same for the lanes of the wavefront; the grid is bounded)
	const uint32_t first = (uint32_t) first64, line = first + lane;
	uint32_t staged_begin;
	const uint32_t staged_end = stage_text(text, line_start, first, n_lines, window, lane, staged_begin);
	// the records of the wavefront lie back to back from records_begin on; those that end inside the window are staged (word-aligned like their place in the stream)
	const uint64_t records_begin = out_base + record_offset[first], aligned_begin = records_begin & ~3ull;
	uint64_t fit_end = records_begin;
	if (line < n_lines) {
		const uint32_t bytes = record_size[line];
		if (bytes != 0) {
			const SamLane l = lane_line(text, line_start, line);
			const uint8_t* p = line_start[line + 1] <= staged_end ? window + (l.begin - staged_begin) : text + l.begin;
			const uint64_t at = out_base + record_offset[line];
			const bool fits = at + bytes - aligned_begin <= SAM_RECORD_WINDOW;
			uint32_t reason;
			sam_line<true>(p, l.end - l.begin, targets, fits ? records + (at - aligned_begin) : out + at, reason);
			if (fits) fit_end = at + bytes;
		}
	}
	for (int step = 32; step > 0; step >>= 1) { const uint64_t other = __shfl_xor(fit_end, step, 64); fit_end = other > fit_end ? other : fit_end; } // (the records that fit are the first ones: this is where they end)
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
	for (uint64_t word = aligned_begin + 4 * lane; word < fit_end; word += 4 * 64) {
		if (word >= records_begin && word + 4 <= fit_end) *(uint32_t*) (out + word) = *(const uint32_t*) (records + (word - aligned_begin));
		else for (uint32_t k = 0; k < 4; ++k) if (word + k >= records_begin && word + k < fit_end) out[word + k] = records[word + k - aligned_begin]; // (the first and the last word are shared with the neighbours)
	}
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); __builtin_amdgcn_wave_barrier(); // (both windows are overwritten by the next turn)
	}
}

__global__ void sam_state_reset_kernel(unsigned long long* state) { state[SAM_STATE_BAD] = SAM_NO_BAD_LINE; state[SAM_STATE_RECORDS] = 0; }

struct SamPiece { uint32_t size = 0, n_lines = 0; uint64_t record_bytes = 0; };

SamTargets device_targets(agpu_ctx* ctx) {
	SamTargets t = { ctx->scratch("sam.names").as<char>(), ctx->scratch("sam.name_offset").as<uint32_t>(), ctx->scratch("sam.table").as<uint32_t>(), ctx->sam_table_mask, ctx->sam_n_targets };
	return t;
}

int upload_targets(agpu_ctx* ctx, const char* names, const uint32_t* name_offset, uint32_t n_targets, hipStream_t s) {
	std::vector<uint32_t> table(sam_table_slots(n_targets));
	sam_build_table(names, name_offset, n_targets, table.data());
	const size_t names_bytes = name_offset[n_targets];
	ALLOC(ctx->scratch("sam.names"), names_bytes + 16); ALLOC(ctx->scratch("sam.name_offset"), ((size_t) n_targets + 1) * 4); ALLOC(ctx->scratch("sam.table"), table.size() * 4); ALLOC(ctx->scratch("sam.state"), SAM_STATE_WORDS * 8);
	if (names_bytes > 0) HIP_CHECK(hipMemcpyAsync(ctx->scratch("sam.names").ptr, names, names_bytes, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(ctx->scratch("sam.name_offset").ptr, name_offset, ((size_t) n_targets + 1) * 4, hipMemcpyHostToDevice, s));
	HIP_CHECK(hipMemcpyAsync(ctx->scratch("sam.table").ptr, table.data(), table.size() * 4, hipMemcpyHostToDevice, s));
	sam_state_reset_kernel<<<1, 1, 0, s>>>(ctx->scratch("sam.state").as<unsigned long long>());
	HIP_CHECK(hipStreamSynchronize(s)); // (`table` leaves with this function)
	ctx->sam_n_targets = n_targets; ctx->sam_table_mask = (uint32_t) table.size() - 1;
	return AGPU_OK;
}

// passes 1 and 2 over text[0 .. size) in HBM (padded by 64 bytes; whole lines): the line starts, the size of every record and their offsets.  Two read-backs (how many
// lines there are, how many bytes their records take) -- the caller needs the second to make room for the records before sam_emit writes them.
int sam_measure(agpu_ctx* ctx, hipStream_t s, const uint8_t* text, uint32_t size, bool ends_with_line_feed, uint64_t first_line_number, SamPiece& piece) {
	piece.size = size; piece.n_lines = 0; piece.record_bytes = 0;
	if (size == 0) return AGPU_OK;
	const uint32_t n_chunks = (size + 15) / 16, n_waves = (n_chunks + 63) / 64, grid = (n_chunks + BLOCK - 1) / BLOCK;
	DeviceBuffer& wave_count = ctx->scratch("sam.wave_count"); DeviceBuffer& wave_base = ctx->scratch("sam.wave_base"); DeviceBuffer& rocprim_scratch = ctx->scratch("sam.rocprim");
	const size_t waves_padded = (size_t) grid * (BLOCK / 64) + 1; // (every wavefront of the grid writes its sum; one more entry: the total)
	ALLOC(wave_count, waves_padded * 4); ALLOC(wave_base, waves_padded * 4);
	HIP_CHECK(hipMemsetAsync(wave_count.as<uint32_t>() + waves_padded - 1, 0, 4, s));
	{ KernelTimer timer(ctx, "sam_newline_count_kernel", size, s);
	  sam_newline_count_kernel<<<grid, BLOCK, 0, s>>>(text, size, wave_count.as<uint32_t>()); }
	size_t temporary = 0;
	HIP_CHECK(rocprim::exclusive_scan(nullptr, temporary, wave_count.as<uint32_t>(), wave_base.as<uint32_t>(), 0u, waves_padded, rocprim::plus<uint32_t>(), s));
	if (temporary > rocprim_scratch.capacity) ALLOC(rocprim_scratch, temporary);
	HIP_CHECK(rocprim::exclusive_scan(rocprim_scratch.ptr, temporary, wave_count.as<uint32_t>(), wave_base.as<uint32_t>(), 0u, waves_padded, rocprim::plus<uint32_t>(), s));
	uint32_t line_feeds = 0;
	HIP_CHECK(hipMemcpyAsync(&line_feeds, wave_base.as<uint32_t>() + waves_padded - 1, 4, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	(void) n_waves;
	const uint32_t n_lines = line_feeds + (ends_with_line_feed ? 0 : 1);
	piece.n_lines = n_lines;
	DeviceBuffer& line_start = ctx->scratch("sam.line_start"); DeviceBuffer& record_size = ctx->scratch("sam.record_size"); DeviceBuffer& record_offset = ctx->scratch("sam.record_offset");
	ALLOC(line_start, ((size_t) n_lines + 1) * 4); ALLOC(record_size, ((size_t) n_lines + 1) * 4); ALLOC(record_offset, ((size_t) n_lines + 1) * 8);
	{ KernelTimer timer(ctx, "sam_line_start_kernel", (uint64_t) size + (uint64_t) n_lines * 4, s);
	  sam_line_start_kernel<<<grid, BLOCK, 0, s>>>(text, size, wave_base.as<uint32_t>(), line_start.as<uint32_t>(), n_lines); }
	HIP_CHECK(hipMemsetAsync(record_size.as<uint32_t>() + n_lines, 0, 4, s));
	{ KernelTimer timer(ctx, "sam_size_kernel", (uint64_t) size + (uint64_t) n_lines * 8, s);
	  sam_size_kernel<<<std::min<uint32_t>((n_lines + 63) / 64, SAM_GRID_LIMIT), 64, 0, s>>>(text, line_start.as<uint32_t>(), n_lines, device_targets(ctx), first_line_number, record_size.as<uint32_t>(), ctx->scratch("sam.state").as<unsigned long long>()); }
	HIP_CHECK(rocprim::exclusive_scan(nullptr, temporary, record_size.as<uint32_t>(), record_offset.as<uint64_t>(), (uint64_t) 0, (size_t) n_lines + 1, rocprim::plus<uint64_t>(), s));
	if (temporary > rocprim_scratch.capacity) ALLOC(rocprim_scratch, temporary);
	HIP_CHECK(rocprim::exclusive_scan(rocprim_scratch.ptr, temporary, record_size.as<uint32_t>(), record_offset.as<uint64_t>(), (uint64_t) 0, (size_t) n_lines + 1, rocprim::plus<uint64_t>(), s));
	HIP_CHECK(hipMemcpyAsync(&piece.record_bytes, record_offset.as<uint64_t>() + n_lines, 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	return AGPU_OK;
}

// pass 3: the records of the piece sam_measure looked at, to out[out_base .. out_base + piece.record_bytes); nothing is waited for
int sam_emit(agpu_ctx* ctx, hipStream_t s, const uint8_t* text, const SamPiece& piece, uint8_t* out, uint64_t out_base) {
	if (piece.n_lines == 0) return AGPU_OK;
	KernelTimer timer(ctx, "sam_emit_kernel", (uint64_t) piece.size + piece.record_bytes, s);
	sam_emit_kernel<<<std::min<uint32_t>((piece.n_lines + 63) / 64, SAM_GRID_LIMIT), 64, 0, s>>>(text, ctx->scratch("sam.line_start").as<uint32_t>(), piece.n_lines, device_targets(ctx), ctx->scratch("sam.record_size").as<uint32_t>(),
		ctx->scratch("sam.record_offset").as<uint64_t>(), out, out_base);
	return AGPU_OK;
}

int read_state(agpu_ctx* ctx, hipStream_t s, uint64_t& bad_line, uint32_t& reason, uint64_t& records) {
	unsigned long long state[SAM_STATE_WORDS];
	HIP_CHECK(hipMemcpyAsync(state, ctx->scratch("sam.state").ptr, sizeof(state), hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	bad_line = state[SAM_STATE_BAD] == SAM_NO_BAD_LINE ? 0 : state[SAM_STATE_BAD] >> 8; reason = (uint32_t) (state[SAM_STATE_BAD] & 0xFF); records = state[SAM_STATE_RECORDS];
	return AGPU_OK;
}

const uint64_t SAM_PIECE_LIMIT = 0xFFFF0000ull; // (offsets inside a piece of text are 32 bits wide)

}

// agpu_ingest_finish asks: the first malformed line of the SAM text of this ingest, if any (the message of the reference's class: "failed to load alignments")
int agpu::sam_ingest_verdict(agpu_ctx* ctx) {
	if (!ctx->ingest_sam) return AGPU_OK;
	uint64_t bad_line = 0, records = 0; uint32_t reason = 0;
	TRY(read_state(ctx, ctx->stream, bad_line, reason, records));
	if (bad_line != 0) { set_last_error("failed to load alignments: SAM line " + std::to_string(bad_line) + ": " + sam_reason_text(reason)); return AGPU_ERR_INVALID; }
	return AGPU_OK;
}

extern "C" {

int agpu_ingest_sam_targets(agpu_ctx* ctx, const char* names, const uint32_t* name_offset, uint32_t n_targets) {
	if (!ctx || !ctx->ingest_active) { set_last_error("agpu_ingest_begin must run first"); return AGPU_ERR_INVALID; }
	if (!name_offset || (!names && name_offset[n_targets] > 0)) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	if (ctx->ingest_first_record != 0) { set_last_error("SAM text: the stream holds records only (agpu_ingest_config.first_record_offset must be 0)"); return AGPU_ERR_INVALID; }
	HIP_CHECK(hipSetDevice(ctx->device));
	TRY(upload_targets(ctx, names ? names : "", name_offset, n_targets, ctx->stream));
	ctx->ingest_sam = true;
	return AGPU_OK;
}

int agpu_ingest_push_sam(agpu_ctx* ctx, const void* text, size_t size, uint64_t first_line_number) {
	if (!ctx || !ctx->ingest_active) { set_last_error("agpu_ingest_begin must run first"); return AGPU_ERR_INVALID; }
	if (!ctx->ingest_sam) { set_last_error("agpu_ingest_sam_targets must run first"); return AGPU_ERR_INVALID; }
	if (size > SAM_PIECE_LIMIT) { set_last_error("a piece of SAM text must be smaller than 4 GiB"); return AGPU_ERR_INVALID; }
	HIP_CHECK(hipSetDevice(ctx->device));
	hipStream_t s = ctx->stream, pieces = ctx->piece_stream;
	const unsigned int slot = ctx->ingest_pushes % AGPU_PIECE_SLOTS;
	if (size > 0) {
		ALLOC(ctx->ingest_raw[slot], size + 64); // (+ 64: the kernels load whole 16-byte words)
		HIP_CHECK(hipStreamWaitEvent(s, ctx->piece_done[slot], 0)); // (the piece that lay in this buffer has been transcoded; an event that was never recorded does not hold anybody up)
		HIP_CHECK(hipMemcpyAsync(ctx->ingest_raw[slot].ptr, text, size, hipMemcpyHostToDevice, s));
		HIP_CHECK(hipEventRecord(ctx->piece_copied[slot], s));
		HIP_CHECK(hipStreamWaitEvent(pieces, ctx->piece_copied[slot], 0));
		// One read-back per pass in front of the emit pass (the number of lines, then the bytes of their records): the records of successive pieces must lie back to back, and
		// the stream must have room for them before they are written, so the host learns the size of a piece's records before it enqueues the piece's last kernel.  The cost:
		// this thread waits for the copy and the first two passes of the piece (the emit pass and the windows of the ingest run behind its back); the thread that reads the
		// file fills the next buffer meanwhile.
		SamPiece piece;
		TRY(sam_measure(ctx, pieces, ctx->ingest_raw[slot].as<uint8_t>(), (uint32_t) size, ((const uint8_t*) text)[size - 1] == '\n', first_line_number, piece));
		TRY(agpu::ingest_grow_stream(ctx, ctx->ingest_stream_size + piece.record_bytes));
		TRY(sam_emit(ctx, pieces, ctx->ingest_raw[slot].as<uint8_t>(), piece, ctx->ingest_stream.as<uint8_t>(), ctx->ingest_stream_size));
		ctx->ingest_stream_size += piece.record_bytes;
		if (ctx->ingest_pushes > 0) HIP_CHECK(hipStreamWaitEvent(pieces, ctx->piece_ready[(ctx->ingest_pushes - 1) % AGPU_PIECE_SLOTS], 0)); // (ready in the order of the pieces)
		HIP_CHECK(hipEventRecord(ctx->piece_ready[slot], pieces));
		HIP_CHECK(hipEventRecord(ctx->piece_done[slot], pieces));
	} else { HIP_CHECK(hipEventRecord(ctx->piece_copied[slot], s)); HIP_CHECK(hipEventRecord(ctx->piece_ready[slot], s)); }
	return agpu::ingest_piece_pushed(ctx);
}

int agpu_sam_transcode(agpu_ctx* ctx, const void* text, size_t size, const char* names, const uint32_t* name_offset, uint32_t n_targets, void* out, size_t capacity, uint64_t* out_bytes, uint64_t* n_records, uint64_t* bad_line) {
	if (!ctx || (!text && size > 0) || !name_offset || !out_bytes || !n_records || !bad_line) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	if (ctx->ingest_active) { set_last_error("agpu_sam_transcode: an ingest is under way on this context"); return AGPU_ERR_INVALID; }
	*out_bytes = 0; *n_records = 0; *bad_line = 0;
	// the '@' lines in front of the first alignment are skipped (and counted) here
	const uint8_t* bytes = (const uint8_t*) text;
	size_t at = 0; uint64_t header_lines = 0;
	while (at < size && bytes[at] == '@') { const uint8_t* feed = (const uint8_t*) memchr(bytes + at, '\n', size - at); at = feed ? (size_t) (feed - bytes) + 1 : size; ++header_lines; }
	bytes += at; size -= at;
	if (size > SAM_PIECE_LIMIT) { set_last_error("a piece of SAM text must be smaller than 4 GiB"); return AGPU_ERR_INVALID; }
	HIP_CHECK(hipSetDevice(ctx->device));
	hipStream_t s = ctx->stream;
	TRY(upload_targets(ctx, names ? names : "", name_offset, n_targets, s));
	if (size == 0) return AGPU_OK;
	DeviceBuffer& device_text = ctx->scratch("sam.tool_text"); DeviceBuffer& device_out = ctx->scratch("sam.tool_records");
	ALLOC(device_text, size + 64);
	HIP_CHECK(hipMemcpyAsync(device_text.ptr, bytes, size, hipMemcpyHostToDevice, s));
	SamPiece piece;
	TRY(sam_measure(ctx, s, device_text.as<uint8_t>(), (uint32_t) size, bytes[size - 1] == '\n', header_lines + 1, piece));
	ALLOC(device_out, piece.record_bytes + 64);
	TRY(sam_emit(ctx, s, device_text.as<uint8_t>(), piece, device_out.as<uint8_t>(), 0));
	uint32_t reason = 0;
	TRY(read_state(ctx, s, *bad_line, reason, *n_records));
	*out_bytes = piece.record_bytes;
	if (piece.record_bytes > capacity) { set_last_error("the buffer is too small for the records"); return AGPU_ERR_INVALID; }
	if (piece.record_bytes > 0) HIP_CHECK(hipMemcpy(out, device_out.ptr, piece.record_bytes, hipMemcpyDeviceToHost));
	if (*bad_line != 0) { set_last_error("failed to load alignments: SAM line " + std::to_string(*bad_line) + ": " + sam_reason_text(reason)); return AGPU_ERR_INVALID; }
	return AGPU_OK;
}

}
