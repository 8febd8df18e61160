// arriba_amd/csrc/device/agpu_depth.hip -- --coverage on the MI355X: the per-base alignment depth of the record stream of the last ingest as bedGraph text (include/arriba_gpu.h:
// agpu_depth_begin / _next / _end).  What decides a byte is depth_core.hpp, which the host steps as well (arriba_amd/csrc/host/depth.cpp); here are
//   depth_mark_kernel   one lane per record through ingest.record_offset (the access pattern of sorted_bam_key_kernel and virus_scan_kernel): the head of the record, a walk over
//                       its CIGAR, +1 at the first and -1 behind the last position of every covered segment (32-bit atomicAdd) in a difference array of LN + 1 slots per contig,
//                       the contigs end to end.  The marks of a contig add up to zero, so ONE inclusive scan (rocPRIM) of the whole array gives the depth of every contig;
//                       integer sums commute: the array is the same under every schedule
//   depth_flag_kernel   one lane per slot of a window of positions: is it the first / the last slot of a run of equal depth > 0 (both counts in one 64-bit word, for one scan)
//   depth_emit_kernel   the first slots and the ends of the runs that END in the window, at the places the scan gives; a run that is open at the end of the window leaves its
//                       first slot in "depth.carry" and is finished by the window that holds its last slot: it comes out as one run
//   depth_line_kernel   one lane per run: (refID, start, end, depth) by binary search in the offsets of the contigs, the bytes of its line, the sums of the statistics
//   depth_text_kernel   one lane per run: the bytes of its line that fall into the staging window (a line may straddle two windows), plain byte stores
// Integer and byte work: the mark kernel is bound by the two dependent loads in front of a record's words and by its atomics, the rest by memory; no MFMA, no LDS.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <rocprim/rocprim.hpp>
#define AGPU_OPTION "--coverage"
#include "resident_stream.hpp"
#include "device_utils.hpp"
#include "depth_core.hpp"

using namespace agpu;

namespace {

const uint64_t DEFAULT_WINDOW = 1ull << 25;      // positions whose runs are found at a time
const uint64_t DEFAULT_TEXT_WINDOW = 16ull << 20; // bytes of a staging window

enum { COUNTER_RECORDS = 0, COUNTER_SEGMENTS = 1, COUNTER_COVERED = 2, COUNTER_ALIGNED = 3, COUNTER_MAX_DEPTH = 4, COUNTER_WORDS = 5 }; // 64-bit words

struct DifferenceMark {
	uint32_t* slots; // of the contig
	__device__ __forceinline__ void operator()(uint32_t begin, uint32_t end) const { atomicAdd(&slots[begin], 1u); atomicAdd(&slots[end], 0xFFFFFFFFu); } // (end <= LN: the contig has LN + 1 slots)
};

__global__ void __launch_bounds__(BLOCK) depth_mark_kernel(const uint8_t* __restrict__ stream, uint64_t stream_size, const uint64_t* __restrict__ record_offset, uint64_t n, const uint64_t* __restrict__ contig_offset,
		const uint32_t* __restrict__ ref_length, uint32_t n_ref, uint32_t* difference, unsigned long long* counters) {
	const uint64_t r = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	unsigned long long counted = 0, segments = 0;
	if (r < n) {
		const uint64_t at = record_offset[r];
		if (at < stream_size) {
			const DepthRecord record = depth_parse(stream, at, stream_size, n_ref);
			if (record.counts) {
				const DifferenceMark mark = { difference + contig_offset[record.ref] };
				segments = depth_cover(stream, record.cigar_at, record.n_cigar, record.pos, ref_length[record.ref], mark);
				counted = 1;
			}
		}
	}
	counted = wave_sum(counted); segments = wave_sum(segments);
	if ((threadIdx.x & 63) == 0) {
		if (counted != 0) atomicAdd(&counters[COUNTER_RECORDS], counted);
		if (segments != 0) atomicAdd(&counters[COUNTER_SEGMENTS], segments);
	}
}

// flags[i] of slot first + i, i < count: 1 if a run begins there, 1 << 32 if one ends there; one entry more (0) for the scan that gives both totals
__global__ void __launch_bounds__(BLOCK) depth_flag_kernel(const uint32_t* __restrict__ depth, uint64_t slots, uint64_t first, uint64_t count, uint64_t* flags) {
	const uint64_t i = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (i > count) return;
	uint64_t flag = 0;
	if (i < count) {
		const uint64_t g = first + i;
		const uint32_t here = depth[g], before = g > 0 ? depth[g - 1] : 0u, after = g + 1 < slots ? depth[g + 1] : 0u;
		flag = (depth_head(before, here) ? 1ull : 0ull) | (depth_tail(here, after) ? 1ull << 32 : 0ull);
	}
	flags[i] = flag;
}

// runs[k]: the k-th run that ends in the window, as (first slot, slot behind its last); carry_in: the first of them began in an earlier window (its first slot is copied from
// "depth.carry" in front of this kernel).  The one head that has no end in the window -- there is at most one, the last -- goes to *carry.
__global__ void __launch_bounds__(BLOCK) depth_emit_kernel(const uint64_t* __restrict__ flags, const uint64_t* __restrict__ place, uint64_t first, uint64_t count, uint32_t carry_in, uint64_t ends, ulonglong2* runs, uint64_t* carry) {
	const uint64_t i = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (i >= count) return;
	const uint64_t flag = flags[i];
	if (flag == 0) return;
	const uint64_t at = place[i];
	if (flag & 1ull) {
		const uint64_t k = (at & 0xFFFFFFFFull) + carry_in;
		if (k < ends) runs[k].x = first + i; else *carry = first + i;
	}
	if (flag >> 32) runs[at >> 32].y = first + i + 1;
}

// runs[k] becomes (refID, start, end, depth), in place (a lane reads its own 16 bytes, then writes them); lane `ends` writes the 0 that ends the line lengths
__global__ void __launch_bounds__(BLOCK) depth_line_kernel(void* runs, uint64_t ends, const uint32_t* __restrict__ depth, const uint64_t* __restrict__ contig_offset, uint32_t n_ref, const uint32_t* __restrict__ name_offset,
		uint32_t* line_bytes, unsigned long long* counters) {
	const uint64_t k = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	unsigned long long covered = 0, aligned = 0, deepest = 0;
	if (k < ends) {
		const ulonglong2 slots = ((const ulonglong2*) runs)[k];
		const uint32_t ref = depth_contig_of(contig_offset, n_ref, slots.x);
		const uint64_t base = contig_offset[ref];
		const uint32_t start = (uint32_t) (slots.x - base), end = (uint32_t) (slots.y - base), d = depth[slots.x];
		((uint4*) runs)[k] = make_uint4(ref, start, end, d);
		line_bytes[k] = depth_line_bytes(name_offset[ref + 1] - name_offset[ref], start, end, d);
		covered = end - start; aligned = covered * d; deepest = d;
	} else if (k == ends) line_bytes[k] = 0;
	covered = wave_sum(covered); aligned = wave_sum(aligned);
	for (int offset = 32; offset > 0; offset >>= 1) { const unsigned long long other = __shfl_down(deepest, offset); deepest = other > deepest ? other : deepest; }
	if ((threadIdx.x & 63) == 0 && covered != 0) { atomicAdd(&counters[COUNTER_COVERED], covered); atomicAdd(&counters[COUNTER_ALIGNED], aligned); atomicMax(&counters[COUNTER_MAX_DEPTH], deepest); }
}

// byte `at` of the file goes to staging[at - window_begin] if from <= at < upto (window_begin <= from, upto <= window_begin + the size of the staging window)
struct StagingPut {
	uint8_t* staging; uint64_t at, from, upto, window_begin;
	__device__ __forceinline__ void operator()(uint8_t byte) { if (at >= from && at < upto) staging[at - window_begin] = byte; ++at; }
};

__global__ void __launch_bounds__(BLOCK) depth_text_kernel(const uint4* __restrict__ runs, const uint64_t* __restrict__ line_offset, uint64_t ends, const char* __restrict__ names, const uint32_t* __restrict__ name_offset,
		uint64_t batch_begin, uint64_t from, uint64_t upto, uint64_t window_begin, uint8_t* staging) {
	const uint64_t k = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (k >= ends) return;
	const uint64_t begin = batch_begin + line_offset[k], end = batch_begin + line_offset[k + 1];
	if (end <= from || begin >= upto) return;
	const uint4 run = runs[k];
	StagingPut put = { staging, begin, from, upto, window_begin };
	depth_line(names + name_offset[run.x], name_offset[run.x + 1] - name_offset[run.x], run.y, run.z, run.w, put);
}

void note_peak(DepthState& state) { state.stats.peak_bytes = std::max<uint64_t>(state.stats.peak_bytes, state.allocated()); }

// behind a hipStreamSynchronize: the milliseconds between the two events of the state go to seconds[part]
void add_seconds(DepthState& state, int part) { float ms = 0; if (hipEventElapsedTime(&ms, state.events[0], state.events[1]) == hipSuccess) state.stats.seconds[part] += ms / 1000.0; }

// the marks and the scan: "depth.depth" holds the depth of every slot
int mark_and_scan(agpu_ctx* ctx, const ResidentStream& resident, const uint32_t* ref_length, const char* names, const uint32_t* name_offset, uint32_t n_ref) {
	hipStream_t s = ctx->stream;
	DepthState& state = ctx->depth;
	const uint64_t size = resident.stream_size, n = resident.records;
	std::vector<uint64_t> host_offset((size_t) n_ref + 1, 0);
	for (uint32_t t = 0; t < n_ref; ++t) host_offset[t + 1] = host_offset[t] + ref_length[t] + 1;
	const uint64_t slots = host_offset[n_ref], name_bytes = n_ref > 0 ? name_offset[n_ref] : 0;
	state.n_ref = n_ref; state.slots = slots;
	state.window = knob_of("ARRIBA_DEPTH_WINDOW", DEFAULT_WINDOW, 1ull << 31); state.text_window = knob_of("ARRIBA_DEPTH_TEXT_WINDOW", DEFAULT_TEXT_WINDOW, 1ull << 31);
	state.next_slot = 0; state.carry = false; state.batch_begin = state.batch_end = state.batch_runs = 0; state.written = state.flushed = 0;
	memset(&state.stats, 0, sizeof(state.stats));
	DeviceBuffer& contig_offset = state.buffer("depth.contig_offset"); DeviceBuffer& lengths = state.buffer("depth.ref_length"); DeviceBuffer& name_text = state.buffer("depth.names"); DeviceBuffer& name_at = state.buffer("depth.name_offset");
	DeviceBuffer& depth = state.buffer("depth.depth"); DeviceBuffer& counters = state.buffer("depth.counters"); DeviceBuffer& carry = state.buffer("depth.carry");
	DeviceBuffer& flags = state.buffer("depth.flags"); DeviceBuffer& place = state.buffer("depth.place"); DeviceBuffer& staging = state.buffer("depth.staging");
	const uint64_t held = std::max<uint64_t>(std::min(state.window, slots), 1);
	ALLOC(contig_offset, ((size_t) n_ref + 1) * 8); ALLOC(lengths, std::max<size_t>(n_ref, 1) * 4); ALLOC(name_text, std::max<uint64_t>(name_bytes, 1)); ALLOC(name_at, ((size_t) n_ref + 1) * 4);
	ALLOC(depth, std::max<uint64_t>(slots, 1) * 4); ALLOC(counters, COUNTER_WORDS * 8); ALLOC(carry, 8); ALLOC(flags, (held + 1) * 8); ALLOC(place, (held + 1) * 8); ALLOC(staging, state.text_window);
	note_peak(state);
	HIP_CHECK(hipMemcpyAsync(contig_offset.ptr, host_offset.data(), host_offset.size() * 8, hipMemcpyHostToDevice, s));
	if (n_ref > 0) {
		HIP_CHECK(hipMemcpyAsync(lengths.ptr, ref_length, (size_t) n_ref * 4, hipMemcpyHostToDevice, s));
		HIP_CHECK(hipMemcpyAsync(name_at.ptr, name_offset, ((size_t) n_ref + 1) * 4, hipMemcpyHostToDevice, s));
		if (name_bytes > 0) HIP_CHECK(hipMemcpyAsync(name_text.ptr, names, name_bytes, hipMemcpyHostToDevice, s));
	}
	HIP_CHECK(hipStreamSynchronize(s)); // (the sources are pageable memory of the caller)
	HIP_CHECK(hipMemsetAsync(counters.ptr, 0, COUNTER_WORDS * 8, s));
	HIP_CHECK(hipEventRecord(state.events[0], s));
	HIP_CHECK(hipMemsetAsync(depth.ptr, 0, std::max<uint64_t>(slots, 1) * 4, s));
	if (n > 0 && slots > 0) { KernelTimer timer(ctx, "depth_mark_kernel", n * 8 + n * 64);
	  depth_mark_kernel<<<grid_for(n), BLOCK, 0, s>>>(resident.stream, size, resident.record_offset, n, contig_offset.as<uint64_t>(), lengths.as<uint32_t>(), n_ref, depth.as<uint32_t>(),
	    counters.as<unsigned long long>()); }
	HIP_CHECK(hipEventRecord(state.events[1], s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	add_seconds(state, 0);
	HIP_CHECK(hipEventRecord(state.events[0], s));
	if (slots > 0) TRY(with_temporary(ctx, state.buffer("depth.rocprim"), "depth rocprim::inclusive_scan(marks)", slots * 8, [&](void* t, size_t& b) { return rocprim::inclusive_scan(t, b, depth.as<uint32_t>(), depth.as<uint32_t>(), (size_t) slots, rocprim::plus<uint32_t>(), s); }));
	note_peak(state);
	HIP_CHECK(hipEventRecord(state.events[1], s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	add_seconds(state, 1);
	return AGPU_OK;
}

// the runs that end in the next window of positions, and where their lines lie in the file
int find_runs(agpu_ctx* ctx) {
	hipStream_t s = ctx->stream;
	DepthState& state = ctx->depth;
	const uint64_t first = state.next_slot, count = std::min(state.window, state.slots - first);
	DeviceBuffer& depth = state.buffer("depth.depth"); DeviceBuffer& flags = state.buffer("depth.flags"); DeviceBuffer& place = state.buffer("depth.place"); DeviceBuffer& carry = state.buffer("depth.carry");
	DeviceBuffer& runs = state.buffer("depth.runs"); DeviceBuffer& line_bytes = state.buffer("depth.line_bytes"); DeviceBuffer& line_offset = state.buffer("depth.line_offset"); DeviceBuffer& counters = state.buffer("depth.counters");
	HIP_CHECK(hipEventRecord(state.events[0], s));
	{ KernelTimer timer(ctx, "depth_flag_kernel", count * 12);
	  depth_flag_kernel<<<grid_for(count + 1), BLOCK, 0, s>>>(depth.as<uint32_t>(), state.slots, first, count, flags.as<uint64_t>()); }
	TRY(with_temporary(ctx, state.buffer("depth.rocprim"), "depth rocprim::exclusive_scan(flags)", count * 16, [&](void* t, size_t& b) { return rocprim::exclusive_scan(t, b, flags.as<uint64_t>(), place.as<uint64_t>(), (uint64_t) 0, (size_t) count + 1, rocprim::plus<uint64_t>(), s); }));
	uint64_t totals = 0;
	HIP_CHECK(hipMemcpyAsync(&totals, place.as<uint64_t>() + count, 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	const uint64_t heads = totals & 0xFFFFFFFFull, ends = totals >> 32, carry_in = state.carry ? 1 : 0;
	if (heads + carry_in != ends && heads + carry_in != ends + 1) { set_last_error("agpu_depth_next: the first and the last slots of the runs do not pair up"); return AGPU_ERR_DEVICE; }
	uint64_t text = 0;
	if (heads > 0 || ends > 0) {
		if (runs.capacity < std::max<uint64_t>(ends, 1) * 16) ALLOC(runs, std::max<uint64_t>(ends, 1) * 16);
		if (line_bytes.capacity < (ends + 1) * 4) ALLOC(line_bytes, (ends + 1) * 4);
		if (line_offset.capacity < (ends + 1) * 8) ALLOC(line_offset, (ends + 1) * 8);
		note_peak(state);
		if (carry_in && ends > 0) HIP_CHECK(hipMemcpyAsync(runs.ptr, carry.ptr, 8, hipMemcpyDeviceToDevice, s)); // (runs[0].x: stream order puts it in front of the kernel that may write the next carry)
		{ KernelTimer timer(ctx, "depth_emit_kernel", count * 16 + ends * 16);
		  depth_emit_kernel<<<grid_for(count), BLOCK, 0, s>>>(flags.as<uint64_t>(), place.as<uint64_t>(), first, count, (uint32_t) carry_in, ends, runs.as<ulonglong2>(), carry.as<uint64_t>()); }
	}
	if (ends > 0) {
		{ KernelTimer timer(ctx, "depth_line_kernel", ends * 40);
		  depth_line_kernel<<<grid_for(ends + 1), BLOCK, 0, s>>>(runs.ptr, ends, depth.as<uint32_t>(), state.buffer("depth.contig_offset").as<uint64_t>(), state.n_ref, state.buffer("depth.name_offset").as<uint32_t>(), line_bytes.as<uint32_t>(),
		    counters.as<unsigned long long>()); }
		TRY(with_temporary(ctx, state.buffer("depth.rocprim"), "depth rocprim::exclusive_scan(line bytes)", ends * 12, [&](void* t, size_t& b) { return rocprim::exclusive_scan(t, b, line_bytes.as<uint32_t>(), line_offset.as<uint64_t>(), (uint64_t) 0, (size_t) ends + 1, rocprim::plus<uint64_t>(), s); }));
		HIP_CHECK(hipMemcpyAsync(&text, line_offset.as<uint64_t>() + ends, 8, hipMemcpyDeviceToHost, s));
	}
	HIP_CHECK(hipEventRecord(state.events[1], s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	add_seconds(state, 2);
	state.carry = heads + carry_in == ends + 1;
	state.next_slot = first + count;
	state.batch_begin = state.batch_end; state.batch_end += text; state.batch_runs = ends;
	state.stats.runs += ends; state.stats.text_bytes += text; ++state.stats.position_windows;
	return AGPU_OK;
}

// bytes [flushed, written) of the file, which lie in the staging window, into the caller's buffer
int fetch(agpu_ctx* ctx, void* pinned, uint64_t* bytes) {
	hipStream_t s = ctx->stream;
	DepthState& state = ctx->depth;
	const uint64_t fetched = state.written - state.flushed;
	HIP_CHECK(hipEventRecord(state.events[0], s));
	{ KernelTimer timer(ctx, "depth copy back", fetched);
	  HIP_CHECK(hipMemcpyAsync(pinned, state.buffer("depth.staging").ptr, fetched, hipMemcpyDeviceToHost, s)); }
	HIP_CHECK(hipEventRecord(state.events[1], s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	add_seconds(state, 3);
	state.flushed = state.written; ++state.stats.text_windows;
	*bytes = fetched;
	return AGPU_OK;
}

int read_counters(agpu_ctx* ctx) {
	DepthState& state = ctx->depth;
	unsigned long long host_counters[COUNTER_WORDS] = {};
	HIP_CHECK(hipMemcpyAsync(host_counters, state.buffer("depth.counters").ptr, sizeof(host_counters), hipMemcpyDeviceToHost, ctx->stream));
	HIP_CHECK(hipStreamSynchronize(ctx->stream));
	state.stats.records = host_counters[COUNTER_RECORDS]; state.stats.segments = host_counters[COUNTER_SEGMENTS]; state.stats.covered_positions = host_counters[COUNTER_COVERED];
	state.stats.aligned_bases = host_counters[COUNTER_ALIGNED]; state.stats.max_depth = host_counters[COUNTER_MAX_DEPTH];
	return AGPU_OK;
}

void leave(agpu_ctx* ctx) {
	DepthState& state = ctx->depth;
	(void) hipStreamSynchronize(ctx->stream);
	for (int k = 0; k < 2; ++k) if (state.events[k]) { (void) hipEventDestroy(state.events[k]); state.events[k] = nullptr; }
	state.release_all();
	state.active = false;
}

}

extern "C" {

int agpu_depth_begin(agpu_ctx* ctx, const uint32_t* ref_length, const char* names, const uint32_t* name_offset, uint32_t n_ref, agpu_depth_info* info) {
	if (!ctx || !info || (n_ref > 0 && (!ref_length || !names || !name_offset))) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	ResidentStream resident;
	TRY(resident_stream(ctx, "agpu_depth_begin", "a coverage track of one sample over several GPUs is not supported", ctx->depth.active ? "agpu_depth_end must run first" : nullptr, resident));
	if (n_ref >= 0x7FFFFFFFu) { set_last_error("agpu_depth_begin: too many references"); return AGPU_ERR_INVALID; }
	for (uint32_t t = 0; t < n_ref; ++t) if (name_offset[t + 1] < name_offset[t]) { set_last_error("agpu_depth_begin: the offsets of the names must ascend"); return AGPU_ERR_INVALID; }
	HIP_CHECK(hipSetDevice(ctx->device));
	ctx->depth.active = true; // (the stream is read from here on: nothing of this context is given back when an allocation fails)
	struct Guard { agpu_ctx* ctx; bool keep; ~Guard() { if (!keep) leave(ctx); } } guard = { ctx, false };
	for (int k = 0; k < 2; ++k) HIP_CHECK(hipEventCreate(&ctx->depth.events[k]));
	const int status = mark_and_scan(ctx, resident, ref_length, names, name_offset, n_ref);
	collect_kernel_samples(ctx);
	if (status != AGPU_OK) return status;
	{ std::lock_guard<std::mutex> lock(ctx->profile_mutex); if (!ctx->failed_launch.empty()) { set_last_error("agpu_depth_begin: " + ctx->failed_launch); return AGPU_ERR_DEVICE; } }
	TRY(read_counters(ctx));
	info->positions = ctx->depth.slots; info->window_bytes = ctx->depth.text_window;
	guard.keep = true;
	return AGPU_OK;
}

int agpu_depth_next(agpu_ctx* ctx, void* pinned, uint64_t capacity, uint64_t* bytes) {
	if (!ctx || !bytes) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	DepthState& state = ctx->depth;
	if (!state.active) { set_last_error("agpu_depth_begin must run first"); return AGPU_ERR_INVALID; }
	*bytes = 0;
	if (!pinned || capacity < state.text_window) { set_last_error("agpu_depth_next: the buffer is smaller than a window (agpu_depth_info.window_bytes)"); return AGPU_ERR_INVALID; }
	HIP_CHECK(hipSetDevice(ctx->device));
	hipStream_t s = ctx->stream;
	struct Collect { agpu_ctx* ctx; ~Collect() { collect_kernel_samples(ctx); } } collect = { ctx };
	for (;;) {
		if (state.written < state.batch_end) { // lines of the runs found last that are not in a staging window yet: as many bytes as the window at hand still takes
			const uint64_t from = state.written, upto = std::min(state.batch_end, state.flushed + state.text_window);
			HIP_CHECK(hipEventRecord(state.events[0], s));
			{ KernelTimer timer(ctx, "depth_text_kernel", state.batch_runs * 24 + (upto - from));
			  depth_text_kernel<<<grid_for(state.batch_runs), BLOCK, 0, s>>>(state.buffer("depth.runs").as<uint4>(), state.buffer("depth.line_offset").as<uint64_t>(), state.batch_runs, state.buffer("depth.names").as<char>(),
			    state.buffer("depth.name_offset").as<uint32_t>(), state.batch_begin, from, upto, state.flushed, state.buffer("depth.staging").as<uint8_t>()); }
			HIP_CHECK(hipEventRecord(state.events[1], s));
			HIP_CHECK(hipStreamSynchronize(s));
			HIP_CHECK(hipGetLastError());
			add_seconds(state, 3);
			state.written = upto;
			if (state.written - state.flushed == state.text_window) return fetch(ctx, pinned, bytes); // a full window
			continue;
		}
		if (state.next_slot < state.slots) { TRY(find_runs(ctx)); continue; }
		if (state.carry) { set_last_error("agpu_depth_next: a run is open behind the last contig"); return AGPU_ERR_DEVICE; }
		TRY(read_counters(ctx));
		if (state.written > state.flushed) return fetch(ctx, pinned, bytes); // the last window
		return AGPU_OK;
	}
}

int agpu_depth_end(agpu_ctx* ctx, agpu_depth_stats* stats) {
	if (!ctx) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	if (stats) memset(stats, 0, sizeof(*stats));
	if (!ctx->depth.active) return AGPU_OK;
	(void) hipSetDevice(ctx->device);
	if (stats) *stats = ctx->depth.stats;
	leave(ctx);
	collect_kernel_samples(ctx);
	return AGPU_OK;
}

int agpu_depth_allocated_bytes(agpu_ctx* ctx, uint64_t* bytes) {
	if (!ctx || !bytes) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	*bytes = ctx->depth.allocated();
	return AGPU_OK;
}

}
