// arriba_amd/csrc/device/mismapper_heavy.hpp -- mismapper_heavy_kernel, the second pass of filter_mismappers (agpu_mismappers.hip), and its launchers.
// Every instantiation of the kernel is a translation unit of its own (agpu_mismappers_heavy_*.hip: the header, then AGPU_MISMAPPER_HEAVY_LAUNCHER(name of the launcher, waves, sweep_only)):
// one instantiation takes hipcc minutes, and make compiles the files side by side.  agpu_mismappers.hip calls the launchers declared at the end.
#pragma once
#include <hip/hip_runtime.h>
#include "agpu_context.hpp"
#include "mismapper_core.hpp"
#include "device_utils.hpp"

namespace { // (as in agpu_mismappers.hip, where the kernel stood in that file's anonymous namespace: the name of an instantiation in a profiler's trace is the one it had)
using namespace agpu;

// Second pass, one wavefront per heavy read: the read positions one after the other, the seeds of a position split among the 64 lanes (every seed of the outermost
// loop of align() is an independent attempt), full stack, no budget; the segment in LDS is shared by the lanes, and so is the memo of failed nested calls
// (AlignMemo, mismapper_core.hpp: it turns the exponential re-evaluation of the reference's recursion into one search per distinct call).  The workgroups are
// persistent: each owns one memo table in HBM and takes the next heavy read from a queue (counters[4]) when it is done with one -- the searches differ in
// length by orders of magnitude, a fixed share per workgroup would wait for the unluckiest one.  The kernel waits for dependent loads (k-mer table -> hit list ->
// genome bases -> memo slot), so the number of wavefronts in flight is what sets its speed: 5120 workgroups of one wavefront = 5 per SIMD.
// Tried and taken back in round 5 (profiles/r05o_waves6.json, r05p_*, r05q_*): (a) six wavefronts per SIMD -- 80 VGPRs, 177 spilled: 457 ms instead of 419 at 10^8 fragments;
// (b) TWO searches per wavefront, the two strands of a gene at once on 32 lanes each with a sweep, a memo and lists of their own (the calls of a block kept in LDS cut from 256 to
// 64 to make room): the same verdict bytes under every schedule of the GPU tier, but 496 ms -- the halves of a wavefront go separate ways through the walks and the look-ups of the
// read positions take twice the turns; with 64 calls in LDS and one search per wavefront: 432 ms.
// SWEEP_ONLY: the searches go through the sweep or are given up -- no recursion, no stack of frames in the kernel; the reads of the searches given up are appended to `leftover`
// (counters[5]) and done by the instantiation that holds everything.  queue: the index of the queue's counter (the second launch has a queue of its own).
template <int WAVES_PER_SIMD, bool SWEEP_ONLY> __global__ void __launch_bounds__(64, WAVES_PER_SIMD) mismapper_heavy_kernel(BatchView b, AnnotationView ann, GenomeView genome, KmerIndexView kmers, SpliceSiteView splice, const uint32_t* heavy, uint32_t n_heavy, int32_t max_mate_gap,
                                                             unsigned long long* memo_tables, uint32_t memo_slots, unsigned long long* task_lists, uint32_t task_capacity, bool by_sweep, unsigned long long* read_times, unsigned int* counters, uint32_t* leftover, int queue, bool lds_front, bool strands_together) {
	__shared__ uint8_t segment_bases[2 * 304]; // (the segment being searched and its reverse complement)
	__shared__ uint8_t segment_chars[2 * 312];  // (... as characters, eight zero bytes behind each)
	__shared__ AlignSweep sweep;
	__shared__ AlignMemo memo;
	__shared__ AlignWorklist worklist;
	__shared__ uint32_t worklist_state[4];
	__shared__ unsigned long long memo_front[ALIGN_MEMO_FRONT_SLOTS]; // (mismapper_core.hpp: the first keys of a search never leave the CU)
	__shared__ unsigned long long list_head[2 * ALIGN_LIST_HEAD_TASKS];
	__shared__ uint32_t memo_spilled;
	__shared__ uint32_t next_job;
	__shared__ uint32_t study[16];
	if (threadIdx.x == 0) {
		worklist.stats = read_times != nullptr ? study : nullptr;
		memo.slots = memo_tables + (size_t) blockIdx.x * memo_slots; memo.mask = memo_slots - 1; memo.epoch = 0;
		memo.front = lds_front ? memo_front : nullptr; memo.front_mask = lds_front ? ALIGN_MEMO_FRONT_SLOTS - 1 : 0; memo.spilled = lds_front ? &memo_spilled : nullptr; memo_spilled = 0;
		worklist.head = lds_front ? list_head : nullptr; worklist.head_capacity = lds_front ? ALIGN_LIST_HEAD_TASKS : 0;
		worklist.words = task_lists != nullptr ? task_lists + (size_t) blockIdx.x * task_capacity * 2 : nullptr; worklist.capacity = task_capacity; worklist.state = worklist_state;
		worklist.sweep = by_sweep ? &sweep : nullptr; // one sweep over the read positions, every seed walked once (mismapper_core.hpp: AlignSweep)
		worklist.relevant_words = task_lists != nullptr ? task_lists + ((size_t) gridDim.x + blockIdx.x) * task_capacity * 2 : nullptr; worklist.relevant_capacity = task_capacity; // (the second half of the buffer: the calls of a block beyond those kept in LDS)
	}
	for (uint32_t k = threadIdx.x; k < ALIGN_MEMO_FRONT_SLOTS; k += 64) memo_front[k] = 0; // (epoch 0 = free)
	__syncthreads();
	__shared__ int64_t given_up; // (SWEEP_ONLY: < 0 when a search of the read was not one for the sweep)
	AlignFrame stack[SWEEP_ONLY ? 1 : ALIGN_MAX_DEPTH];
	AlignRunnerT<SWEEP_ONLY> runner; runner.stack = stack; runner.lane = threadIdx.x; runner.lanes = 64; runner.budget = SWEEP_ONLY ? &given_up : nullptr; runner.max_depth = SWEEP_ONLY ? 1 : ALIGN_MAX_DEPTH;
	runner.lanes_share_seeds = true; // a read lands here because its search is long: the lanes split the seeds of every read position (when the task list is off or overflows)
	runner.memo = &memo;
	runner.worklist = task_lists != nullptr ? &worklist : nullptr; // the search as rounds of up to 64 tasks (mismapper_core.hpp: AlignWorklist)
	runner.cache = segment_bases; runner.cache_stride = 1; runner.cache_capacity = 304; runner.cache2 = segment_bases + 304; runner.strands_together = strands_together; runner.chars = segment_chars; runner.chars2 = segment_chars + 312;
	while (true) {
		__syncthreads(); // (every lane has read next_job of the previous round)
		if (threadIdx.x == 0) { next_job = atomicAdd(&counters[queue], 1u); given_up = 0; }
		__syncthreads();
		if (next_job >= n_heavy) break;
		const uint32_t read = heavy[next_job];
		const unsigned long long started = read_times != nullptr ? wall_clock64() : 0ull;
		if (read_times != nullptr && threadIdx.x == 0) for (int k = 0; k < 16; ++k) study[k] = 0;
		const bool verdict = is_mismapper(b, ann, genome, kmers, splice, read, max_mate_gap, runner);
		if (SWEEP_ONLY && runner.exhausted()) { if (threadIdx.x == 0) leftover[atomicAdd(&counters[5], 1u)] = read; continue; } // (the same for every lane: written behind a barrier)
		if (verdict && threadIdx.x == 0) { b.filter[read] = FILTER_mismappers; atomicAdd(&counters[1], 1u); }
		if (read_times != nullptr && threadIdx.x == 0) { // (ARRIBA_MISMAPPER_TIMES=1: ticks of the 100 MHz clock per read, and what the search of the read consisted of)
			read_times[4 * (size_t) next_job] = wall_clock64() - started; read_times[4 * (size_t) next_job + 1] = (unsigned long long) study[0] << 32 | study[1]; read_times[4 * (size_t) next_job + 2] = (unsigned long long) study[2] << 32 | study[3];
			read_times[4 * (size_t) next_job + 3] = (unsigned long long) read << 8 | b.n_aln[read];
			atomicAdd(&read_times[4 * (size_t) n_heavy], (unsigned long long) study[4]); atomicAdd(&read_times[4 * (size_t) n_heavy + 1], (unsigned long long) study[5]); atomicAdd(&read_times[4 * (size_t) n_heavy + 2], (unsigned long long) study[6]);
			for (int k = 8; k < 16; ++k) atomicAdd(&read_times[4 * (size_t) n_heavy + 4 + (k - 8)], (unsigned long long) study[k]);
		}
	}
}

} // namespace

namespace agpu {
#define AGPU_MISMAPPER_HEAVY_ARGUMENTS uint32_t workgroups, hipStream_t stream, BatchView b, AnnotationView ann, GenomeView genome, KmerIndexView kmers, SpliceSiteView splice, const uint32_t* heavy, uint32_t n_heavy, int32_t max_mate_gap, \
	unsigned long long* memo_tables, uint32_t memo_slots, unsigned long long* task_lists, uint32_t task_capacity, bool by_sweep, unsigned long long* read_times, unsigned int* counters, uint32_t* leftover, int queue, bool lds_front, bool strands_together
// the launch of one instantiation: `workgroups` persistent workgroups of one wavefront on `stream`
void launch_mismapper_heavy_6_sweep_only(AGPU_MISMAPPER_HEAVY_ARGUMENTS);
void launch_mismapper_heavy_5_sweep_only(AGPU_MISMAPPER_HEAVY_ARGUMENTS);
void launch_mismapper_heavy_4_sweep_only(AGPU_MISMAPPER_HEAVY_ARGUMENTS);
void launch_mismapper_heavy_5_everything(AGPU_MISMAPPER_HEAVY_ARGUMENTS);
void launch_mismapper_heavy_4_everything(AGPU_MISMAPPER_HEAVY_ARGUMENTS);
#define AGPU_MISMAPPER_HEAVY_LAUNCHER(name, WAVES, SWEEP_ONLY) void agpu::name(AGPU_MISMAPPER_HEAVY_ARGUMENTS) { \
	mismapper_heavy_kernel<WAVES, SWEEP_ONLY><<<workgroups, 64, 0, stream>>>(b, ann, genome, kmers, splice, heavy, n_heavy, max_mate_gap, memo_tables, memo_slots, task_lists, task_capacity, by_sweep, read_times, counters, leftover, queue, lds_front, strands_together); }
} // namespace agpu
