// arriba_amd/csrc/device/resident_stream.hpp -- what the consumers of the record stream that the last ingest left in HBM have in common (--sorted-bam, --mark-duplicates,
// --supporting-alignments, --virus-expression, --coverage, --gene-counts, --splice-junctions, --allele-counts, --realign-reads, --rna-metrics, --variant-sites, --indel-sites): the guard in front of the stream
// (resident_stream), the macros and launch helpers of their host code, and the frame of those that do their work inside one call (one_shot).  Their state is a StreamConsumer
// (agpu_context.hpp).  A file names its option before it includes this header: #define AGPU_OPTION "--gene-counts".
#ifndef AGPU_RESIDENT_STREAM_HPP
#define AGPU_RESIDENT_STREAM_HPP 1

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <string>
#include "agpu_context.hpp"

#define HIP_CHECK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { set_last_error(std::string(#call) + ": " + hipGetErrorString(e_)); return AGPU_ERR_DEVICE; } } while (0)
#define TRY(call) do { const int status_ = (call); if (status_ != AGPU_OK) return status_; } while (0)
// AGPU_ALLOC_MESSAGE(buffer): what a failed allocation says, for the two files that do not say it like the others.  A file whose state keeps the peak of its buffers
// (--splice-junctions, --allele-counts, --variant-sites, --indel-sites) defines ALLOC itself, with state.note_peak() for `then`.
#ifndef AGPU_ALLOC_MESSAGE
#define AGPU_ALLOC_MESSAGE(buffer) AGPU_OPTION ": hipMalloc failed (" buffer ")"
#endif
#define AGPU_ALLOC(buffer, bytes, then) do { if (!(buffer).allocate(bytes)) { set_last_error(AGPU_ALLOC_MESSAGE(#buffer)); return AGPU_ERR_NO_MEMORY; } then; } while (0)
#ifndef ALLOC
#define ALLOC(buffer, bytes) AGPU_ALLOC(buffer, bytes, (void) 0)
#endif

namespace agpu {

const int BLOCK = 256; // threads of a workgroup
const uint64_t LAUNCH_ITEMS = 1ull << 30; // a kernel with one lane per record (or slot, or crossing) is launched in pieces that stay below 2^32 work-items

inline unsigned int grid_for(uint64_t n) { return (unsigned int) std::max<uint64_t>((n + BLOCK - 1) / BLOCK, 1); }
// launch(first, grid): the workgroups of items [first, first + items) of n; a kernel that gives an item more than one lane says how many items a launch may take
template <class Launch> inline void for_each_launch_piece(uint64_t n, Launch launch, uint64_t items = LAUNCH_ITEMS) {
	for (uint64_t first = 0; first < n; first += items) launch(first, grid_for(std::min(items, n - first)));
}

// a rocPRIM call with its temporary storage in a buffer of the consumer: call(nullptr, bytes) asks for the size, call(storage, bytes) does the work, timed as `name`
template <class Call> int with_temporary(agpu_ctx* ctx, DeviceBuffer& temporary_buffer, const char* name, uint64_t bytes, Call call) {
	size_t temporary = 0;
	HIP_CHECK(call(nullptr, temporary));
	if (temporary > temporary_buffer.capacity) AGPU_ALLOC(temporary_buffer, temporary, (void) 0);
	KernelTimer timer(ctx, name, bytes);
	HIP_CHECK(call(temporary_buffer.ptr, temporary));
	return AGPU_OK;
}
// knobs of the environment, for the tests and the measurements: a size (at least 1, at most `most`), and the bits of a name hash that the tables of read names compare (0 .. 64)
inline uint64_t knob_of(const char* name, uint64_t otherwise, uint64_t most) {
	const char* knob = getenv(name);
	uint64_t value = otherwise;
	if (knob != nullptr && knob[0] != 0) value = std::max<uint64_t>(strtoull(knob, nullptr, 10), 1);
	return std::min(value, most);
}
inline uint32_t hash_bits_knob(const char* name) {
	const char* knob = getenv(name);
	if (knob == nullptr || knob[0] == 0) return 64;
	const long bits = atol(knob);
	return bits < 0 ? 0u : bits > 64 ? 64u : (uint32_t) bits;
}
inline unsigned int bits_of(uint64_t below) { unsigned int bits = 1; while (bits < 32 && (1ull << bits) < below) ++bits; return bits; } // enough for every value < below

// The guard: is the stream of the last ingest still there, and may `entry` (the name of the entry point) read it.  several_gpus: its sentence for a part of a sample; busy: not
// null if a call of the consumer is under way, and what to say then; needs: what else the consumer reads.  Fills `view`, or sets the message and returns the status.  The consumer
// sets `active` of its state right behind it: from there on nothing of the context is given back when an allocation fails (DeviceBuffer::release_idle_buffers).
enum { NEEDS_ANNOTATION = 1, NEEDS_GENOME = 2, NEEDS_REFERENCES = 4 /* n_ref references, those of the header of the ingest */ };
inline int resident_stream(agpu_ctx* ctx, const char* entry, const char* several_gpus, const char* busy, ResidentStream& view, unsigned int needs = 0, uint32_t n_ref = 0) {
	const std::string name = std::string(entry) + ": ";
	if (ctx->ingest_active) { set_last_error(name + "an ingest is under way on this context (it comes behind agpu_ingest_finish)"); return AGPU_ERR_INVALID; }
	if (busy != nullptr) { set_last_error(name + busy); return AGPU_ERR_INVALID; }
	if (ctx->last_ingest_part_of_sample) { set_last_error(several_gpus); return AGPU_ERR_INVALID; }
	const uint64_t size = ctx->last_ingest_stream_size, base = ctx->last_ingest_first_record, n = ctx->last_ingest_records;
	DeviceBuffer& record_offset = ctx->scratch("ingest.record_offset");
	if (!ctx->batch_from_ingest || !ctx->last_ingest_kept || ctx->ingest_stream.ptr == nullptr || record_offset.ptr == nullptr || ctx->ingest_stream.capacity < (size + 3) / 4 * 4 || record_offset.capacity < n * 8) {
		set_last_error(name + "the record stream of the last ingest is not on the device any more (it was given back under memory pressure, another ingest has begun, or there was no ingest)");
		return AGPU_ERR_INVALID;
	}
	if (n >= 0xFFFFFFF0ull || base > size) { set_last_error(name + "more than 2^32-16 alignment records"); return AGPU_ERR_INVALID; }
	if ((needs & NEEDS_ANNOTATION) && !ctx->have_annotation) { set_last_error(name + "agpu_upload_annotation must run first"); return AGPU_ERR_INVALID; }
	if ((needs & NEEDS_GENOME) && !ctx->have_genome) { set_last_error(name + "agpu_upload_genome must run first"); return AGPU_ERR_INVALID; }
	if ((needs & NEEDS_REFERENCES) && (n_ref != ctx->ingest_n_targets || (n_ref > 0 && ctx->ingest_tid_to_contig.ptr == nullptr))) { set_last_error(name + "the lengths are not those of the references of the last ingest"); return AGPU_ERR_INVALID; }
	view.stream = ctx->ingest_stream.as<uint8_t>(); view.stream_size = size; view.first_record = base; view.records = n; view.record_offset = record_offset.as<uint64_t>();
	return AGPU_OK;
}

// The frame of a consumer that does its work inside one call: from `active` to the last of its buffers nothing of the context is given back; body(events) runs between
// N_EVENTS fresh events; nothing of a failed body is in flight when release(status) lets the buffers go; a launch the runtime refused fails the call under the name of the entry
// point.  (A body whose events are read behind it synchronises the stream itself, whatever its status.)
template <int N_EVENTS, class Body, class Release> int one_shot(agpu_ctx* ctx, StreamConsumer& state, const char* entry, Body body, Release release) {
	state.active = true;
	hipEvent_t events[N_EVENTS] = {};
	int status = AGPU_OK;
	for (int k = 0; k < N_EVENTS && status == AGPU_OK; ++k) if (hipEventCreate(&events[k]) != hipSuccess) { set_last_error(AGPU_OPTION ": hipEventCreate failed"); status = AGPU_ERR_DEVICE; }
	if (status == AGPU_OK) status = body(events);
	if (status != AGPU_OK) (void) hipStreamSynchronize(ctx->stream);
	for (int k = 0; k < N_EVENTS; ++k) if (events[k]) (void) hipEventDestroy(events[k]);
	release(status);
	state.active = false;
	collect_kernel_samples(ctx);
	if (status != AGPU_OK) return status;
	std::lock_guard<std::mutex> lock(ctx->profile_mutex);
	if (!ctx->failed_launch.empty()) { set_last_error(std::string(entry) + ": " + ctx->failed_launch); return AGPU_ERR_DEVICE; }
	return AGPU_OK;
}

}

#endif
