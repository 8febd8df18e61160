// arriba_amd/csrc/device/agpu_rnametrics.hip -- --rna-metrics on the MI355X: the alignment QC table of the record stream of the last ingest (include/arriba_gpu.h:
// agpu_rna_metrics).  What decides a number is rnametrics_core.hpp, which the host steps as well (arriba_amd/csrc/host/rna_metrics.cpp); the rule is DESIGN.md 4.19.  Here is
//   rnametrics_record_kernel   one lane per record through ingest.record_offset, persistent workgroups with a grid stride: the fixed fields, NH, the CIGAR, and every block through
//                              the runs of the region track (one lower bound per block, galloping from the run the previous block ended in).  A lane keeps its scalar counters in
//                              registers over all its records; when the workgroup is done they are summed over the wavefront by shuffles and over the workgroup in LDS.  The three
//                              histograms (256 + 1002 + 100 bins) live in LDS as 64-bit words with LDS atomics, so no bin can overflow.  Every word of the workgroup that is not zero
//                              leaves as one 64-bit global atomic.  PLAIN (ARRIBA_RNAMETRICS_PLAIN_ATOMICS=1, for the measurement): no LDS, every lane adds to global memory.
// All sums are integer and commute: the block is the same under every schedule.  The stream and the track are only read.  Integer work bound by dependent loads: record_offset ->
// the head of the record -> its CIGAR and aux bytes -> run_start (the search) -> run_bits / run_gene / run_rank -> gene_body; no MFMA.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#define AGPU_OPTION "--rna-metrics"
#include "resident_stream.hpp"
#include "device_utils.hpp"
#include "rnametrics_core.hpp"

using namespace agpu;

namespace {

const uint64_t LAUNCH_RECORDS = 1ull << 30; // the records of one launch: its grid stays far below 2^30 work-items
const unsigned int BLOCKS_PER_CU = 4;       // persistent workgroups: what the registers of the kernel let a CU hold (3 wavefronts per SIMD), and one more to fill in behind the first that is done

// the three histograms of a counter block in LDS or in global memory: 64-bit atomics either way
struct AtomicBins {
	unsigned long long* words;
	__device__ __forceinline__ void mapq(uint32_t q) { atomicAdd(&words[RNAM_MAPQ_AT + q], 1ull); }
	__device__ __forceinline__ void insert(uint32_t bin) { atomicAdd(&words[RNAM_INSERT_AT + bin], 1ull); }
	__device__ __forceinline__ void body(uint32_t bin, uint64_t bases) { atomicAdd(&words[RNAM_BODY_AT + bin], (unsigned long long) bases); }
};

// records [first, first + count) of the stream; out: [RNAM_WORDS], zeroed before the first launch
template <bool PLAIN> __global__ void __launch_bounds__(BLOCK) rnametrics_record_kernel(RnamInput in, const uint64_t* __restrict__ record_offset, uint64_t first, uint64_t count, unsigned long long* out) {
	__shared__ unsigned long long shared[PLAIN ? 1 : RNAM_WORDS];
	if (!PLAIN) {
		for (uint32_t w = threadIdx.x; w < RNAM_WORDS; w += BLOCK) shared[w] = 0;
		__syncthreads();
	}
	AtomicBins bins = { PLAIN ? out : shared };
	RnamLane lane;
	rnam_clear(lane);
	const uint64_t stride = (uint64_t) gridDim.x * BLOCK;
	for (uint64_t r = (uint64_t) blockIdx.x * BLOCK + threadIdx.x; r < count; r += stride) rnam_record(in, record_offset[first + r], lane, bins);
	if (PLAIN) {
		AGPU_UNROLL for (int k = 0; k < RNAM_SCALARS; ++k) if (lane.c[k] != 0) atomicAdd(&out[k], (unsigned long long) lane.c[k]);
		return;
	}
	AGPU_UNROLL for (int k = 0; k < RNAM_SCALARS; ++k) { // (no lane has left: the shuffles see the whole wavefront)
		const unsigned long long sum = wave_sum((unsigned long long) lane.c[k]);
		if ((threadIdx.x & 63u) == 0 && sum != 0) atomicAdd(&shared[k], sum);
	}
	__syncthreads();
	for (uint32_t w = threadIdx.x; w < RNAM_WORDS; w += BLOCK) { const unsigned long long sum = shared[w]; if (sum != 0) atomicAdd(&out[w], sum); }
}

bool plain_atomics_knob() { const char* knob = getenv("ARRIBA_RNAMETRICS_PLAIN_ATOMICS"); return knob != nullptr && knob[0] == '1'; } // (for the measurement of DESIGN.md 4.19)

template <class T> int upload(DeviceBuffer& buffer, const T* from, size_t n, hipStream_t s) {
	ALLOC(buffer, std::max<size_t>(n, 1) * sizeof(T));
	if (n > 0) HIP_CHECK(hipMemcpyAsync(buffer.ptr, from, n * sizeof(T), hipMemcpyHostToDevice, s));
	return AGPU_OK;
}

// the track on the device: copied when the context sees its id for the first time
int bring_track(agpu_ctx* ctx, const agpu_region_track* track) {
	RnametricsState& state = ctx->rnametrics;
	if (state.track_id == track->id && state.track_id != 0) return AGPU_OK;
	hipStream_t s = ctx->stream;
	state.track_id = 0;
	DeviceBuffer& contig_offset = state.buffer("rnametrics.track.contig_offset"); DeviceBuffer& run_start = state.buffer("rnametrics.track.run_start"); DeviceBuffer& run_bits = state.buffer("rnametrics.track.run_bits");
	DeviceBuffer& run_gene = state.buffer("rnametrics.track.run_gene"); DeviceBuffer& run_rank = state.buffer("rnametrics.track.run_rank"); DeviceBuffer& gene_body = state.buffer("rnametrics.track.gene_body");
	TRY(upload(contig_offset, track->contig_offset, (size_t) track->n_contigs + 1, s)); TRY(upload(run_start, track->run_start, track->n_runs, s)); TRY(upload(run_bits, track->run_bits, track->n_runs, s));
	TRY(upload(run_gene, track->run_gene, track->n_runs, s)); TRY(upload(run_rank, track->run_rank, track->n_runs, s)); TRY(upload(gene_body, track->gene_body, track->n_genes, s));
	HIP_CHECK(hipStreamSynchronize(s)); // (the sources are pageable memory of the caller)
	state.track = *track;
	state.track.contig_offset = contig_offset.as<uint32_t>(); state.track.run_start = run_start.as<int32_t>(); state.track.run_bits = run_bits.as<uint8_t>();
	state.track.run_gene = run_gene.as<uint32_t>(); state.track.run_rank = run_rank.as<uint32_t>(); state.track.gene_body = gene_body.as<uint32_t>();
	state.track_id = track->id;
	return AGPU_OK;
}

// what the kernel relies on, checked on the host's copy before anything is uploaded: every contig has a run, which starts at 0, and starts ascend
bool track_is_sound(const agpu_region_track* track) {
	if (track->id == 0 || !track->contig_offset || (track->n_runs > 0 && (!track->run_start || !track->run_bits || !track->run_gene || !track->run_rank)) || (track->n_genes > 0 && !track->gene_body)) return false;
	if (track->contig_offset[0] != 0 || track->contig_offset[track->n_contigs] != track->n_runs) return false;
	for (uint32_t c = 0; c < track->n_contigs; ++c) {
		const uint32_t begin = track->contig_offset[c], end = track->contig_offset[c + 1];
		if (begin >= end || end > track->n_runs || track->run_start[begin] != 0) return false;
		for (uint32_t r = begin + 1; r < end; ++r) if (track->run_start[r] <= track->run_start[r - 1]) return false;
	}
	return true;
}

int count(agpu_ctx* ctx, const ResidentStream& resident, const agpu_region_track* track, const uint32_t* ref_length, uint32_t n_ref, uint64_t* counters_out, hipEvent_t* events) {
	RnametricsState& state = ctx->rnametrics;
	hipStream_t s = ctx->stream;
	const uint64_t size = resident.stream_size, n = resident.records;
	TRY(bring_track(ctx, track));
	DeviceBuffer& counters = state.buffer("rnametrics.counters"); DeviceBuffer& lengths = state.buffer("rnametrics.ref_length");
	ALLOC(counters, RNAM_WORDS * 8); ALLOC(lengths, std::max<size_t>(n_ref, 1) * 4);
	state.stats.peak_bytes = state.allocated();
	HIP_CHECK(hipMemsetAsync(counters.ptr, 0, RNAM_WORDS * 8, s));
	if (n_ref > 0) { HIP_CHECK(hipMemcpyAsync(lengths.ptr, ref_length, (size_t) n_ref * 4, hipMemcpyHostToDevice, s)); HIP_CHECK(hipStreamSynchronize(s)); } // (the source is pageable memory of the caller)
	HIP_CHECK(hipEventRecord(events[0], s));
	if (n > 0) {
		int compute_units = 0;
		HIP_CHECK(hipDeviceGetAttribute(&compute_units, hipDeviceAttributeMultiprocessorCount, ctx->device));
		const uint64_t persistent = (uint64_t) std::max(compute_units, 1) * BLOCKS_PER_CU;
		RnamInput in;
		in.stream = resident.stream; in.stream_size = size; in.track = state.track;
		in.tid_to_contig = ctx->ingest_tid_to_contig.as<uint32_t>(); in.ref_length = lengths.as<uint32_t>(); in.n_ref = n_ref;
		const uint64_t* record_offset = resident.record_offset;
		const bool plain = plain_atomics_knob();
		KernelTimer timer(ctx, "rnametrics_record_kernel", n * 8 + n * 72);
		for (uint64_t first = 0; first < n; first += LAUNCH_RECORDS) {
			const uint64_t records = std::min(LAUNCH_RECORDS, n - first);
			const unsigned int grid = (unsigned int) std::min<uint64_t>((records + BLOCK - 1) / BLOCK, persistent);
			if (plain) rnametrics_record_kernel<true><<<grid, BLOCK, 0, s>>>(in, record_offset, first, records, counters.as<unsigned long long>());
			else rnametrics_record_kernel<false><<<grid, BLOCK, 0, s>>>(in, record_offset, first, records, counters.as<unsigned long long>());
		}
	}
	HIP_CHECK(hipEventRecord(events[1], s));
	static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the counters are copied as they are");
	HIP_CHECK(hipMemcpyAsync(counters_out, counters.ptr, RNAM_WORDS * 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	state.stats.records = counters_out[RNAM_RECORDS]; state.stats.base_records = counters_out[RNAM_BASE_RECORDS]; state.stats.blocks = counters_out[RNAM_BLOCKS]; state.stats.segments = counters_out[RNAM_SEGMENTS];
	state.stats.track_runs = track->n_runs;
	if (state.stats.records != n) { set_last_error("agpu_rna_metrics: the kernel counted " + std::to_string(state.stats.records) + " records of " + std::to_string(n)); return AGPU_ERR_DEVICE; }
	float ms = 0;
	if (hipEventElapsedTime(&ms, events[0], events[1]) == hipSuccess) state.stats.seconds[0] = ms / 1000.0;
	return AGPU_OK;
}

}

extern "C" {

int agpu_rna_metrics(agpu_ctx* ctx, const agpu_region_track* track, const uint32_t* ref_length, uint32_t n_ref, uint64_t* counters, agpu_rna_metrics_stats* stats) {
	if (!ctx || !track || !counters || (n_ref > 0 && !ref_length)) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	if (stats) memset(stats, 0, sizeof(*stats));
	ResidentStream resident;
	TRY(resident_stream(ctx, "agpu_rna_metrics", "rna metrics of one sample over several GPUs are not supported", nullptr, resident, NEEDS_REFERENCES, n_ref));
	if (!track_is_sound(track)) { set_last_error("agpu_rna_metrics: the region track is not one ahost_region_track built (a contig without a run, starts that do not ascend from 0, or no id)"); return AGPU_ERR_INVALID; }
	HIP_CHECK(hipSetDevice(ctx->device));
	RnametricsState& state = ctx->rnametrics;
	memset(&state.stats, 0, sizeof(state.stats));
	TRY(one_shot<2>(ctx, state, "agpu_rna_metrics", [&](hipEvent_t* events) { return count(ctx, resident, track, ref_length, n_ref, counters, events); }, [&](int status) {
		state.buffer("rnametrics.counters").release(); state.buffer("rnametrics.ref_length").release();
		if (status != AGPU_OK && state.track_id == 0) state.release_all(); // (a track that did not arrive whole)
	}));
	if (stats) *stats = state.stats;
	return AGPU_OK;
}

int agpu_rna_metrics_allocated_bytes(agpu_ctx* ctx, uint64_t* bytes) {
	if (!ctx || !bytes) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	*bytes = ctx->rnametrics.allocated();
	return AGPU_OK;
}

}
