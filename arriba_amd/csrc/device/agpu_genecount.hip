// arriba_amd/csrc/device/agpu_genecount.hip -- --gene-counts on the MI355X: reads per gene of the record stream of the last ingest, three columns (unstranded, read strand = gene
// strand, read strand != gene strand), the numbers of STAR's ReadsPerGene.out.tab (include/arriba_gpu.h: agpu_gene_counts).  What decides a number is genecount_core.hpp, which the
// host steps as well (arriba_amd/csrc/host/gene_counts.cpp); the rule is DESIGN.md 4.15.  Here are
//   genecount_name_kernel     one lane per record through ingest.record_offset: its QNAME into the open-addressing table of markdup_core.hpp (64-bit atomicCAS, every hit confirmed
//                             by the bytes), the id of its template -- the record whose name got there first --, and, if it is primary, its claim on its slot: atomicMin of the
//                             record number
//   genecount_assign_kernel   one lane per record that is its own template id: the NH of both claimed ends, their CIGARs block by block through the exon index (the bins directory
//                             for the first block, the hint from there on), the row of the template in each column, and the adds into counts[3][n_genes + 4]: the four special rows
//                             are summed over the wavefront first (one atomic per wavefront, row and column); for the gene rows the lanes of a wavefront that hold the same gene
//                             merge their add (a leader loop over the distinct values of the active lanes): a highly expressed gene otherwise takes millions of adds to one address
// Counters are unsigned integers and sums commute: the table is the same under every schedule.  The stream is only read.  Integer work bound by dependent loads: record_offset ->
// the head of the record -> its name / CIGAR / aux bytes in the name and assign passes, and keys -> member_offset -> members -> exon_gene -> gene_bits in the index walk; no MFMA,
// no LDS.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#define AGPU_OPTION "--gene-counts"
#include "resident_stream.hpp"
#include "device_utils.hpp"
#include "genecount_core.hpp"

using namespace agpu;

namespace {

enum { COUNT_TEMPLATES = 0, COUNT_WITHOUT_PRIMARY = 1, COUNT_ENDS = 2, COUNT_BLOCKS = 3, COUNT_WORDS = 4 }; // 64-bit words

__global__ void __launch_bounds__(BLOCK) genecount_name_kernel(const uint8_t* __restrict__ stream, uint64_t stream_size, const uint64_t* __restrict__ record_offset, uint64_t n, uint64_t first, unsigned long long* table, uint64_t slots,
		uint32_t hash_bits, uint32_t* name_id, uint32_t* slot_first) {
	const uint64_t r = first + (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (r >= n) return;
	uint32_t id = MDUP_NONE;
	const uint64_t at = record_offset[r];
	if (at + 36 <= stream_size) {
		id = mdup_name_insert(table, slots, stream, stream_size, record_offset, (uint32_t) r, hash_bits);
		const uint32_t flags = sbam_load16(stream, at + 18);
		if (id != MDUP_NONE && mdup_primary(flags)) atomicMin(&slot_first[2ull * id + mdup_slot(flags)], (uint32_t) r);
	}
	name_id[r] = id;
}

// Record t is a template if it is the id of its own name.  No lane leaves before the sums over the wavefront.  LEADER: the lanes that hold one gene merge their add.
template <bool LEADER> __global__ void __launch_bounds__(BLOCK) genecount_assign_kernel(GcountInput in, const uint32_t* __restrict__ name_id, const uint32_t* __restrict__ slot_first, uint64_t n, uint64_t first,
		unsigned long long* counts, unsigned long long* counters) {
	const uint64_t t = first + (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t stride = (uint64_t) in.ann.n_genes + GCOUNT_SPECIAL;
	const bool is_template = t < n && name_id[t] == (uint32_t) t;
	GcountTemplate mine;
	mine.counted = false; mine.ends = 0; mine.blocks = 0;
	for (int c = 0; c < GCOUNT_COLUMNS; ++c) mine.row[c] = GCOUNT_UNMAPPED;
	if (is_template) mine = gcount_template(in, slot_first[2 * t], slot_first[2 * t + 1]);
	// the statistics: templates and templates without a primary record in one word, ends and blocks in another (a wavefront adds less than 2^32 to either half)
	const unsigned long long templates = wave_sum((is_template ? 1ull : 0ull) | (is_template && !mine.counted ? 1ull << 32 : 0ull));
	const unsigned long long walked = wave_sum((unsigned long long) mine.ends | (unsigned long long) mine.blocks << 32);
	if (lane == 0) {
		if (templates & 0xFFFFFFFFull) atomicAdd(&counters[COUNT_TEMPLATES], templates & 0xFFFFFFFFull);
		if (templates >> 32) atomicAdd(&counters[COUNT_WITHOUT_PRIMARY], templates >> 32);
		if (walked & 0xFFFFFFFFull) atomicAdd(&counters[COUNT_ENDS], walked & 0xFFFFFFFFull);
		if (walked >> 32) atomicAdd(&counters[COUNT_BLOCKS], walked >> 32);
	}
	for (int c = 0; c < GCOUNT_COLUMNS; ++c) {
		const uint32_t row = mine.row[c];
		// the four special rows: 16 bits each of one word (a wavefront adds at most 64 to a field)
		const unsigned long long special = wave_sum(mine.counted && row < GCOUNT_SPECIAL ? 1ull << (16 * row) : 0ull);
		if (lane == 0) for (uint32_t k = 0; k < GCOUNT_SPECIAL; ++k) { const unsigned long long add = (special >> (16 * k)) & 0xFFFFull; if (add != 0) atomicAdd(&counts[c * stride + k], add); }
		const bool gene_row = mine.counted && row >= GCOUNT_SPECIAL; // (row < stride: gcount_fold admits genes < n_genes only)
		if (LEADER) {
			unsigned long long todo = __ballot(gene_row);
			while (todo != 0) { // (todo is the same in every lane)
				const int leader = __ffsll((long long) todo) - 1;
				const uint32_t theirs = __shfl(row, leader);
				const unsigned long long same = __ballot(gene_row && row == theirs);
				if (lane == (uint32_t) leader) atomicAdd(&counts[c * stride + theirs], (unsigned long long) __popcll(same));
				todo &= ~same;
			}
		} else if (gene_row) atomicAdd(&counts[c * stride + row], 1ull);
	}
}

bool plain_atomics_knob() { const char* knob = getenv("ARRIBA_GENECOUNT_PLAIN_ATOMICS"); return knob != nullptr && knob[0] == '1'; } // (for the measurement of DESIGN.md 4.15: one atomic per lane)

int count(agpu_ctx* ctx, const ResidentStream& resident, const uint32_t* ref_length, uint32_t n_ref, uint64_t* counts_out, hipEvent_t* events) {
	GenecountState& state = ctx->genecount;
	hipStream_t s = ctx->stream;
	const uint64_t size = resident.stream_size, n = resident.records;
	const uint64_t stride = (uint64_t) ctx->annotation.n_genes + GCOUNT_SPECIAL, words = GCOUNT_COLUMNS * stride;
	DeviceBuffer& counts = state.buffer("genecount.counts"); DeviceBuffer& counters = state.buffer("genecount.counters");
	ALLOC(counts, words * 8); ALLOC(counters, COUNT_WORDS * 8);
	HIP_CHECK(hipMemsetAsync(counts.ptr, 0, words * 8, s));
	HIP_CHECK(hipMemsetAsync(counters.ptr, 0, COUNT_WORDS * 8, s));
	for (int k = 0; k < 3; ++k) if (n == 0) HIP_CHECK(hipEventRecord(events[k], s));
	if (n > 0) {
		DeviceBuffer& name_id = state.buffer("genecount.name_id"); DeviceBuffer& slot_first = state.buffer("genecount.slot_first"); DeviceBuffer& table = state.buffer("genecount.table"); DeviceBuffer& lengths = state.buffer("genecount.ref_length");
		const uint64_t slots = support_table_slots(n);
		ALLOC(name_id, n * 4); ALLOC(slot_first, n * 8); ALLOC(table, slots * 8); ALLOC(lengths, std::max<size_t>(n_ref, 1) * 4);
		state.stats.peak_bytes = state.allocated();
		if (n_ref > 0) { HIP_CHECK(hipMemcpyAsync(lengths.ptr, ref_length, (size_t) n_ref * 4, hipMemcpyHostToDevice, s)); HIP_CHECK(hipStreamSynchronize(s)); } // (the source is pageable memory of the caller)
		HIP_CHECK(hipMemsetAsync(slot_first.ptr, 0xFF, n * 8, s));
		HIP_CHECK(hipMemsetAsync(table.ptr, 0, slots * 8, s));
		const uint8_t* stream = resident.stream;
		const uint64_t* record_offset = resident.record_offset;
		HIP_CHECK(hipEventRecord(events[0], s));
		{ KernelTimer timer(ctx, "genecount_name_kernel", n * 64 + slots * 8);
		  for_each_launch_piece(n, [&](uint64_t first, unsigned int grid) {
			genecount_name_kernel<<<grid, BLOCK, 0, s>>>(stream, size, record_offset, n, first, table.as<unsigned long long>(), slots, hash_bits_knob("ARRIBA_GENECOUNT_HASH_BITS"), name_id.as<uint32_t>(), slot_first.as<uint32_t>()); }); }
		HIP_CHECK(hipEventRecord(events[1], s));
		GcountInput in;
		in.stream = stream; in.stream_size = size; in.record_offset = record_offset; in.ann = ctx->annotation;
		in.tid_to_contig = ctx->ingest_tid_to_contig.as<uint32_t>(); in.ref_length = lengths.as<uint32_t>(); in.n_ref = n_ref;
		const bool plain = plain_atomics_knob();
		{ KernelTimer timer(ctx, "genecount_assign_kernel", n * 8 + n * 64);
		  for_each_launch_piece(n, [&](uint64_t first, unsigned int grid) {
			if (plain) genecount_assign_kernel<false><<<grid, BLOCK, 0, s>>>(in, name_id.as<uint32_t>(), slot_first.as<uint32_t>(), n, first, counts.as<unsigned long long>(), counters.as<unsigned long long>());
			else genecount_assign_kernel<true><<<grid, BLOCK, 0, s>>>(in, name_id.as<uint32_t>(), slot_first.as<uint32_t>(), n, first, counts.as<unsigned long long>(), counters.as<unsigned long long>());
		  }); }
		HIP_CHECK(hipEventRecord(events[2], s));
	}
	unsigned long long host_counters[COUNT_WORDS] = {};
	static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the counts are copied as they are");
	HIP_CHECK(hipMemcpyAsync(host_counters, counters.ptr, sizeof(host_counters), hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipMemcpyAsync(counts_out, counts.ptr, words * 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	state.stats.peak_bytes = std::max<uint64_t>(state.stats.peak_bytes, state.allocated());
	state.stats.records = n; state.stats.templates = host_counters[COUNT_TEMPLATES]; state.stats.without_primary = host_counters[COUNT_WITHOUT_PRIMARY];
	state.stats.ends = host_counters[COUNT_ENDS]; state.stats.blocks = host_counters[COUNT_BLOCKS];
	for (int k = 0; k < 2; ++k) { float ms = 0; if (hipEventElapsedTime(&ms, events[k], events[k + 1]) == hipSuccess) state.stats.seconds[k] = ms / 1000.0; }
	return AGPU_OK;
}

}

extern "C" {

int agpu_gene_counts(agpu_ctx* ctx, const uint32_t* ref_length, uint32_t n_ref, uint64_t* counts, agpu_gene_count_stats* stats) {
	if (!ctx || !counts || (n_ref > 0 && !ref_length)) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	if (stats) memset(stats, 0, sizeof(*stats));
	ResidentStream resident;
	TRY(resident_stream(ctx, "agpu_gene_counts", "gene counts of one sample over several GPUs are not supported", nullptr, resident, NEEDS_ANNOTATION | NEEDS_REFERENCES, n_ref));
	HIP_CHECK(hipSetDevice(ctx->device));
	GenecountState& state = ctx->genecount;
	memset(&state.stats, 0, sizeof(state.stats));
	TRY(one_shot<3>(ctx, state, "agpu_gene_counts", [&](hipEvent_t* events) { return count(ctx, resident, ref_length, n_ref, counts, events); }, [&](int) { state.release_all(); }));
	if (stats) *stats = state.stats;
	return AGPU_OK;
}

int agpu_gene_counts_allocated_bytes(agpu_ctx* ctx, uint64_t* bytes) {
	if (!ctx || !bytes) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	*bytes = ctx->genecount.allocated();
	return AGPU_OK;
}

}
