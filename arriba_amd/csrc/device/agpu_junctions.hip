// arriba_amd/csrc/device/agpu_junctions.hip -- --splice-junctions on the MI355X: the splice junctions of the record stream of the last ingest, the rows of STAR's SJ.out.tab
// (include/arriba_gpu.h: agpu_splice_junctions).  What decides a field is junction_core.hpp, which the host steps as well (arriba_amd/csrc/host/splice_junctions.cpp); the rule is
// DESIGN.md 4.16.  Here are
//   junction_count_kernel     one lane per record through ingest.record_offset: whether it contributes and how many introns of its CIGAR are kept; a rocPRIM exclusive scan over
//                             the counts gives every record its place among the crossings and their exact total: nothing is sized by guess
//   junction_name_kernel      one lane per record: its QNAME into the open-addressing table of markdup_core.hpp, the id of its template (only if there is a crossing at all)
//   junction_emit_kernel      the same walk again: per kept intron the two key words (reference, s) and (e, template, unique bit) and the overhang
//   rocPRIM radix sorts       stable, the low word first: crossings by (reference, s, e, template, unique bit); junction_gather_kernel between the passes
//   junction_head_kernel      heads of junction runs by neighbour compares -> 0 / 1, whose inclusive scan numbers the rows
//   junction_reduce_kernel    one lane per crossing: the head of a (junction, template) run counts once, as multimapping if its unique bit is clear (a multimapping crossing of a
//                             pair sorts in front of its unique ones); a segmented scan over the wavefront sums the two counts and takes the maximum overhang per row, and the last
//                             lane of every segment adds them to the row -- one atomic per wavefront, row and column, however many templates cross a junction
//   junction_intron_kernel    one lane per exon: the intron between it and its next exon as a key with the strand of its gene; sorted by the same two passes
//   junction_class_kernel     one lane per row: four bytes of the assembly for the motif, a binary search among the annotated introns, the strand
// Counters are unsigned integers, sums and maxima commute, and template ids enter only through equality: the rows are the same under every schedule.  The stream is only read.
// Integer work bound by dependent loads (record_offset -> the head of the record -> its CIGAR and aux bytes) and by the sorts; no MFMA, no LDS.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <rocprim/rocprim.hpp>
#define AGPU_OPTION "--splice-junctions"
#define ALLOC(buffer, bytes) AGPU_ALLOC(buffer, bytes, state.note_peak())
#include "resident_stream.hpp"
#include "device_utils.hpp"
#include "junction_core.hpp"

using namespace agpu;

namespace {

enum { COUNT_CONTRIBUTING = 0, COUNT_PAIRS = 1, COUNT_ANNOTATED = 2, COUNT_WORDS = 4 }; // 64-bit words
enum { PASS_COUNT = 0, PASS_NAMES = 1, PASS_EMIT = 2, PASS_ORDER = 3, PASS_CLASS = 4, PASSES = 5 };

// No lane leaves before it.
__device__ __forceinline__ void wave_count(unsigned long long* counter, unsigned int mine) {
	const unsigned int sum = wave_sum(mine);
	if ((threadIdx.x & 63u) == 0 && sum != 0) atomicAdd(counter, (unsigned long long) sum);
}

struct JuncNothing { AGPU_HD void operator()(int32_t, int32_t, uint32_t) {} };

__global__ void __launch_bounds__(BLOCK) junction_count_kernel(const uint8_t* __restrict__ stream, uint64_t stream_size, const uint64_t* __restrict__ record_offset, uint64_t n, uint64_t first, const uint32_t* __restrict__ ref_length,
		uint32_t n_ref, uint32_t* kept, unsigned long long* counters) {
	const uint64_t r = first + (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	unsigned int contributes = 0;
	if (r < n) {
		JuncRecord record;
		uint32_t count = 0;
		if (junc_record(stream, stream_size, record_offset, r, n_ref, record)) {
			contributes = 1;
			JuncNothing nothing;
			count = junc_walk(stream, record.cigar_at, record.n_cigar, record.pos, ref_length[record.ref], nothing);
		}
		kept[r] = count;
	}
	wave_count(&counters[COUNT_CONTRIBUTING], contributes);
}

__global__ void __launch_bounds__(BLOCK) junction_name_kernel(const uint8_t* __restrict__ stream, uint64_t stream_size, const uint64_t* __restrict__ record_offset, uint64_t n, uint64_t first, unsigned long long* table, uint64_t slots,
		uint32_t hash_bits, uint32_t* name_id) {
	const uint64_t r = first + (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (r >= n) return;
	uint32_t id = MDUP_NONE;
	if (record_offset[r] + 36 <= stream_size) id = mdup_name_insert(table, slots, stream, stream_size, record_offset, (uint32_t) r, hash_bits);
	name_id[r] = id != MDUP_NONE ? id : (uint32_t) r; // (a record without a name is a template of its own)
}

// the crossings of a record go to [begin, begin + room) of the three arrays
struct JuncEmit {
	uint64_t* high; uint64_t* low; uint32_t* overhang; uint64_t begin; uint32_t room, written; uint32_t ref, name; bool multimapping;
	AGPU_HD void operator()(int32_t s, int32_t e, uint32_t least) {
		if (written < room) { high[begin + written] = junc_key_high(ref, s); low[begin + written] = junc_key_low(e, name, multimapping); overhang[begin + written] = least; }
		++written;
	}
};

__global__ void __launch_bounds__(BLOCK) junction_emit_kernel(const uint8_t* __restrict__ stream, uint64_t stream_size, const uint64_t* __restrict__ record_offset, uint64_t n, uint64_t first, const uint32_t* __restrict__ ref_length,
		uint32_t n_ref, const uint32_t* __restrict__ kept, const uint64_t* __restrict__ place, const uint32_t* __restrict__ name_id, uint64_t* high, uint64_t* low, uint32_t* overhang) {
	const uint64_t r = first + (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (r >= n || kept[r] == 0) return;
	JuncRecord record;
	if (!junc_record(stream, stream_size, record_offset, r, n_ref, record)) return;
	JuncEmit emit = { high, low, overhang, place[r], kept[r], 0, record.ref, name_id[r], record.multimapping };
	junc_walk(stream, record.cigar_at, record.n_cigar, record.pos, ref_length[record.ref], emit);
}

__global__ void __launch_bounds__(BLOCK) junction_identity_kernel(uint32_t* order, uint64_t count) {
	const uint64_t i = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (i < count) order[i] = (uint32_t) i;
}
__global__ void __launch_bounds__(BLOCK) junction_gather_kernel(const uint64_t* __restrict__ words, const uint32_t* __restrict__ order, uint64_t count, uint64_t* out) {
	const uint64_t i = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (i < count) out[i] = words[order[i]];
}
__global__ void __launch_bounds__(BLOCK) junction_gather32_kernel(const uint32_t* __restrict__ words, const uint32_t* __restrict__ order, uint64_t count, uint32_t* out) {
	const uint64_t i = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (i < count) out[i] = words[order[i]];
}

// high, low: the crossings in their order.  head[i] = 1 where a junction begins
__global__ void __launch_bounds__(BLOCK) junction_head_kernel(const uint64_t* __restrict__ high, const uint64_t* __restrict__ low, uint64_t count, uint32_t* head) {
	const uint64_t i = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (i >= count) return;
	head[i] = i == 0 || !junc_same_junction(high[i], low[i], high[i - 1], low[i - 1]) ? 1u : 0u;
}

struct JuncRows { uint64_t* high; uint32_t* end; uint32_t* unique; uint32_t* multimapping; uint32_t* overhang; };

// row_of[i]: the inclusive scan of head, so crossing i belongs to row row_of[i] - 1.  No lane leaves before the scans over the wavefront.
__global__ void __launch_bounds__(BLOCK) junction_reduce_kernel(const uint64_t* __restrict__ high, const uint64_t* __restrict__ low, const uint32_t* __restrict__ overhang, const uint32_t* __restrict__ row_of, uint64_t count,
		uint64_t first, JuncRows rows, unsigned long long* counters) {
	const uint64_t i = first + (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	const uint32_t lane = threadIdx.x & 63u;
	const bool live = i < count;
	uint32_t row = 0xFFFFFFFFu, unique = 0, multimapping = 0, longest = 0;
	bool junction_head = false;
	if (live) {
		const uint64_t h = high[i], l = low[i];
		row = row_of[i] - 1u;
		longest = overhang[i];
		bool pair_head = true;
		junction_head = true;
		if (i > 0) { const uint64_t ph = high[i - 1], pl = low[i - 1]; pair_head = !junc_same_pair(h, l, ph, pl); junction_head = !junc_same_junction(h, l, ph, pl); }
		if (pair_head) { if (junc_key_multimapping(l)) multimapping = 1; else unique = 1; }
		if (junction_head) { rows.high[row] = h; rows.end[row] = (uint32_t) junc_key_e(l); }
	}
	wave_count(&counters[COUNT_PAIRS], unique + multimapping);
	// the lanes of one row are neighbours: an inclusive scan that stops at the first lane of the row
	for (int offset = 1; offset < 64; offset <<= 1) {
		const uint32_t their_row = __shfl_up(row, offset), their_unique = __shfl_up(unique, offset), their_multimapping = __shfl_up(multimapping, offset), their_longest = __shfl_up(longest, offset);
		if (lane >= (uint32_t) offset && their_row == row) { unique += their_unique; multimapping += their_multimapping; longest = longest > their_longest ? longest : their_longest; }
	}
	const uint32_t next_row = __shfl_down(row, 1);
	if (live && (lane == 63u || next_row != row)) { // the last lane of its row in this wavefront
		if (unique != 0) atomicAdd(&rows.unique[row], unique);
		if (multimapping != 0) atomicAdd(&rows.multimapping[row], multimapping);
		atomicMax(&rows.overhang[row], longest);
	}
}

__global__ void __launch_bounds__(BLOCK) junction_intron_kernel(AnnotationView ann, uint64_t* high, uint64_t* low, uint32_t* mask) {
	const uint32_t x = blockIdx.x * BLOCK + threadIdx.x;
	if (x >= ann.n_exons) return;
	uint64_t l; uint32_t m;
	high[x] = junc_intron_key_high(ann, x, l, m);
	low[x] = l; mask[x] = m;
}

__global__ void __launch_bounds__(BLOCK) junction_class_kernel(JuncRows rows, uint64_t n_rows, const uint32_t* __restrict__ tid_to_contig, GenomeView genome, JuncIntrons introns, agpu_junction_row* out, unsigned long long* counters) {
	const uint64_t j = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	unsigned int annotated = 0;
	if (j < n_rows) {
		const uint64_t high = rows.high[j];
		const uint32_t ref = junc_key_ref(high), contig = tid_to_contig[ref];
		const int32_t s = junc_key_s(high), e = (int32_t) rows.end[j];
		const uint32_t motif = junc_motif(genome, contig, s, e), seen = junc_annotated(introns, contig, s, e);
		annotated = seen != 0 ? 1u : 0u;
		agpu_junction_row row;
		row.ref = ref; row.start = s; row.end = e; row.strand = (uint8_t) junc_strand(motif, seen); row.motif = (uint8_t) motif; row.annotated = (uint8_t) annotated; row.reserved = 0;
		row.unique = rows.unique[j]; row.multimapping = rows.multimapping[j]; row.overhang = rows.overhang[j];
		out[j] = row;
	}
	wave_count(&counters[COUNT_ANNOTATED], annotated);
}

// `count` < 2^32 items ordered by (high, low): a stable radix sort by the low word, then one by the high word gathered in that order.  order_out: the items in their order;
// sorted_high_out: the high words in that order.  Both point into "junction.order*" / "junction.sort_out" of the state.
int sort_by_two_words(agpu_ctx* ctx, const uint64_t* low, const uint64_t* high, unsigned int high_bits, uint64_t count, const char* what, const uint32_t*& order_out, const uint64_t*& sorted_high_out) {
	JunctionState& state = ctx->junction;
	hipStream_t s = ctx->stream;
	DeviceBuffer& gathered = state.buffer("junction.sort_in"); DeviceBuffer& sorted = state.buffer("junction.sort_out"); DeviceBuffer& temporary_storage = state.buffer("junction.rocprim");
	DeviceBuffer& order0 = state.buffer("junction.order0"); DeviceBuffer& order1 = state.buffer("junction.order1");
	ALLOC(gathered, count * 8); ALLOC(sorted, count * 8); ALLOC(order0, count * 4); ALLOC(order1, count * 4);
	{ KernelTimer timer(ctx, "junction_identity_kernel", count * 4);
	  junction_identity_kernel<<<grid_for(count), BLOCK, 0, s>>>(order0.as<uint32_t>(), count); }
	size_t temporary = 0;
	HIP_CHECK(rocprim::radix_sort_pairs(nullptr, temporary, low, sorted.as<uint64_t>(), order0.as<uint32_t>(), order1.as<uint32_t>(), (size_t) count, 0u, 64u, s));
	if (temporary > temporary_storage.capacity) { HIP_CHECK(hipStreamSynchronize(s)); ALLOC(temporary_storage, temporary); }
	{ KernelTimer timer(ctx, what, count * 24);
	  HIP_CHECK(rocprim::radix_sort_pairs(temporary_storage.ptr, temporary, low, sorted.as<uint64_t>(), order0.as<uint32_t>(), order1.as<uint32_t>(), (size_t) count, 0u, 64u, s)); }
	{ KernelTimer timer(ctx, "junction_gather_kernel", count * 20);
	  junction_gather_kernel<<<grid_for(count), BLOCK, 0, s>>>(high, order1.as<uint32_t>(), count, gathered.as<uint64_t>()); }
	HIP_CHECK(rocprim::radix_sort_pairs(nullptr, temporary, gathered.as<uint64_t>(), sorted.as<uint64_t>(), order1.as<uint32_t>(), order0.as<uint32_t>(), (size_t) count, 0u, high_bits, s));
	if (temporary > temporary_storage.capacity) { HIP_CHECK(hipStreamSynchronize(s)); ALLOC(temporary_storage, temporary); }
	{ KernelTimer timer(ctx, what, count * 24);
	  HIP_CHECK(rocprim::radix_sort_pairs(temporary_storage.ptr, temporary, gathered.as<uint64_t>(), sorted.as<uint64_t>(), order1.as<uint32_t>(), order0.as<uint32_t>(), (size_t) count, 0u, high_bits, s)); }
	order_out = order0.as<uint32_t>(); sorted_high_out = sorted.as<uint64_t>();
	return AGPU_OK;
}

int find(agpu_ctx* ctx, const ResidentStream& resident, const uint32_t* ref_length, uint32_t n_ref, hipEvent_t* events) {
	JunctionState& state = ctx->junction;
	hipStream_t s = ctx->stream;
	const uint64_t size = resident.stream_size, n = resident.records;
	state.stats.records = n;
	if (n == 0) { for (int k = 0; k <= PASSES; ++k) HIP_CHECK(hipEventRecord(events[k], s)); return AGPU_OK; }
	const uint8_t* stream = resident.stream;
	const uint64_t* record_offset = resident.record_offset;
	const uint32_t* tid_to_contig = ctx->ingest_tid_to_contig.as<uint32_t>();
	DeviceBuffer& counters = state.buffer("junction.counters"); DeviceBuffer& lengths = state.buffer("junction.ref_length"); DeviceBuffer& kept = state.buffer("junction.kept"); DeviceBuffer& place = state.buffer("junction.place");
	DeviceBuffer& temporary_storage = state.buffer("junction.rocprim");
	ALLOC(counters, COUNT_WORDS * 8); ALLOC(lengths, std::max<size_t>(n_ref, 1) * 4); ALLOC(kept, (n + 1) * 4); ALLOC(place, (n + 1) * 8);
	HIP_CHECK(hipMemsetAsync(counters.ptr, 0, COUNT_WORDS * 8, s));
	HIP_CHECK(hipMemsetAsync(kept.as<uint32_t>() + n, 0, 4, s)); // (the scan runs over n + 1 counts: the last place is the total)
	if (n_ref > 0) { HIP_CHECK(hipMemcpyAsync(lengths.ptr, ref_length, (size_t) n_ref * 4, hipMemcpyHostToDevice, s)); HIP_CHECK(hipStreamSynchronize(s)); } // (the source is pageable memory of the caller)
	// count and offsets
	HIP_CHECK(hipEventRecord(events[0], s));
	{ KernelTimer timer(ctx, "junction_count_kernel", n * 72);
	  for_each_launch_piece(n, [&](uint64_t first, unsigned int grid) {
		junction_count_kernel<<<grid, BLOCK, 0, s>>>(stream, size, record_offset, n, first, lengths.as<uint32_t>(), n_ref, kept.as<uint32_t>(), counters.as<unsigned long long>()); }); }
	{ size_t temporary = 0;
	  HIP_CHECK(rocprim::exclusive_scan(nullptr, temporary, kept.as<uint32_t>(), place.as<uint64_t>(), (uint64_t) 0, (size_t) (n + 1), rocprim::plus<uint64_t>(), s));
	  if (temporary > temporary_storage.capacity) ALLOC(temporary_storage, temporary);
	  KernelTimer timer(ctx, "junction rocprim::exclusive_scan(kept)", n * 12);
	  HIP_CHECK(rocprim::exclusive_scan(temporary_storage.ptr, temporary, kept.as<uint32_t>(), place.as<uint64_t>(), (uint64_t) 0, (size_t) (n + 1), rocprim::plus<uint64_t>(), s)); }
	HIP_CHECK(hipEventRecord(events[1], s));
	uint64_t crossings = 0;
	unsigned long long host_counters[COUNT_WORDS] = {};
	HIP_CHECK(hipMemcpyAsync(&crossings, place.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipMemcpyAsync(host_counters, counters.ptr, sizeof(host_counters), hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	state.stats.contributing = host_counters[COUNT_CONTRIBUTING]; state.stats.crossings = crossings;
	if (crossings == 0) { for (int k = 2; k <= PASSES; ++k) HIP_CHECK(hipEventRecord(events[k], s)); return AGPU_OK; } // (no name table, no tuple)
	if (crossings >= 0xFFFFFFF0ull) { set_last_error("agpu_splice_junctions: more than 2^32-16 crossings of splice junctions"); return AGPU_ERR_INVALID; }
	// name ids
	DeviceBuffer& name_id = state.buffer("junction.name_id");
	{ DeviceBuffer& table = state.buffer("junction.table");
	  const uint64_t slots = support_table_slots(n);
	  ALLOC(name_id, n * 4); ALLOC(table, slots * 8);
	  HIP_CHECK(hipMemsetAsync(table.ptr, 0, slots * 8, s));
	  { KernelTimer timer(ctx, "junction_name_kernel", n * 64 + slots * 8);
	    for_each_launch_piece(n, [&](uint64_t first, unsigned int grid) {
		junction_name_kernel<<<grid, BLOCK, 0, s>>>(stream, size, record_offset, n, first, table.as<unsigned long long>(), slots, hash_bits_knob("ARRIBA_JUNCTION_HASH_BITS"), name_id.as<uint32_t>()); }); }
	  HIP_CHECK(hipEventRecord(events[2], s));
	  HIP_CHECK(hipStreamSynchronize(s));
	  table.release(); }
	// emit
	DeviceBuffer& key_high = state.buffer("junction.key_high"); DeviceBuffer& key_low = state.buffer("junction.key_low"); DeviceBuffer& overhang = state.buffer("junction.overhang");
	ALLOC(key_high, crossings * 8); ALLOC(key_low, crossings * 8); ALLOC(overhang, crossings * 4);
	{ KernelTimer timer(ctx, "junction_emit_kernel", n * 84 + crossings * 20);
	  for_each_launch_piece(n, [&](uint64_t first, unsigned int grid) {
		junction_emit_kernel<<<grid, BLOCK, 0, s>>>(stream, size, record_offset, n, first, lengths.as<uint32_t>(), n_ref, kept.as<uint32_t>(), place.as<uint64_t>(), name_id.as<uint32_t>(), key_high.as<uint64_t>(), key_low.as<uint64_t>(),
		                                            overhang.as<uint32_t>()); }); }
	HIP_CHECK(hipEventRecord(events[3], s));
	HIP_CHECK(hipStreamSynchronize(s));
	kept.release(); place.release(); name_id.release();
	// order and reduce
	const uint32_t* order = nullptr; const uint64_t* sorted_high = nullptr;
	TRY(sort_by_two_words(ctx, key_low.as<uint64_t>(), key_high.as<uint64_t>(), 32 + bits_of(n_ref), crossings, "junction rocprim::radix_sort_pairs(crossings)", order, sorted_high));
	// (the low words and the overhangs in that order: into the buffers the sort is done with)
	DeviceBuffer& sorted_low = state.buffer("junction.sort_in"); DeviceBuffer& sorted_overhang = state.buffer("junction.order1"); DeviceBuffer& head = state.buffer("junction.head"); DeviceBuffer& row_of = state.buffer("junction.row_of");
	ALLOC(head, crossings * 4); ALLOC(row_of, crossings * 4);
	{ KernelTimer timer(ctx, "junction_gather_kernel", crossings * 32);
	  junction_gather_kernel<<<grid_for(crossings), BLOCK, 0, s>>>(key_low.as<uint64_t>(), order, crossings, sorted_low.as<uint64_t>());
	  junction_gather32_kernel<<<grid_for(crossings), BLOCK, 0, s>>>(overhang.as<uint32_t>(), order, crossings, sorted_overhang.as<uint32_t>()); }
	{ KernelTimer timer(ctx, "junction_head_kernel", crossings * 20);
	  junction_head_kernel<<<grid_for(crossings), BLOCK, 0, s>>>(sorted_high, sorted_low.as<uint64_t>(), crossings, head.as<uint32_t>()); }
	{ size_t temporary = 0;
	  HIP_CHECK(rocprim::inclusive_scan(nullptr, temporary, head.as<uint32_t>(), row_of.as<uint32_t>(), (size_t) crossings, rocprim::plus<uint32_t>(), s));
	  if (temporary > temporary_storage.capacity) { HIP_CHECK(hipStreamSynchronize(s)); ALLOC(temporary_storage, temporary); }
	  KernelTimer timer(ctx, "junction rocprim::inclusive_scan(heads)", crossings * 8);
	  HIP_CHECK(rocprim::inclusive_scan(temporary_storage.ptr, temporary, head.as<uint32_t>(), row_of.as<uint32_t>(), (size_t) crossings, rocprim::plus<uint32_t>(), s)); }
	uint32_t n_rows32 = 0;
	HIP_CHECK(hipMemcpyAsync(&n_rows32, row_of.as<uint32_t>() + (crossings - 1), 4, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	const uint64_t n_rows = n_rows32;
	if (n_rows == 0 || n_rows > crossings) { set_last_error("--splice-junctions: the heads of the junction runs do not add up"); return AGPU_ERR_DEVICE; }
	key_high.release(); key_low.release(); overhang.release(); head.release();
	DeviceBuffer& row_high = state.buffer("junction.row_high"); DeviceBuffer& row_end = state.buffer("junction.row_end"); DeviceBuffer& row_counts = state.buffer("junction.row_counts"); DeviceBuffer& out = state.buffer("junction.rows");
	ALLOC(row_high, n_rows * 8); ALLOC(row_end, n_rows * 4); ALLOC(row_counts, n_rows * 12); ALLOC(out, n_rows * sizeof(agpu_junction_row));
	HIP_CHECK(hipMemsetAsync(row_counts.ptr, 0, n_rows * 12, s));
	const JuncRows rows = { row_high.as<uint64_t>(), row_end.as<uint32_t>(), row_counts.as<uint32_t>(), row_counts.as<uint32_t>() + n_rows, row_counts.as<uint32_t>() + 2 * n_rows };
	{ KernelTimer timer(ctx, "junction_reduce_kernel", crossings * 24);
	  for_each_launch_piece(crossings, [&](uint64_t first, unsigned int grid) {
		junction_reduce_kernel<<<grid, BLOCK, 0, s>>>(sorted_high, sorted_low.as<uint64_t>(), sorted_overhang.as<uint32_t>(), row_of.as<uint32_t>(), crossings, first, rows, counters.as<unsigned long long>()); }); }
	HIP_CHECK(hipEventRecord(events[4], s));
	HIP_CHECK(hipStreamSynchronize(s));
	row_of.release();
	// annotated introns and classes
	const uint64_t n_exons = ctx->annotation.n_exons;
	JuncIntrons introns = { nullptr, nullptr, nullptr, 0 };
	if (n_exons > 0) {
		DeviceBuffer& intron_high = state.buffer("junction.intron_high"); DeviceBuffer& intron_low = state.buffer("junction.intron_low"); DeviceBuffer& intron_mask = state.buffer("junction.intron_mask");
		DeviceBuffer& sorted_intron_low = state.buffer("junction.sorted_intron_low"); DeviceBuffer& sorted_intron_mask = state.buffer("junction.sorted_intron_mask");
		ALLOC(intron_high, n_exons * 8); ALLOC(intron_low, n_exons * 8); ALLOC(intron_mask, n_exons * 4); ALLOC(sorted_intron_low, n_exons * 8); ALLOC(sorted_intron_mask, n_exons * 4);
		{ KernelTimer timer(ctx, "junction_intron_kernel", n_exons * 36);
		  junction_intron_kernel<<<grid_for(n_exons), BLOCK, 0, s>>>(ctx->annotation, intron_high.as<uint64_t>(), intron_low.as<uint64_t>(), intron_mask.as<uint32_t>()); }
		const uint32_t* intron_order = nullptr; const uint64_t* sorted_intron_high = nullptr;
		TRY(sort_by_two_words(ctx, intron_low.as<uint64_t>(), intron_high.as<uint64_t>(), 64, n_exons, "junction rocprim::radix_sort_pairs(introns)", intron_order, sorted_intron_high));
		{ KernelTimer timer(ctx, "junction_gather_kernel", n_exons * 32);
		  junction_gather_kernel<<<grid_for(n_exons), BLOCK, 0, s>>>(intron_low.as<uint64_t>(), intron_order, n_exons, sorted_intron_low.as<uint64_t>());
		  junction_gather32_kernel<<<grid_for(n_exons), BLOCK, 0, s>>>(intron_mask.as<uint32_t>(), intron_order, n_exons, sorted_intron_mask.as<uint32_t>()); }
		introns.high = sorted_intron_high; introns.low = sorted_intron_low.as<uint64_t>(); introns.mask = sorted_intron_mask.as<uint32_t>(); introns.n = n_exons;
	}
	{ KernelTimer timer(ctx, "junction_class_kernel", n_rows * 80);
	  junction_class_kernel<<<grid_for(n_rows), BLOCK, 0, s>>>(rows, n_rows, tid_to_contig, ctx->genome, introns, out.as<agpu_junction_row>(), counters.as<unsigned long long>()); }
	HIP_CHECK(hipEventRecord(events[5], s));
	state.rows.resize(n_rows);
	HIP_CHECK(hipMemcpyAsync(state.rows.data(), out.ptr, n_rows * sizeof(agpu_junction_row), hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipMemcpyAsync(host_counters, counters.ptr, sizeof(host_counters), hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	state.stats.pairs = host_counters[COUNT_PAIRS]; state.stats.junctions = n_rows; state.stats.annotated = host_counters[COUNT_ANNOTATED];
	return AGPU_OK;
}

}

extern "C" {

int agpu_splice_junctions(agpu_ctx* ctx, const uint32_t* ref_length, uint32_t n_ref, const agpu_junction_row** rows, uint64_t* n_rows, agpu_junction_stats* stats) {
	if (!ctx || !rows || !n_rows || (n_ref > 0 && !ref_length)) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	*rows = nullptr; *n_rows = 0;
	if (stats) memset(stats, 0, sizeof(*stats));
	ResidentStream resident;
	TRY(resident_stream(ctx, "agpu_splice_junctions", "splice junctions of one sample over several GPUs are not supported", nullptr, resident, NEEDS_ANNOTATION | NEEDS_GENOME | NEEDS_REFERENCES, n_ref));
	HIP_CHECK(hipSetDevice(ctx->device));
	JunctionState& state = ctx->junction;
	memset(&state.stats, 0, sizeof(state.stats));
	state.rows.clear(); state.peak = 0;
	const int status = one_shot<PASSES + 1>(ctx, state, "agpu_splice_junctions", [&](hipEvent_t* events) {
		const int found = find(ctx, resident, ref_length, n_ref, events);
		(void) hipStreamSynchronize(ctx->stream); // (the events of a call without crossings have happened)
		if (found == AGPU_OK) for (int k = 0; k < PASSES; ++k) { float ms = 0; if (hipEventElapsedTime(&ms, events[k], events[k + 1]) == hipSuccess) state.stats.seconds[k] = ms / 1000.0; }
		return found;
	}, [&](int) { state.stats.peak_bytes = state.peak; state.release_all(); });
	if (status != AGPU_OK) { state.rows.clear(); return status; }
	*rows = state.rows.data(); *n_rows = state.rows.size();
	if (stats) *stats = state.stats;
	return AGPU_OK;
}

int agpu_splice_junctions_allocated_bytes(agpu_ctx* ctx, uint64_t* bytes) {
	if (!ctx || !bytes) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	*bytes = ctx->junction.allocated();
	return AGPU_OK;
}

}
