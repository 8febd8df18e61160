// arriba_amd/csrc/device/agpu_alleles.hip -- --allele-counts on the MI355X: the bases the records of the last ingest show at a list of known positions
// (include/arriba_gpu.h: agpu_allele_counts).  What decides a number is allele_core.hpp, which the host steps as well (arriba_amd/csrc/host/allele_counts.cpp); the rule is
// DESIGN.md 4.17.  Here are
//   rocPRIM radix sort      the placed sites by (reference, position), each with its line: duplicate lines become neighbours
//   allele_bitmap_kernel    one lane per sorted site: the bit of its 64-base window of the concatenated references (6 MB at the size of hg38: it stays in L2 / Infinity Cache)
//   allele_count_kernel     one lane per record through ingest.record_offset: the filter, then the walk of allele_core.hpp as an iterator.  A block of the CIGAR whose windows
//                           hold no site costs one probe of the bitmap: no binary search, no SEQ and no QUAL byte.  Every step of the loop, each lane brings at most one
//                           (site slot, column); the lanes of the wavefront that bring the same one merge into one atomic add of their number (the leader loop of
//                           agpu_genecount.hip: __ballot over the distinct values), so a SNP in a highly expressed gene costs one atomic per wavefront and column, not one per read.
//                           The loop ends when no lane has a hit left; no lane leaves before that
//   allele_rows_kernel      one lane per sorted site: its eight counters into the row of its line
//   allele_ref_kernel       one lane per line: REF from the assembly through tid_to_contig, '.' for an unplaced line
// The bitmap and the count work on sorted keys that lie on the device and are shared with --variant-sites: allele_count.hpp has the two kernels and their launches.
// Counters are unsigned sums: the rows are the same under every schedule.  The stream is only read.
// Integer work bound by dependent loads: record_offset -> the head of the record -> its CIGAR words -> (only where a window holds a site) the sorted keys, one SEQ and one QUAL
// byte.  No MFMA, no LDS.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <rocprim/rocprim.hpp>
#define AGPU_OPTION "--allele-counts"
#define ALLOC(buffer, bytes) AGPU_ALLOC(buffer, bytes, state.note_peak())
#include "allele_count.hpp"

using namespace agpu;

namespace {

enum { PASS_SITES = 0, PASS_COUNT = 1, PASS_ROWS = 2, PASSES = 3 };

__global__ void __launch_bounds__(BLOCK) allele_rows_kernel(const uint32_t* __restrict__ counts, const uint32_t* __restrict__ line_of, uint64_t placed, uint64_t n_sites, agpu_allele_row* rows) {
	const uint64_t k = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (k >= placed) return;
	const uint32_t line = line_of[k];
	if (line >= n_sites) return;
	const uint32_t* mine = counts + k * ALLELE_COLUMNS;
	agpu_allele_row& row = rows[line];
	row.a = mine[ALLELE_A]; row.c = mine[ALLELE_C]; row.g = mine[ALLELE_G]; row.t = mine[ALLELE_T]; row.n = mine[ALLELE_N]; row.del = mine[ALLELE_DEL]; row.skip = mine[ALLELE_SKIP]; row.lowq = mine[ALLELE_LOWQ];
}

__global__ void __launch_bounds__(BLOCK) allele_ref_kernel(const agpu_allele_site* __restrict__ sites, uint64_t n_sites, const uint32_t* __restrict__ tid_to_contig, uint32_t n_ref, GenomeView genome, agpu_allele_row* rows) {
	const uint64_t line = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (line >= n_sites) return;
	const agpu_allele_site site = sites[line];
	rows[line].ref_base = site.ref < n_ref && site.pos >= 0 ? allele_ref_base(genome, tid_to_contig[site.ref], (uint32_t) site.pos) : (uint8_t) '.';
}

int count(agpu_ctx* ctx, const ResidentStream& resident, const agpu_allele_site* sites, uint64_t n_sites, const uint32_t* ref_length, uint32_t n_ref, uint32_t min_mapq, uint32_t min_baseq, hipEvent_t* events) {
	AlleleState& state = ctx->allele;
	hipStream_t s = ctx->stream;
	const uint64_t n = resident.records;
	state.stats.records = n; state.stats.sites = n_sites;
	// the placed sites as keys with their lines
	std::vector<uint64_t> keys; std::vector<uint32_t> lines;
	for (uint64_t line = 0; line < n_sites; ++line) {
		const agpu_allele_site& site = sites[line];
		if (site.ref == ALLELE_UNPLACED) continue;
		if (site.ref >= n_ref || site.pos < 0 || (uint32_t) site.pos >= ref_length[site.ref]) { set_last_error("agpu_allele_counts: site " + std::to_string(line) + " lies on no reference of the header or beyond its length (unplaced sites have ref 0xFFFFFFFF)"); return AGPU_ERR_INVALID; }
		keys.push_back(allele_key(site.ref, (uint32_t) site.pos)); lines.push_back((uint32_t) line);
	}
	const uint64_t placed = keys.size();
	state.stats.placed = placed;
	state.rows.assign(n_sites, agpu_allele_row());
	if (n_sites == 0 && n == 0) { for (int k = 0; k <= PASSES; ++k) HIP_CHECK(hipEventRecord(events[k], s)); return AGPU_OK; }
	DeviceBuffer& keys_in = state.buffer("allele.keys_in"); DeviceBuffer& lines_in = state.buffer("allele.lines_in"); DeviceBuffer& sorted_keys = state.buffer("allele.keys"); DeviceBuffer& sorted_lines = state.buffer("allele.lines");
	DeviceBuffer& temporary_storage = state.buffer("allele.rocprim"); DeviceBuffer& counts = state.buffer("allele.counts");
	DeviceBuffer& device_sites = state.buffer("allele.sites"); DeviceBuffer& rows = state.buffer("allele.rows");
	AlleleCounting counting = { state.buffer("allele.ref_length"), state.buffer("allele.window_offset"), state.buffer("allele.contributing"), state.buffer("allele.bitmap"), counts, 0, true };
	DeviceBuffer& contributing = counting.contributing;
	TRY(allele_counting_begin(ctx, state, counting, ref_length, n_ref, placed)); // (LN and the first window of every reference, the zeroed counters and bitmap)
	ALLOC(device_sites, std::max<size_t>(n_sites, 1) * sizeof(agpu_allele_site)); ALLOC(rows, std::max<size_t>(n_sites, 1) * sizeof(agpu_allele_row));
	HIP_CHECK(hipMemsetAsync(rows.ptr, 0, std::max<size_t>(n_sites, 1) * sizeof(agpu_allele_row), s));
	if (n_sites > 0) HIP_CHECK(hipMemcpyAsync(device_sites.ptr, sites, n_sites * sizeof(agpu_allele_site), hipMemcpyHostToDevice, s));
	if (placed > 0) {
		ALLOC(keys_in, placed * 8); ALLOC(lines_in, placed * 4); ALLOC(sorted_keys, placed * 8); ALLOC(sorted_lines, placed * 4);
		HIP_CHECK(hipMemcpyAsync(keys_in.ptr, keys.data(), placed * 8, hipMemcpyHostToDevice, s));
		HIP_CHECK(hipMemcpyAsync(lines_in.ptr, lines.data(), placed * 4, hipMemcpyHostToDevice, s));
	}
	HIP_CHECK(hipStreamSynchronize(s)); // (the sources are pageable memory of the caller and of this function)
	// sorted sites and window bitmap
	HIP_CHECK(hipEventRecord(events[PASS_SITES], s));
	if (placed > 0) {
		const unsigned int key_bits = 32 + bits_of(n_ref);
		size_t temporary = 0;
		HIP_CHECK(rocprim::radix_sort_pairs(nullptr, temporary, keys_in.as<uint64_t>(), sorted_keys.as<uint64_t>(), lines_in.as<uint32_t>(), sorted_lines.as<uint32_t>(), (size_t) placed, 0u, key_bits, s));
		ALLOC(temporary_storage, std::max<size_t>(temporary, 4));
		{ KernelTimer timer(ctx, "allele rocprim::radix_sort_pairs(sites)", placed * 24);
		  HIP_CHECK(rocprim::radix_sort_pairs(temporary_storage.ptr, temporary, keys_in.as<uint64_t>(), sorted_keys.as<uint64_t>(), lines_in.as<uint32_t>(), sorted_lines.as<uint32_t>(), (size_t) placed, 0u, key_bits, s)); }
		allele_counting_bitmap(ctx, counting, sorted_keys.as<uint64_t>(), n_ref);
	}
	// the count over the records
	HIP_CHECK(hipEventRecord(events[PASS_COUNT], s));
	allele_counting_records(ctx, counting, resident, sorted_keys.as<uint64_t>(), n_ref, min_mapq, min_baseq);
	// REF and the rows in the order of the lines
	HIP_CHECK(hipEventRecord(events[PASS_ROWS], s));
	if (placed > 0) { KernelTimer timer(ctx, "allele_rows_kernel", placed * 68);
	  allele_rows_kernel<<<grid_for(placed), BLOCK, 0, s>>>(counts.as<uint32_t>(), sorted_lines.as<uint32_t>(), placed, n_sites, rows.as<agpu_allele_row>()); }
	if (n_sites > 0) { KernelTimer timer(ctx, "allele_ref_kernel", n_sites * 16);
	  allele_ref_kernel<<<grid_for(n_sites), BLOCK, 0, s>>>(device_sites.as<agpu_allele_site>(), n_sites, ctx->ingest_tid_to_contig.as<uint32_t>(), n_ref, ctx->genome, rows.as<agpu_allele_row>()); }
	HIP_CHECK(hipEventRecord(events[PASSES], s));
	unsigned long long host_contributing = 0;
	if (n_sites > 0) HIP_CHECK(hipMemcpyAsync(state.rows.data(), rows.ptr, n_sites * sizeof(agpu_allele_row), hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipMemcpyAsync(&host_contributing, contributing.ptr, 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	state.stats.contributing = host_contributing;
	for (uint64_t line = 0; line < n_sites; ++line) {
		const agpu_allele_row& row = state.rows[line];
		const uint64_t sum = (uint64_t) row.a + row.c + row.g + row.t + row.n + row.del + row.skip + row.lowq;
		state.stats.hits += sum; if (sum != 0) ++state.stats.covered;
	}
	return AGPU_OK;
}

}

extern "C" {

int agpu_allele_counts(agpu_ctx* ctx, const agpu_allele_site* sites, uint64_t n_sites, const uint32_t* ref_length, uint32_t n_ref, uint32_t min_mapq, uint32_t min_baseq, const agpu_allele_row** rows, agpu_allele_stats* stats) {
	if (!ctx || !rows || (n_sites > 0 && !sites) || (n_ref > 0 && !ref_length)) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	*rows = nullptr;
	if (stats) memset(stats, 0, sizeof(*stats));
	if (min_mapq > 255 || min_baseq > 255) { set_last_error("agpu_allele_counts: a threshold above 255"); return AGPU_ERR_INVALID; }
	if (n_sites > ALLELE_MAX_SITES) { set_last_error("agpu_allele_counts: more than 2^29-1 sites"); return AGPU_ERR_INVALID; }
	ResidentStream resident;
	TRY(resident_stream(ctx, "agpu_allele_counts", "allele counts of one sample over several GPUs are not supported", nullptr, resident, NEEDS_GENOME | NEEDS_REFERENCES, n_ref));
	HIP_CHECK(hipSetDevice(ctx->device));
	AlleleState& state = ctx->allele;
	memset(&state.stats, 0, sizeof(state.stats));
	state.rows.clear(); state.peak = 0;
	const int status = one_shot<PASSES + 1>(ctx, state, "agpu_allele_counts", [&](hipEvent_t* events) {
		const int counted = count(ctx, resident, sites, n_sites, ref_length, n_ref, min_mapq, min_baseq, events);
		(void) hipStreamSynchronize(ctx->stream); // (the events of a call without sites and records have happened)
		if (counted == AGPU_OK) for (int k = 0; k < PASSES; ++k) { float ms = 0; if (hipEventElapsedTime(&ms, events[k], events[k + 1]) == hipSuccess) state.stats.seconds[k] = ms / 1000.0; }
		return counted;
	}, [&](int) { state.stats.peak_bytes = state.peak; state.release_all(); });
	if (status != AGPU_OK) { state.rows.clear(); return status; }
	*rows = state.rows.data();
	if (stats) *stats = state.stats;
	return AGPU_OK;
}

int agpu_allele_counts_allocated_bytes(agpu_ctx* ctx, uint64_t* bytes) {
	if (!ctx || !bytes) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	*bytes = ctx->allele.allocated();
	return AGPU_OK;
}

}
