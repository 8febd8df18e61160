// arriba_amd/csrc/device/agpu_variants.hip -- --variant-sites on the MI355X: the positions at which the records of the last ingest show a base that differs from the assembly, with
// their full base counts (include/arriba_gpu.h: agpu_variant_sites).  What decides a number is variant_core.hpp and allele_core.hpp, which the host steps as well
// (arriba_amd/csrc/host/variant_sites.cpp); the rule is DESIGN.md 4.21.  Here are
//   variant_event_kernel      one WAVEFRONT per record through ingest.record_offset: the head and the filter (allele_record) once per wavefront, the CIGAR walked by all 64 lanes
//                             together (every value of the walk is the same in every lane: scalar work), and inside a block of M, = or X lane i takes base step * 64 + i, so that
//                             neighbouring lanes read neighbouring QUAL bytes, neighbouring SEQ nibbles and neighbouring bytes of the assembly.  Two instantiations: the count
//                             pass (a ballot and a popcount per step, one atomic add per wavefront into the total, which is spread over 1 024 cache lines) and the fill pass into a buffer of exactly that many keys (the
//                             leader claims popcount slots with one atomic per step that has events, the lanes write at the claim plus the events in the lanes below them).  A
//                             claim beyond the capacity is not written and fails the call.  The order of the buffer is that of the claims: it is sorted next
//   rocPRIM radix_sort_keys   the event keys ((ref << 32 | pos) << 2 | alt) over 2 + 32 + bits_of(n_ref) bits; run_length_encode: (key, support) per distinct key
//   variant_candidate_kernel  one lane per run: support >= min_alt and no earlier run of the site with it -> the site key and a flag; rocPRIM select: the candidate sites, ascending
//   allele_bitmap_kernel, allele_count_kernel   of --allele-counts (allele_count.hpp): the eight counters of every candidate site
//   variant_rows_kernel       one lane per candidate: its counters, its (up to three) runs, neighbours in the run table, found by allele_lower_bound; the percent test, the check that
//                             every support equals its counter, REF and the mask of the reported alts; rocPRIM select: the reported rows, one copy to the host
// Counters are unsigned sums and the keys are sorted: the rows are the same under every schedule.  The stream is only read.
// The event kernel reads every base of every counting record once: bound by the bytes of SEQ, QUAL and the assembly under the blocks.  No MFMA, no LDS.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <rocprim/rocprim.hpp>
#define AGPU_OPTION "--variant-sites"
#define ALLOC(buffer, bytes) AGPU_ALLOC(buffer, bytes, state.note_peak())
#include "allele_count.hpp"
#include "variant_core.hpp"

using namespace agpu;

namespace {

enum { PASS_COUNT = 0, PASS_FILL = 1, PASS_GROUP = 2, PASS_COUNTERS = 3, PASS_ROWS = 4, PASSES = 5 };
enum { WORD_CURSOR = 0, WORD_OVERFLOW = 1, WORD_INCONSISTENT = 2, WORDS = 3 };
const uint64_t LAUNCH_RECORDS = LAUNCH_ITEMS / 64; // a wavefront per record: 64 work-items each
// The totals of the count pass: one atomic add per wavefront and total, spread by workgroup over TOTAL_SLOTS cache lines of (events, contributing) that the host adds up.  On two
// words for all wavefronts the count pass took 372 ms where the fill pass, which claims per step, took 82 (2.7 x 10^7 records: DESIGN.md 4.21).
enum { TOTAL_SLOTS = 1024, TOTAL_SLOT_WORDS = 8, TOTAL_EVENTS = 0, TOTAL_CONTRIBUTING = 1 };

// The records [first, end) of the stream, one per wavefront.  FILL false: the events of the record and 1 if it counts are added to the slot of the workgroup in `totals`.  FILL true:
// the keys of its events into keys[0 .. capacity) at places claimed from words[WORD_CURSOR]; a claim beyond the capacity adds to words[WORD_OVERFLOW] and writes nothing.
template <bool FILL> __global__ void __launch_bounds__(BLOCK) variant_event_kernel(const uint8_t* __restrict__ stream, uint64_t stream_size, const uint64_t* __restrict__ record_offset, uint64_t first, uint64_t end,
		const uint32_t* __restrict__ ref_length, const uint32_t* __restrict__ tid_to_contig, uint32_t n_ref, GenomeView genome, uint32_t min_mapq, uint32_t min_baseq, uint64_t* keys, uint64_t capacity, unsigned long long* words, unsigned long long* totals) {
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t r = first + (uint64_t) blockIdx.x * (BLOCK / 64) + (uint32_t) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6)); // (the same in every lane, and the compiler knows it)
	if (r >= end) return;
	AlleleRecord record;
	if (!allele_record(stream, record_offset[r], stream_size, n_ref, min_mapq, record)) return;
	const uint32_t length = ref_length[record.ref], contig = tid_to_contig[record.ref];
	int64_t at = record.pos; uint64_t read_index = 0;
	unsigned long long mine = 0;
	for (uint32_t k = 0; k < record.n_cigar; ++k) {
		const uint32_t word = sbam_load32(stream, record.cigar_at + 4ull * k), op = word & 15u;
		const int64_t span = word >> 4;
		if (op == 0 || op == 7 || op == 8) { // M, =, X
			const int64_t lo = at < 0 ? -at : 0, hi = at + span < (int64_t) length ? span : (int64_t) length - at; // the bases of the block that lie inside [0, LN)
			for (int64_t step = lo & ~63ll; step < hi; step += 64) { // (the steps count from the start of the block)
				const int64_t j = step + lane;
				const uint32_t alt = j >= lo && j < hi ? variant_base_event(stream, record, genome, contig, length, at, read_index, (uint64_t) j, min_baseq) : VARIANT_NO_EVENT;
				const unsigned long long events = __ballot(alt != VARIANT_NO_EVENT);
				if (events == 0) continue; // (the same in every lane)
				const unsigned long long found = (unsigned long long) __popcll(events);
				if (!FILL) { mine += found; continue; }
				unsigned long long claim = 0;
				if (lane == 0) claim = atomicAdd(&words[WORD_CURSOR], found);
				claim = __shfl(claim, 0);
				if (claim + found > capacity) { if (lane == 0) atomicAdd(&words[WORD_OVERFLOW], found); continue; }
				const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t) (events >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) events, 0u)); // the events in the lanes below this one
				if (alt != VARIANT_NO_EVENT) keys[claim + below] = variant_key(record.ref, (uint32_t) (at + j), alt);
			}
			at += span; read_index += (uint64_t) span;
		}
		else if (op == 2 || op == 3) at += span;               // D, N
		else if (op == 1 || op == 4) read_index += (uint64_t) span; // I, S
	}
	if (!FILL && lane == 0) {
		unsigned long long* slot = totals + (size_t) (blockIdx.x % TOTAL_SLOTS) * TOTAL_SLOT_WORDS;
		atomicAdd(&slot[TOTAL_CONTRIBUTING], 1ull);
		if (mine != 0) atomicAdd(&slot[TOTAL_EVENTS], mine);
	}
}

// run_keys, support: the distinct event keys, ascending, with the number of their events.  site[i]: the allele_key of run i; flag[i]: 1 if run i is the first of its site with
// support >= min_alt (a site has at most three runs: the alts that are not REF)
__global__ void __launch_bounds__(BLOCK) variant_candidate_kernel(const uint64_t* __restrict__ run_keys, const uint32_t* __restrict__ support, uint64_t n_runs, uint32_t min_alt, uint64_t* site, uint8_t* flag) {
	const uint64_t i = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (i >= n_runs) return;
	const uint64_t mine = variant_key_site(run_keys[i]);
	bool first = support[i] >= min_alt;
	for (uint64_t back = 1; first && back <= 3 && back <= i; ++back) {
		if (variant_key_site(run_keys[i - back]) != mine) break;
		if (support[i - back] >= min_alt) first = false;
	}
	site[i] = mine; flag[i] = first ? 1 : 0;
}

// one lane per candidate site: the row, and flag[c] = 1 if it is reported
__global__ void __launch_bounds__(BLOCK) variant_rows_kernel(const uint64_t* __restrict__ candidates, uint64_t n_candidates, const uint32_t* __restrict__ counts, const uint64_t* __restrict__ run_keys, const uint32_t* __restrict__ support,
		uint64_t n_runs, const uint32_t* __restrict__ tid_to_contig, uint32_t n_ref, GenomeView genome, uint32_t min_alt, uint32_t min_percent, agpu_variant_row* rows, uint8_t* flag, unsigned long long* words) {
	const uint64_t c = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (c >= n_candidates) return;
	const uint64_t site = candidates[c];
	const uint32_t ref = (uint32_t) (site >> 32), pos = (uint32_t) site;
	const uint32_t* mine = counts + c * ALLELE_COLUMNS;
	uint32_t of_alt[4] = { 0, 0, 0, 0 };
	for (uint64_t i = allele_lower_bound(run_keys, n_runs, site << 2); i < n_runs && variant_key_site(run_keys[i]) == site; ++i) of_alt[variant_key_alt(run_keys[i])] = support[i];
	const uint8_t ref_base = ref < n_ref ? allele_ref_base(genome, tid_to_contig[ref], pos) : (uint8_t) 'N';
	bool consistent = true;
	const uint32_t mask = variant_row_mask(mine, of_alt, ref_base, min_alt, min_percent, consistent);
	if (!consistent) atomicAdd(&words[WORD_INCONSISTENT], 1ull);
	agpu_variant_row row;
	row.ref = ref; row.pos = (int32_t) pos;
	row.a = mine[ALLELE_A]; row.c = mine[ALLELE_C]; row.g = mine[ALLELE_G]; row.t = mine[ALLELE_T]; row.n = mine[ALLELE_N]; row.del = mine[ALLELE_DEL]; row.skip = mine[ALLELE_SKIP]; row.lowq = mine[ALLELE_LOWQ];
	row.ref_base = ref_base; row.alt_mask = (uint8_t) mask; row.reserved[0] = row.reserved[1] = 0;
	rows[c] = row; flag[c] = mask != 0 ? 1 : 0;
}

template <bool FILL> void launch_events(agpu_ctx* ctx, const ResidentStream& resident, const uint32_t* lengths, uint32_t n_ref, uint32_t min_mapq, uint32_t min_baseq, uint64_t* keys, uint64_t capacity, unsigned long long* words, unsigned long long* totals) {
	const uint64_t n = resident.records, piece = knob_of("ARRIBA_VARIANT_LAUNCH_RECORDS", LAUNCH_RECORDS, LAUNCH_RECORDS);
	const uint32_t* tid_to_contig = ctx->ingest_tid_to_contig.as<uint32_t>();
	// SEQ, QUAL and the assembly under 100 bases, the head and the CIGAR, the offset: what a record of the headline sample costs
	KernelTimer timer(ctx, FILL ? "variant_event_kernel<fill>" : "variant_event_kernel<count>", n * (8 + 64 + 250));
	for_each_launch_piece(n, [&](uint64_t first, unsigned int) { // (the pieces are counted in records: 64 work-items each)
		const uint64_t end = std::min(n, first + piece);
		const unsigned int grid = (unsigned int) ((end - first + BLOCK / 64 - 1) / (BLOCK / 64));
		variant_event_kernel<FILL><<<grid, BLOCK, 0, ctx->stream>>>(resident.stream, resident.stream_size, resident.record_offset, first, end, lengths, tid_to_contig, n_ref, ctx->genome, min_mapq, min_baseq, keys, capacity, words, totals);
	}, piece);
}

int find(agpu_ctx* ctx, const ResidentStream& resident, const uint32_t* ref_length, uint32_t n_ref, uint32_t min_mapq, uint32_t min_baseq, uint32_t min_alt, uint32_t min_percent, hipEvent_t* events) {
	VariantState& state = ctx->variant;
	hipStream_t s = ctx->stream;
	const uint64_t n = resident.records;
	state.stats.records = n;
	// events[2 k] stands directly in front of the first launch of pass k and events[2 k + 1] behind its last one: the read-backs and allocations between two passes are in no
	// interval (the one inside the group pass, the number of runs, is).  The events of the passes that did not run are recorded where the call ends.
	int passed = 0;
	auto skip_to_end = [&]() -> int { for (int k = passed; k < 2 * PASSES; ++k) HIP_CHECK(hipEventRecord(events[k], s)); return AGPU_OK; };
	auto begin_pass = [&](int pass) -> int { HIP_CHECK(hipEventRecord(events[2 * pass], s)); passed = 2 * pass + 1; return AGPU_OK; };
	auto end_pass = [&](int pass) -> int { HIP_CHECK(hipEventRecord(events[2 * pass + 1], s)); passed = 2 * pass + 2; return AGPU_OK; };
	if (n == 0) return skip_to_end();
	DeviceBuffer& words = state.buffer("variant.words"); DeviceBuffer& counts = state.buffer("variant.counts");
	AlleleCounting counting = { state.buffer("variant.ref_length"), state.buffer("variant.window_offset"), state.buffer("variant.contributing"), state.buffer("variant.bitmap"), counts, 0, true };
	DeviceBuffer& totals = state.buffer("variant.totals");
	const size_t totals_bytes = (size_t) TOTAL_SLOTS * TOTAL_SLOT_WORDS * 8;
	ALLOC(words, WORDS * 8); ALLOC(totals, totals_bytes);
	HIP_CHECK(hipMemsetAsync(words.ptr, 0, WORDS * 8, s));
	HIP_CHECK(hipMemsetAsync(totals.ptr, 0, totals_bytes, s));
	{ DeviceBuffer& lengths = counting.lengths; // (the lengths for the event passes; the counters bring them again with the rest of their tables)
	  ALLOC(lengths, std::max<size_t>(n_ref, 1) * 4);
	  if (n_ref > 0) { HIP_CHECK(hipMemcpyAsync(lengths.ptr, ref_length, (size_t) n_ref * 4, hipMemcpyHostToDevice, s)); HIP_CHECK(hipStreamSynchronize(s)); } } // (the source is pageable memory of the caller)
	unsigned long long host_words[WORDS] = {};
	// the count pass
	TRY(begin_pass(PASS_COUNT));
	launch_events<false>(ctx, resident, counting.lengths.as<uint32_t>(), n_ref, min_mapq, min_baseq, nullptr, 0, words.as<unsigned long long>(), totals.as<unsigned long long>());
	TRY(end_pass(PASS_COUNT));
	std::vector<unsigned long long> host_totals((size_t) TOTAL_SLOTS * TOTAL_SLOT_WORDS, 0);
	HIP_CHECK(hipMemcpyAsync(host_totals.data(), totals.ptr, totals_bytes, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	uint64_t n_events = 0;
	for (size_t slot = 0; slot < TOTAL_SLOTS; ++slot) { n_events += host_totals[slot * TOTAL_SLOT_WORDS + TOTAL_EVENTS]; state.stats.contributing += host_totals[slot * TOTAL_SLOT_WORDS + TOTAL_CONTRIBUTING]; }
	state.stats.events = n_events;
	const uint64_t most = knob_of("ARRIBA_VARIANT_MAX_EVENTS", VARIANT_MAX_EVENTS, VARIANT_MAX_EVENTS);
	if (n_events > most) {
		set_last_error("agpu_variant_sites: " + std::to_string(n_events) + " bases differ from the assembly, more than " + std::to_string(most) + " (ARRIBA_VARIANT_MAX_EVENTS): the assembly of -a hardly matches the sample");
		return AGPU_ERR_INVALID;
	}
	if (n_events == 0) return skip_to_end();
	// the fill pass
	DeviceBuffer& keys_in = state.buffer("variant.keys_in"); DeviceBuffer& sorted_keys = state.buffer("variant.keys"); DeviceBuffer& temporary_storage = state.buffer("variant.rocprim");
	ALLOC(keys_in, n_events * 8);
	TRY(begin_pass(PASS_FILL));
	launch_events<true>(ctx, resident, counting.lengths.as<uint32_t>(), n_ref, min_mapq, min_baseq, keys_in.as<uint64_t>(), n_events, words.as<unsigned long long>(), nullptr);
	TRY(end_pass(PASS_FILL));
	HIP_CHECK(hipMemcpyAsync(host_words, words.ptr, sizeof(host_words), hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	if (host_words[WORD_OVERFLOW] != 0 || host_words[WORD_CURSOR] != n_events) {
		set_last_error("agpu_variant_sites: internal error: the fill pass found " + std::to_string(host_words[WORD_CURSOR]) + " events where the count pass found " + std::to_string(n_events));
		return AGPU_ERR_DEVICE;
	}
	// sort, runs, candidates
	DeviceBuffer& support = state.buffer("variant.support"); DeviceBuffer& n_out = state.buffer("variant.n_out");
	ALLOC(sorted_keys, n_events * 8); ALLOC(support, n_events * 4); ALLOC(n_out, 8);
	TRY(begin_pass(PASS_GROUP));
	const unsigned int key_bits = std::min(64u, 2 + 32 + bits_of(n_ref));
	TRY(with_temporary(ctx, temporary_storage, "variant rocprim::radix_sort_keys(events)", n_events * 16, [&](void* storage, size_t& bytes) {
		return rocprim::radix_sort_keys(storage, bytes, keys_in.as<uint64_t>(), sorted_keys.as<uint64_t>(), (size_t) n_events, 0u, key_bits, s); }));
	state.note_peak();
	DeviceBuffer& run_keys = keys_in; // (the unsorted keys are not needed any more: at most as many runs as events)
	TRY(with_temporary(ctx, temporary_storage, "variant rocprim::run_length_encode(events)", n_events * 20, [&](void* storage, size_t& bytes) {
		return rocprim::run_length_encode(storage, bytes, sorted_keys.as<uint64_t>(), (unsigned int) n_events, run_keys.as<uint64_t>(), support.as<uint32_t>(), n_out.as<uint64_t>(), s); }));
	state.note_peak();
	uint64_t n_runs = 0;
	HIP_CHECK(hipMemcpyAsync(&n_runs, n_out.ptr, 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	if (n_runs == 0 || n_runs > n_events) { set_last_error("agpu_variant_sites: internal error: " + std::to_string(n_runs) + " runs of " + std::to_string(n_events) + " events"); return AGPU_ERR_DEVICE; }
	state.stats.runs = n_runs;
	sorted_keys.release();
	DeviceBuffer& run_site = state.buffer("variant.run_site"); DeviceBuffer& run_flag = state.buffer("variant.run_flag"); DeviceBuffer& candidates = state.buffer("variant.candidates");
	ALLOC(run_site, n_runs * 8); ALLOC(run_flag, n_runs); ALLOC(candidates, n_runs * 8);
	{ KernelTimer timer(ctx, "variant_candidate_kernel", n_runs * 21);
	  variant_candidate_kernel<<<grid_for(n_runs), BLOCK, 0, s>>>(run_keys.as<uint64_t>(), support.as<uint32_t>(), n_runs, min_alt, run_site.as<uint64_t>(), run_flag.as<uint8_t>()); }
	TRY(with_temporary(ctx, temporary_storage, "variant rocprim::select(candidates)", n_runs * 17, [&](void* storage, size_t& bytes) {
		return rocprim::select(storage, bytes, run_site.as<uint64_t>(), run_flag.as<uint8_t>(), candidates.as<uint64_t>(), n_out.as<uint64_t>(), (size_t) n_runs, s); }));
	state.note_peak();
	TRY(end_pass(PASS_GROUP));
	uint64_t n_candidates = 0;
	HIP_CHECK(hipMemcpyAsync(&n_candidates, n_out.ptr, 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	if (n_candidates > n_runs) { set_last_error("agpu_variant_sites: internal error: " + std::to_string(n_candidates) + " candidate sites of " + std::to_string(n_runs) + " runs"); return AGPU_ERR_DEVICE; }
	if (n_candidates > ALLELE_MAX_SITES) { set_last_error("agpu_variant_sites: more than 2^29-1 candidate sites: the assembly of -a hardly matches the sample"); return AGPU_ERR_INVALID; }
	state.stats.candidates = n_candidates;
	run_site.release(); run_flag.release();
	if (n_candidates == 0) return skip_to_end();
	// the eight counters of every candidate site: the bitmap and the count of --allele-counts
	DeviceBuffer& all_rows = state.buffer("variant.all_rows"); DeviceBuffer& row_flag = state.buffer("variant.row_flag"); DeviceBuffer& rows = state.buffer("variant.rows");
	ALLOC(all_rows, n_candidates * sizeof(agpu_variant_row)); ALLOC(row_flag, n_candidates); ALLOC(rows, n_candidates * sizeof(agpu_variant_row));
	TRY(allele_counting_begin(ctx, state, counting, ref_length, n_ref, n_candidates));
	HIP_CHECK(hipStreamSynchronize(s)); // (the tables of the counters come from pageable memory)
	TRY(begin_pass(PASS_COUNTERS));
	allele_counting_bitmap(ctx, counting, candidates.as<uint64_t>(), n_ref);
	allele_counting_records(ctx, counting, resident, candidates.as<uint64_t>(), n_ref, min_mapq, min_baseq);
	TRY(end_pass(PASS_COUNTERS));
	// the rows
	TRY(begin_pass(PASS_ROWS));
	{ KernelTimer timer(ctx, "variant_rows_kernel", n_candidates * (8 + 32 + 36 + sizeof(agpu_variant_row) + 1));
	  variant_rows_kernel<<<grid_for(n_candidates), BLOCK, 0, s>>>(candidates.as<uint64_t>(), n_candidates, counts.as<uint32_t>(), run_keys.as<uint64_t>(), support.as<uint32_t>(), n_runs, ctx->ingest_tid_to_contig.as<uint32_t>(), n_ref, ctx->genome,
	                                                                 min_alt, min_percent, all_rows.as<agpu_variant_row>(), row_flag.as<uint8_t>(), words.as<unsigned long long>()); }
	TRY(with_temporary(ctx, temporary_storage, "variant rocprim::select(rows)", n_candidates * (2 * sizeof(agpu_variant_row) + 1), [&](void* storage, size_t& bytes) {
		return rocprim::select(storage, bytes, all_rows.as<agpu_variant_row>(), row_flag.as<uint8_t>(), rows.as<agpu_variant_row>(), n_out.as<uint64_t>(), (size_t) n_candidates, s); }));
	state.note_peak();
	TRY(end_pass(PASS_ROWS));
	uint64_t n_rows = 0; unsigned long long counted_records = 0;
	HIP_CHECK(hipMemcpyAsync(&n_rows, n_out.ptr, 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipMemcpyAsync(host_words, words.ptr, sizeof(host_words), hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipMemcpyAsync(&counted_records, counting.contributing.ptr, 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	if (counted_records != state.stats.contributing) { // (the counter kernel applies the same filter as the event passes)
		set_last_error("agpu_variant_sites: internal error: the counters come from " + std::to_string(counted_records) + " records, the events from " + std::to_string(state.stats.contributing));
		return AGPU_ERR_DEVICE;
	}
	if (n_rows > n_candidates) { set_last_error("agpu_variant_sites: internal error: " + std::to_string(n_rows) + " rows of " + std::to_string(n_candidates) + " candidate sites"); return AGPU_ERR_DEVICE; }
	state.stats.reported = n_rows; state.stats.inconsistent = host_words[WORD_INCONSISTENT];
	if (state.stats.inconsistent != 0) {
		set_last_error("agpu_variant_sites: internal error: the events of " + std::to_string(state.stats.inconsistent) + " candidate sites disagree with their counters");
		return AGPU_ERR_DEVICE;
	}
	state.rows.resize(n_rows);
	if (n_rows > 0) { HIP_CHECK(hipMemcpyAsync(state.rows.data(), rows.ptr, n_rows * sizeof(agpu_variant_row), hipMemcpyDeviceToHost, s)); HIP_CHECK(hipStreamSynchronize(s)); }
	return AGPU_OK;
}

}

extern "C" {

int agpu_variant_sites(agpu_ctx* ctx, const uint32_t* ref_length, uint32_t n_ref, uint32_t min_mapq, uint32_t min_baseq, uint32_t min_alt, uint32_t min_percent, const agpu_variant_row** rows, uint64_t* n_rows, agpu_variant_stats* stats) {
	if (!ctx || !rows || !n_rows || (n_ref > 0 && !ref_length)) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	*rows = nullptr; *n_rows = 0;
	if (stats) memset(stats, 0, sizeof(*stats));
	if (min_mapq > 255 || min_baseq > 255) { set_last_error("agpu_variant_sites: a threshold above 255"); return AGPU_ERR_INVALID; }
	if (min_alt < 1 || min_alt > 0x7FFFFFFFu) { set_last_error("agpu_variant_sites: min_alt is 1 to 2^31-1"); return AGPU_ERR_INVALID; }
	if (min_percent > 100) { set_last_error("agpu_variant_sites: min_percent is 0 to 100"); return AGPU_ERR_INVALID; }
	if (n_ref >= VARIANT_MAX_REFERENCES) { set_last_error("agpu_variant_sites: 2^30 references or more"); return AGPU_ERR_INVALID; }
	ResidentStream resident;
	TRY(resident_stream(ctx, "agpu_variant_sites", "variant sites of one sample over several GPUs are not supported", nullptr, resident, NEEDS_GENOME | NEEDS_REFERENCES, n_ref));
	HIP_CHECK(hipSetDevice(ctx->device));
	VariantState& state = ctx->variant;
	memset(&state.stats, 0, sizeof(state.stats));
	state.rows.clear(); state.peak = 0;
	const int status = one_shot<2 * PASSES>(ctx, state, "agpu_variant_sites", [&](hipEvent_t* events) {
		const int found = find(ctx, resident, ref_length, n_ref, min_mapq, min_baseq, min_alt, min_percent, events);
		(void) hipStreamSynchronize(ctx->stream); // (the events of a call that ended early have happened)
		if (found == AGPU_OK) for (int k = 0; k < PASSES; ++k) { float ms = 0; if (hipEventElapsedTime(&ms, events[2 * k], events[2 * k + 1]) == hipSuccess) state.stats.seconds[k] = ms / 1000.0; }
		return found;
	}, [&](int) { state.stats.peak_bytes = state.peak; state.release_all(); });
	if (stats) *stats = state.stats; // (also of a call that failed: what it had counted)
	if (status != AGPU_OK) { state.rows.clear(); return status; }
	*rows = state.rows.data(); *n_rows = state.rows.size();
	return AGPU_OK;
}

int agpu_variant_sites_allocated_bytes(agpu_ctx* ctx, uint64_t* bytes) {
	if (!ctx || !bytes) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	*bytes = ctx->variant.allocated();
	return AGPU_OK;
}

}
