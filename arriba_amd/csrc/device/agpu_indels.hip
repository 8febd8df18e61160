// arriba_amd/csrc/device/agpu_indels.hip -- --indel-sites on the MI355X: the insertions and deletions the records of the last ingest carry in their CIGARs, left-normalised against
// the assembly, with their support and the depth at their anchor (include/arriba_gpu.h: agpu_indel_sites).  What decides a number is indel_core.hpp and allele_core.hpp, which the
// host steps as well (arriba_amd/csrc/host/indel_sites.cpp); the rule is DESIGN.md 4.22.  Here are
//   indel_event_kernel       one LANE per record through ingest.record_offset: the head and the filter (allele_record), then the CIGAR words (indel_walk); only a record with an I
//                            or D between two aligned blocks -- about one in a hundred -- touches a few SEQ bytes (the nibbles of an insertion) and a few bytes of the assembly
//                            (the normalisation).  Two instantiations.  The count pass writes ONE total per wavefront (wave_sum) into wave_total[]; rocPRIM's exclusive_scan over
//                            those totals gives every wavefront its place, and the last element the number of events.  The fill pass counts its records again (the CIGAR is in
//                            the cache of the walk that follows), takes the in-wavefront prefix of the lanes below with six shuffles, and writes its events at place + prefix:
//                            no claim cursor, no atomic, and the unsorted buffer is the same under every run.  Every write is checked against the capacity and the last lane of
//                            every wavefront checks where it ended against the place of the next one; a disagreement fails the call
//   rocPRIM merge_sort       the two-word events by (site, shape); run_length_encode: (event, support) per distinct event
//   indel_candidate_kernel   one lane per run: its site and whether support >= min_alt; rocPRIM select, then unique: the candidate sites, ascending (a site has any number of runs)
//   allele_bitmap_kernel, allele_count_kernel   of --allele-counts (allele_count.hpp), unchanged, with min_baseq 0: the eight counters of every candidate site
//   indel_rows_kernel        one lane per run; a run below min_alt leaves at once, the others find the counters of their site by allele_lower_bound, apply the percent test and
//                            write the row; the supports are summed on the way (they must add up to the events); rocPRIM select: the reported rows, one copy to the host
// The stream is only read.  No MFMA, no LDS, no scratch.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <rocprim/rocprim.hpp>
#define AGPU_OPTION "--indel-sites"
#define ALLOC(buffer, bytes) AGPU_ALLOC(buffer, bytes, state.note_peak())
#include "allele_count.hpp"
#include "indel_core.hpp"

using namespace agpu;

namespace {

enum { PASS_COUNT = 0, PASS_FILL = 1, PASS_GROUP = 2, PASS_COUNTERS = 3, PASS_ROWS = 4, PASSES = 5 };
enum { WORD_OVERFLOW = 0, WORD_MISPLACED = 1, WORD_SUPPORT = 2, WORD_NO_SITE = 3, WORDS = 4 };
// The statistics of the count pass (not the events: those go to wave_total): an atomic add per wavefront and number that is not zero, spread by workgroup over TOTAL_SLOTS cache
// lines that the host adds up (on one line for all wavefronts such adds serialise: DESIGN.md 4.21).
enum { TOTAL_SLOTS = 1024, TOTAL_SLOT_WORDS = 8, TOTAL_CONTRIBUTING = 0, TOTAL_OPERATIONS = 1, TOTAL_UNKEYED = 2, TOTAL_CAPPED = 3 };

// writes the events of one record at events[at ..), below the capacity only
struct IndelWriter {
	IndelEvent* events; uint64_t at, capacity; unsigned long long* words;
	AGPU_HD void operator()(uint64_t site, uint64_t shape) {
		if (at < capacity) { events[at].site = site; events[at].shape = shape; } else words[WORD_OVERFLOW] = 1; // (a plain store: every lane that gets here writes the same value)
		++at;
	}
};

// The records [first, end) of the stream, one per lane; the wavefronts of the launch are first_wave, first_wave + 1, ... of the call.  FILL false: wave_total[wavefront] = the
// events of its 64 records; contributing records, operations, unkeyed insertions and capped events are added to the slot of the workgroup in `totals`.  FILL true: wave_place is the
// exclusive scan of wave_total with the total behind it; the events of the wavefront go to events[wave_place[wavefront] ..), record by record.  No lane leaves early: every one
// takes part in the shuffles.
template <bool FILL> __global__ void __launch_bounds__(BLOCK) indel_event_kernel(const uint8_t* __restrict__ stream, uint64_t stream_size, const uint64_t* __restrict__ record_offset, uint64_t first, uint64_t end,
		const uint32_t* __restrict__ ref_length, const uint32_t* __restrict__ tid_to_contig, uint32_t n_ref, GenomeView genome, uint32_t min_mapq, uint32_t max_shift, uint64_t first_wave,
		unsigned long long* wave_total, const unsigned long long* __restrict__ wave_place, IndelEvent* events, uint64_t capacity, unsigned long long* words, unsigned long long* totals) {
	const uint32_t lane = threadIdx.x & 63u;
	const uint64_t r = first + (uint64_t) blockIdx.x * BLOCK + threadIdx.x, wave = first_wave + (uint64_t) blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
	AlleleRecord record;
	const bool live = r < end && allele_record(stream, record_offset[r], stream_size, n_ref, min_mapq, record);
	uint32_t length = 0, contig = 0;
	IndelTally tally = { 0, 0, 0, 0 };
	IndelNoSink nothing;
	if (live) {
		length = ref_length[record.ref]; contig = tid_to_contig[record.ref];
		indel_walk(stream, record, genome, contig, length, max_shift, false, tally, nothing);
	}
	const uint32_t mine = tally.events;
	if (!FILL) {
		if (mine != 0) { IndelTally resolved = { 0, 0, 0, 0 }; indel_walk(stream, record, genome, contig, length, max_shift, true, resolved, nothing); tally.capped = resolved.capped; }
		const unsigned int found = wave_sum((unsigned int) mine), contributing = wave_sum(live ? 1u : 0u), operations = wave_sum((unsigned int) tally.operations),
		                   unkeyed = wave_sum((unsigned int) tally.unkeyed), capped = wave_sum((unsigned int) tally.capped);
		if (lane == 0) {
			wave_total[wave] = found;
			unsigned long long* slot = totals + (size_t) (blockIdx.x % TOTAL_SLOTS) * TOTAL_SLOT_WORDS;
			if (contributing != 0) atomicAdd(&slot[TOTAL_CONTRIBUTING], (unsigned long long) contributing);
			if (operations != 0) atomicAdd(&slot[TOTAL_OPERATIONS], (unsigned long long) operations);
			if (unkeyed != 0) atomicAdd(&slot[TOTAL_UNKEYED], (unsigned long long) unkeyed);
			if (capped != 0) atomicAdd(&slot[TOTAL_CAPPED], (unsigned long long) capped);
		}
	} else {
		uint32_t inclusive = mine; // the events of this lane and the lanes below it
		for (int offset = 1; offset < 64; offset <<= 1) {
			const uint32_t other = __shfl_up(inclusive, offset);
			if (lane >= (uint32_t) offset) inclusive += other;
		}
		const uint64_t place = wave_place[wave];
		if (mine != 0) {
			IndelWriter writer = { events, place + inclusive - mine, capacity, words };
			IndelTally resolved = { 0, 0, 0, 0 };
			indel_walk(stream, record, genome, contig, length, max_shift, true, resolved, writer);
			if (writer.at != place + inclusive) words[WORD_MISPLACED] = 1; // (the second walk found another number than the first)
		}
		if (lane == 63 && place + inclusive != wave_place[wave + 1]) words[WORD_MISPLACED] = 1; // (the count pass found another number)
	}
}

// run_events, support: the distinct events, ascending, with the number of their records.  site[i]: the allele_key of run i; flag[i]: 1 if support >= min_alt
__global__ void __launch_bounds__(BLOCK) indel_candidate_kernel(const IndelEvent* __restrict__ run_events, const uint32_t* __restrict__ support, uint64_t n_runs, uint32_t min_alt, uint64_t* site, uint8_t* flag) {
	const uint64_t i = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (i >= n_runs) return;
	site[i] = run_events[i].site; flag[i] = support[i] >= min_alt ? 1 : 0;
}

// one lane per run: the row of a run with support >= min_alt, and flag[i] = 1 if it is reported.  sites, counts: the candidate sites, ascending, and their eight counters.  No
// lane leaves before the supports of the wavefront are summed.
__global__ void __launch_bounds__(BLOCK) indel_rows_kernel(const IndelEvent* __restrict__ run_events, const uint32_t* __restrict__ support, uint64_t n_runs, const uint64_t* __restrict__ sites, uint64_t n_sites,
		const uint32_t* __restrict__ counts, const uint32_t* __restrict__ tid_to_contig, uint32_t n_ref, GenomeView genome, uint32_t min_alt, uint32_t min_percent, agpu_indel_row* rows, uint8_t* flag, unsigned long long* words) {
	const uint64_t i = (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	const uint32_t mine = i < n_runs ? support[i] : 0u;
	const unsigned long long sum = wave_sum((unsigned long long) mine);
	if ((threadIdx.x & 63u) == 0 && sum != 0) atomicAdd(&words[WORD_SUPPORT], sum);
	if (i >= n_runs) return;
	agpu_indel_row row = {};
	bool reported = false;
	if (mine >= min_alt) {
		const IndelEvent event = run_events[i];
		const uint64_t slot = allele_lower_bound(sites, n_sites, event.site);
		if (slot >= n_sites || sites[slot] != event.site) atomicAdd(&words[WORD_NO_SITE], 1ull);
		else {
			const uint32_t* of_site = counts + slot * ALLELE_COLUMNS;
			const uint64_t depth = (uint64_t) of_site[ALLELE_A] + of_site[ALLELE_C] + of_site[ALLELE_G] + of_site[ALLELE_T] + of_site[ALLELE_N] + of_site[ALLELE_DEL]; // (a record adds to one column: below 2^32)
			const uint32_t ref = (uint32_t) (event.site >> 32), pos = (uint32_t) event.site;
			row.ref = ref; row.pos = (int32_t) pos; row.bases = indel_shape_bases(event.shape); row.length = indel_shape_length(event.shape); row.support = mine; row.depth = (uint32_t) depth;
			row.type = (uint8_t) indel_shape_type(event.shape); row.ref_base = ref < n_ref ? allele_ref_base(genome, tid_to_contig[ref], pos) : (uint8_t) 'N';
			reported = indel_reported(mine, depth, min_alt, min_percent);
		}
	}
	rows[i] = row; flag[i] = reported ? 1 : 0;
}

// the launches of the event kernel: pieces of `piece` records; launch(first, end, grid, first_wave).  Returns the wavefronts of all launches.
template <class Launch> uint64_t for_each_event_launch(uint64_t n, uint64_t piece, Launch launch) {
	uint64_t waves = 0;
	for_each_launch_piece(n, [&](uint64_t first, unsigned int grid) { launch(first, std::min(n, first + piece), grid, waves); waves += (uint64_t) grid * (BLOCK / 64); }, piece);
	return waves;
}
uint64_t launch_records() { return knob_of("ARRIBA_INDEL_LAUNCH_RECORDS", LAUNCH_ITEMS, LAUNCH_ITEMS); }

template <bool FILL> void launch_events(agpu_ctx* ctx, const ResidentStream& resident, const uint32_t* lengths, uint32_t n_ref, uint32_t min_mapq, uint32_t max_shift, unsigned long long* wave_total, const unsigned long long* wave_place,
                                        IndelEvent* events, uint64_t capacity, unsigned long long* words, unsigned long long* totals) {
	const uint32_t* tid_to_contig = ctx->ingest_tid_to_contig.as<uint32_t>();
	// the offset, the head and a CIGAR of two operations: what a record of the headline sample costs (the name is skipped)
	KernelTimer timer(ctx, FILL ? "indel_event_kernel<fill>" : "indel_event_kernel<count>", resident.records * (8 + 36 + 8));
	for_each_event_launch(resident.records, launch_records(), [&](uint64_t first, uint64_t end, unsigned int grid, uint64_t first_wave) {
		indel_event_kernel<FILL><<<grid, BLOCK, 0, ctx->stream>>>(resident.stream, resident.stream_size, resident.record_offset, first, end, lengths, tid_to_contig, n_ref, ctx->genome, min_mapq, max_shift, first_wave,
		                                                         wave_total, wave_place, events, capacity, words, totals);
	});
}

int find(agpu_ctx* ctx, const ResidentStream& resident, const uint32_t* ref_length, uint32_t n_ref, uint32_t min_mapq, uint32_t min_alt, uint32_t min_percent, hipEvent_t* events) {
	IndelState& state = ctx->indel;
	hipStream_t s = ctx->stream;
	const uint64_t n = resident.records;
	state.stats.records = n;
	// events[2 k] stands directly in front of the first launch of pass k and events[2 k + 1] behind its last one: the read-backs and allocations between two passes are in no
	// interval.  The events of the passes that did not run are recorded where the call ends.
	int passed = 0;
	auto skip_to_end = [&]() -> int { for (int k = passed; k < 2 * PASSES; ++k) HIP_CHECK(hipEventRecord(events[k], s)); return AGPU_OK; };
	auto begin_pass = [&](int pass) -> int { HIP_CHECK(hipEventRecord(events[2 * pass], s)); passed = 2 * pass + 1; return AGPU_OK; };
	auto end_pass = [&](int pass) -> int { HIP_CHECK(hipEventRecord(events[2 * pass + 1], s)); passed = 2 * pass + 2; return AGPU_OK; };
	if (n == 0) return skip_to_end();
	const uint32_t max_shift = (uint32_t) knob_of("ARRIBA_INDEL_MAX_SHIFT", INDEL_MAX_SHIFT, INDEL_MAX_SHIFT);
	const uint64_t n_waves = for_each_event_launch(n, launch_records(), [](uint64_t, uint64_t, unsigned int, uint64_t) {});
	DeviceBuffer& words = state.buffer("indel.words"); DeviceBuffer& counts = state.buffer("indel.counts"); DeviceBuffer& totals = state.buffer("indel.totals");
	DeviceBuffer& wave_total = state.buffer("indel.wave_total"); DeviceBuffer& wave_place = state.buffer("indel.wave_place"); DeviceBuffer& temporary_storage = state.buffer("indel.rocprim");
	AlleleCounting counting = { state.buffer("indel.ref_length"), state.buffer("indel.window_offset"), state.buffer("indel.contributing"), state.buffer("indel.bitmap"), counts, 0, true };
	const size_t totals_bytes = (size_t) TOTAL_SLOTS * TOTAL_SLOT_WORDS * 8, wave_bytes = (size_t) (n_waves + 1) * 8; // (one more: the scan leaves the number of events there)
	ALLOC(words, WORDS * 8); ALLOC(totals, totals_bytes); ALLOC(wave_total, wave_bytes); ALLOC(wave_place, wave_bytes);
	HIP_CHECK(hipMemsetAsync(words.ptr, 0, WORDS * 8, s));
	HIP_CHECK(hipMemsetAsync(totals.ptr, 0, totals_bytes, s));
	HIP_CHECK(hipMemsetAsync(wave_total.ptr, 0, wave_bytes, s));
	{ DeviceBuffer& lengths = counting.lengths; // (the lengths for the event passes; the counters bring them again with the rest of their tables)
	  ALLOC(lengths, std::max<size_t>(n_ref, 1) * 4);
	  if (n_ref > 0) { HIP_CHECK(hipMemcpyAsync(lengths.ptr, ref_length, (size_t) n_ref * 4, hipMemcpyHostToDevice, s)); HIP_CHECK(hipStreamSynchronize(s)); } } // (the source is pageable memory of the caller)
	unsigned long long host_words[WORDS] = {};
	// the count pass, and the scan of its totals
	TRY(begin_pass(PASS_COUNT));
	launch_events<false>(ctx, resident, counting.lengths.as<uint32_t>(), n_ref, min_mapq, max_shift, wave_total.as<unsigned long long>(), nullptr, nullptr, 0, words.as<unsigned long long>(), totals.as<unsigned long long>());
	TRY(with_temporary(ctx, temporary_storage, "indel rocprim::exclusive_scan(wave totals)", (n_waves + 1) * 16, [&](void* storage, size_t& bytes) {
		return rocprim::exclusive_scan(storage, bytes, wave_total.as<unsigned long long>(), wave_place.as<unsigned long long>(), 0ull, (size_t) (n_waves + 1), rocprim::plus<unsigned long long>(), s); }));
	state.note_peak();
	TRY(end_pass(PASS_COUNT));
	std::vector<unsigned long long> host_totals((size_t) TOTAL_SLOTS * TOTAL_SLOT_WORDS, 0);
	unsigned long long n_events = 0;
	HIP_CHECK(hipMemcpyAsync(host_totals.data(), totals.ptr, totals_bytes, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipMemcpyAsync(&n_events, wave_place.as<unsigned long long>() + n_waves, 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	for (size_t slot = 0; slot < TOTAL_SLOTS; ++slot) {
		const unsigned long long* of_slot = &host_totals[slot * TOTAL_SLOT_WORDS];
		state.stats.contributing += of_slot[TOTAL_CONTRIBUTING]; state.stats.operations += of_slot[TOTAL_OPERATIONS]; state.stats.unkeyed_insertions += of_slot[TOTAL_UNKEYED]; state.stats.shift_capped += of_slot[TOTAL_CAPPED];
	}
	state.stats.events = n_events;
	if (state.stats.operations != n_events + state.stats.unkeyed_insertions) {
		set_last_error("agpu_indel_sites: internal error: " + std::to_string(state.stats.operations) + " operations, " + std::to_string(n_events) + " events and " + std::to_string(state.stats.unkeyed_insertions) + " unkeyed insertions");
		return AGPU_ERR_DEVICE;
	}
	const uint64_t most = knob_of("ARRIBA_INDEL_MAX_EVENTS", INDEL_MAX_EVENTS, INDEL_MAX_EVENTS);
	if (n_events > most) {
		set_last_error("agpu_indel_sites: " + std::to_string(n_events) + " insertions and deletions, more than " + std::to_string(most) + " (ARRIBA_INDEL_MAX_EVENTS)");
		return AGPU_ERR_INVALID;
	}
	if (n_events == 0) return skip_to_end();
	wave_total.release();
	// the fill pass
	DeviceBuffer& events_in = state.buffer("indel.events_in"); DeviceBuffer& sorted_events = state.buffer("indel.events");
	ALLOC(events_in, n_events * sizeof(IndelEvent));
	TRY(begin_pass(PASS_FILL));
	launch_events<true>(ctx, resident, counting.lengths.as<uint32_t>(), n_ref, min_mapq, max_shift, nullptr, wave_place.as<unsigned long long>(), events_in.as<IndelEvent>(), n_events, words.as<unsigned long long>(), nullptr);
	TRY(end_pass(PASS_FILL));
	HIP_CHECK(hipMemcpyAsync(host_words, words.ptr, sizeof(host_words), hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	if (host_words[WORD_OVERFLOW] != 0 || host_words[WORD_MISPLACED] != 0) {
		set_last_error(std::string("agpu_indel_sites: internal error: the fill pass ") + (host_words[WORD_OVERFLOW] != 0 ? "would have written beyond" : "did not end at") + " the " + std::to_string(n_events) + " events of the count pass");
		return AGPU_ERR_DEVICE;
	}
	wave_place.release();
	// sort, runs, candidates
	DeviceBuffer& support = state.buffer("indel.support"); DeviceBuffer& n_out = state.buffer("indel.n_out");
	ALLOC(sorted_events, n_events * sizeof(IndelEvent)); ALLOC(support, n_events * 4); ALLOC(n_out, 8);
	TRY(begin_pass(PASS_GROUP));
	TRY(with_temporary(ctx, temporary_storage, "indel rocprim::merge_sort(events)", n_events * 2 * sizeof(IndelEvent), [&](void* storage, size_t& bytes) {
		return rocprim::merge_sort(storage, bytes, events_in.as<IndelEvent>(), sorted_events.as<IndelEvent>(), (size_t) n_events, IndelEventLess(), s); }));
	state.note_peak();
	DeviceBuffer& run_events = events_in; // (the unsorted events are not needed any more: at most as many runs as events)
	TRY(with_temporary(ctx, temporary_storage, "indel rocprim::run_length_encode(events)", n_events * (2 * sizeof(IndelEvent) + 4), [&](void* storage, size_t& bytes) {
		return rocprim::run_length_encode(storage, bytes, sorted_events.as<IndelEvent>(), (unsigned int) n_events, run_events.as<IndelEvent>(), support.as<uint32_t>(), n_out.as<uint64_t>(), s); }));
	state.note_peak();
	uint64_t n_runs = 0;
	HIP_CHECK(hipMemcpyAsync(&n_runs, n_out.ptr, 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	if (n_runs == 0 || n_runs > n_events) { set_last_error("agpu_indel_sites: internal error: " + std::to_string(n_runs) + " runs of " + std::to_string(n_events) + " events"); return AGPU_ERR_DEVICE; }
	state.stats.runs = n_runs;
	sorted_events.release();
	DeviceBuffer& run_site = state.buffer("indel.run_site"); DeviceBuffer& run_flag = state.buffer("indel.run_flag"); DeviceBuffer& flagged = state.buffer("indel.flagged"); DeviceBuffer& sites = state.buffer("indel.sites");
	ALLOC(run_site, n_runs * 8); ALLOC(run_flag, n_runs); ALLOC(flagged, n_runs * 8); ALLOC(sites, n_runs * 8);
	{ KernelTimer timer(ctx, "indel_candidate_kernel", n_runs * (sizeof(IndelEvent) + 4 + 8 + 1));
	  indel_candidate_kernel<<<grid_for(n_runs), BLOCK, 0, s>>>(run_events.as<IndelEvent>(), support.as<uint32_t>(), n_runs, min_alt, run_site.as<uint64_t>(), run_flag.as<uint8_t>()); }
	TRY(with_temporary(ctx, temporary_storage, "indel rocprim::select(candidates)", n_runs * 17, [&](void* storage, size_t& bytes) {
		return rocprim::select(storage, bytes, run_site.as<uint64_t>(), run_flag.as<uint8_t>(), flagged.as<uint64_t>(), n_out.as<uint64_t>(), (size_t) n_runs, s); }));
	state.note_peak();
	uint64_t n_flagged = 0;
	HIP_CHECK(hipMemcpyAsync(&n_flagged, n_out.ptr, 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	if (n_flagged > n_runs) { set_last_error("agpu_indel_sites: internal error: " + std::to_string(n_flagged) + " candidates of " + std::to_string(n_runs) + " runs"); return AGPU_ERR_DEVICE; }
	state.stats.candidates = n_flagged;
	uint64_t n_sites = 0;
	if (n_flagged > 0) {
		TRY(with_temporary(ctx, temporary_storage, "indel rocprim::unique(candidate sites)", n_flagged * 16, [&](void* storage, size_t& bytes) {
			return rocprim::unique(storage, bytes, flagged.as<uint64_t>(), sites.as<uint64_t>(), n_out.as<uint64_t>(), (size_t) n_flagged, rocprim::equal_to<uint64_t>(), s); }));
		state.note_peak();
	}
	TRY(end_pass(PASS_GROUP));
	if (n_flagged > 0) {
		HIP_CHECK(hipMemcpyAsync(&n_sites, n_out.ptr, 8, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		HIP_CHECK(hipGetLastError());
		if (n_sites == 0 || n_sites > n_flagged) { set_last_error("agpu_indel_sites: internal error: " + std::to_string(n_sites) + " sites of " + std::to_string(n_flagged) + " candidates"); return AGPU_ERR_DEVICE; }
	}
	if (n_sites > ALLELE_MAX_SITES) { set_last_error("agpu_indel_sites: more than 2^29-1 candidate sites"); return AGPU_ERR_INVALID; }
	state.stats.sites = n_sites;
	run_site.release(); run_flag.release(); flagged.release();
	if (n_sites == 0) return skip_to_end();
	// the eight counters of every candidate site: the bitmap and the count of --allele-counts, every base whatever its quality
	DeviceBuffer& all_rows = state.buffer("indel.all_rows"); DeviceBuffer& row_flag = state.buffer("indel.row_flag"); DeviceBuffer& rows = state.buffer("indel.rows");
	ALLOC(all_rows, n_runs * sizeof(agpu_indel_row)); ALLOC(row_flag, n_runs); ALLOC(rows, n_flagged * sizeof(agpu_indel_row));
	TRY(allele_counting_begin(ctx, state, counting, ref_length, n_ref, n_sites));
	HIP_CHECK(hipStreamSynchronize(s)); // (the tables of the counters come from pageable memory)
	TRY(begin_pass(PASS_COUNTERS));
	allele_counting_bitmap(ctx, counting, sites.as<uint64_t>(), n_ref);
	allele_counting_records(ctx, counting, resident, sites.as<uint64_t>(), n_ref, min_mapq, 0);
	TRY(end_pass(PASS_COUNTERS));
	// the rows
	TRY(begin_pass(PASS_ROWS));
	{ KernelTimer timer(ctx, "indel_rows_kernel", n_runs * (sizeof(IndelEvent) + 4 + 1) + n_flagged * (32 + sizeof(agpu_indel_row)));
	  indel_rows_kernel<<<grid_for(n_runs), BLOCK, 0, s>>>(run_events.as<IndelEvent>(), support.as<uint32_t>(), n_runs, sites.as<uint64_t>(), n_sites, counts.as<uint32_t>(), ctx->ingest_tid_to_contig.as<uint32_t>(), n_ref, ctx->genome,
	                                                      min_alt, min_percent, all_rows.as<agpu_indel_row>(), row_flag.as<uint8_t>(), words.as<unsigned long long>()); }
	TRY(with_temporary(ctx, temporary_storage, "indel rocprim::select(rows)", n_runs * (sizeof(agpu_indel_row) + 1) + n_flagged * sizeof(agpu_indel_row), [&](void* storage, size_t& bytes) {
		return rocprim::select(storage, bytes, all_rows.as<agpu_indel_row>(), row_flag.as<uint8_t>(), rows.as<agpu_indel_row>(), n_out.as<uint64_t>(), (size_t) n_runs, s); }));
	state.note_peak();
	TRY(end_pass(PASS_ROWS));
	uint64_t n_rows = 0; unsigned long long counted_records = 0;
	HIP_CHECK(hipMemcpyAsync(&n_rows, n_out.ptr, 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipMemcpyAsync(host_words, words.ptr, sizeof(host_words), hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipMemcpyAsync(&counted_records, counting.contributing.ptr, 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	if (counted_records != state.stats.contributing) { // (the counter kernel applies the same filter as the event passes)
		set_last_error("agpu_indel_sites: internal error: the counters come from " + std::to_string(counted_records) + " records, the events from " + std::to_string(state.stats.contributing));
		return AGPU_ERR_DEVICE;
	}
	if (host_words[WORD_SUPPORT] != n_events || host_words[WORD_NO_SITE] != 0) {
		set_last_error("agpu_indel_sites: internal error: the supports add up to " + std::to_string(host_words[WORD_SUPPORT]) + " of " + std::to_string(n_events) + " events, " + std::to_string(host_words[WORD_NO_SITE]) + " candidates without their site");
		return AGPU_ERR_DEVICE;
	}
	if (n_rows > n_flagged) { set_last_error("agpu_indel_sites: internal error: " + std::to_string(n_rows) + " rows of " + std::to_string(n_flagged) + " candidates"); return AGPU_ERR_DEVICE; }
	state.stats.reported = n_rows;
	state.rows.resize(n_rows);
	if (n_rows > 0) { HIP_CHECK(hipMemcpyAsync(state.rows.data(), rows.ptr, n_rows * sizeof(agpu_indel_row), hipMemcpyDeviceToHost, s)); HIP_CHECK(hipStreamSynchronize(s)); }
	return AGPU_OK;
}

}

extern "C" {

int agpu_indel_sites(agpu_ctx* ctx, const uint32_t* ref_length, uint32_t n_ref, uint32_t min_mapq, uint32_t min_alt, uint32_t min_percent, const agpu_indel_row** rows, uint64_t* n_rows, agpu_indel_stats* stats) {
	if (!ctx || !rows || !n_rows || (n_ref > 0 && !ref_length)) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	*rows = nullptr; *n_rows = 0;
	if (stats) memset(stats, 0, sizeof(*stats));
	if (min_mapq > 255) { set_last_error("agpu_indel_sites: a threshold above 255"); return AGPU_ERR_INVALID; }
	if (min_alt < 1 || min_alt > 0x7FFFFFFFu) { set_last_error("agpu_indel_sites: min_alt is 1 to 2^31-1"); return AGPU_ERR_INVALID; }
	if (min_percent > 100) { set_last_error("agpu_indel_sites: min_percent is 0 to 100"); return AGPU_ERR_INVALID; }
	ResidentStream resident;
	TRY(resident_stream(ctx, "agpu_indel_sites", "indel sites of one sample over several GPUs are not supported", nullptr, resident, NEEDS_GENOME | NEEDS_REFERENCES, n_ref));
	HIP_CHECK(hipSetDevice(ctx->device));
	IndelState& state = ctx->indel;
	memset(&state.stats, 0, sizeof(state.stats));
	state.rows.clear(); state.peak = 0;
	const int status = one_shot<2 * PASSES>(ctx, state, "agpu_indel_sites", [&](hipEvent_t* events) {
		const int found = find(ctx, resident, ref_length, n_ref, min_mapq, min_alt, min_percent, events);
		(void) hipStreamSynchronize(ctx->stream); // (the events of a call that ended early have happened)
		if (found == AGPU_OK) for (int k = 0; k < PASSES; ++k) { float ms = 0; if (hipEventElapsedTime(&ms, events[2 * k], events[2 * k + 1]) == hipSuccess) state.stats.seconds[k] = ms / 1000.0; }
		return found;
	}, [&](int) { state.stats.peak_bytes = state.peak; state.release_all(); });
	if (stats) *stats = state.stats; // (also of a call that failed: what it had counted)
	if (status != AGPU_OK) { state.rows.clear(); return status; }
	*rows = state.rows.data(); *n_rows = state.rows.size();
	return AGPU_OK;
}

int agpu_indel_sites_allocated_bytes(agpu_ctx* ctx, uint64_t* bytes) {
	if (!ctx || !bytes) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	*bytes = ctx->indel.allocated();
	return AGPU_OK;
}

}
