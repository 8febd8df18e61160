// arriba_amd/csrc/device/agpu_realign.hip -- --realign-reads on the MI355X: the record stream of the last ingest split into the templates that must be aligned again and the
// templates that are passed on, both as SAM text, fields 1-11 (include/arriba_gpu.h: agpu_realign_begin / _next / _end).  What decides a byte is realign_core.hpp, which the host
// steps as well (arriba_amd/csrc/host/realign_split.cpp); the rule is DESIGN.md 4.18.  Here are
//   realign_name_kernel      paired-end only, one lane per record: its QNAME into the open-addressing table of markdup_core.hpp, and, if it is primary, its claim on its slot
//                            (atomicMin of the record number) -- the name pass of agpu_genecount.hip
//   realign_verdict_kernel   one lane per record: what the record is to the split (dropped, extra, orphan, mate, owner).  The owner of a template -- its slot-0 record, or every
//                            primary record of a single-end stream -- evaluates both ends and writes the byte length of the template's lines into the column of the file it goes
//                            to; the other column stays 0, which IS the verdict.  The statistics are summed over the wavefront first: one atomic per wavefront and word
//   rocPRIM exclusive scans  of the two length columns (32-bit in, 64-bit out): where the lines of each template begin in its file.  Templates go by the rank of their owner, so
//                            the order does not depend on the schedule, and the id the name table hands out appears nowhere in it
//   realign_bound_kernel     one lane: the records whose lines touch a window of text, by binary search in the scanned offsets
//   realign_text_kernel      the bytes of a staging window.  <false>: one lane per template writes all bytes of its lines that fall into the window.  <true>: the lane writes
//                            fields 1-9, and the 64 lanes of the wavefront write SEQ, tab, QUAL and newline of one of their templates after the other, 64 bytes at a time (a
//                            leader loop over the lanes that hold a template): neighbouring lanes store neighbouring bytes
// Byte and integer work bound by dependent loads (record_offset -> the head of the record -> its fields) and by the byte stores of the text; no MFMA, no LDS.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <rocprim/rocprim.hpp>
#define AGPU_OPTION "--realign-reads"
#include "resident_stream.hpp"
#include "device_utils.hpp"
#include "realign_core.hpp"

using namespace agpu;

namespace {

const uint64_t DEFAULT_TEXT_WINDOW = 16ull << 20;  // bytes of a staging window

enum { COUNT_TEMPLATES = 0, COUNT_REALIGN = 1, COUNT_KEPT = 2, COUNT_ORPHANS = 3, COUNT_DROPPED = 4, COUNT_EXTRA = 5, COUNT_PLACEHOLDER = 6, COUNT_MALFORMED = 7, COUNT_REALIGN_BYTES = 8, COUNT_KEPT_BYTES = 9,
       COUNT_WORDS = 10 }; // 64-bit words

struct RealignInput {
	const uint8_t* stream; uint64_t stream_size;
	const uint64_t* record_offset; uint64_t n;
	const uint8_t* in_assembly; RealignNames names;
	bool paired;
};

// records [first, upto)
__global__ void __launch_bounds__(BLOCK) realign_name_kernel(const uint8_t* __restrict__ stream, uint64_t stream_size, const uint64_t* __restrict__ record_offset, uint64_t first, uint64_t upto, unsigned long long* table, uint64_t slots,
		uint32_t hash_bits, uint32_t* name_id, uint32_t* slot_first) {
	const uint64_t r = first + (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	if (r >= upto) return;
	uint32_t id = MDUP_NONE;
	const uint64_t at = record_offset[r];
	if (at + 36 <= stream_size) {
		id = mdup_name_insert(table, slots, stream, stream_size, record_offset, (uint32_t) r, hash_bits);
		const uint32_t flags = sbam_load16(stream, at + 18);
		if (id != MDUP_NONE && mdup_primary(flags)) atomicMin(&slot_first[2ull * id + mdup_slot(flags)], (uint32_t) r);
	}
	name_id[r] = id;
}

// records [first, upto).  length[file][r] (zeroed in front of the kernel) gets the bytes of the template that record r owns, mate_of[r] its slot-1 record.  No lane leaves before the
// sums over the wavefront.
__global__ void __launch_bounds__(BLOCK) realign_verdict_kernel(RealignInput in, const uint32_t* __restrict__ name_id, const uint32_t* __restrict__ slot_first, uint64_t first, uint64_t upto, uint32_t* length_realign,
		uint32_t* length_kept /* may be null */, uint32_t* mate_of, unsigned long long* counters) {
	const uint64_t r = first + (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	// 16 bits each (a wavefront adds at most 128 to a field): templates, realign, kept, orphans | dropped, extra, placeholders, malformed
	unsigned long long templates = 0, others = 0, realign_bytes = 0, kept_bytes = 0;
	if (r < upto) {
		const RealignRecord own = realign_parse(in.stream, in.record_offset[r], in.stream_size, in.names.n_ref);
		uint32_t first0 = MDUP_NONE, first1 = MDUP_NONE;
		bool named = true;
		if (own.valid && in.paired) {
			const uint32_t id = name_id[r];
			if (id == MDUP_NONE) named = false; else { first0 = slot_first[2ull * id]; first1 = slot_first[2ull * id + 1]; }
		}
		if (!own.valid || !named) others |= 1ull << 48;
		else switch (realign_role(own.flag, in.paired, (uint32_t) r, first0, first1)) {
			case REALIGN_ROLE_DROPPED: others |= 1ull; break;
			case REALIGN_ROLE_EXTRA: others |= 1ull << 16; break;
			case REALIGN_ROLE_ORPHAN: templates |= 1ull | 1ull << 48; break;
			case REALIGN_ROLE_MATE: break;
			default: {
				RealignRecord mate = own;
				if (in.paired) mate = realign_parse(in.stream, in.record_offset[first1], in.stream_size, in.names.n_ref);
				if (!mate.valid) { others |= 1ull << 48; break; }
				const RealignVerdict v = realign_verdict(in.stream, own, mate, in.paired, in.in_assembly, in.names);
				if (v.bytes > 0xFFFFFFFFull) { others |= 1ull << 48; break; }
				templates |= 1ull;
				others |= (unsigned long long) v.placeholders << 32;
				if (in.paired) mate_of[r] = first1;
				if (v.file == REALIGN_FILE_REALIGN) { templates |= 1ull << 16; realign_bytes = v.bytes; length_realign[r] = (uint32_t) v.bytes; }
				else { templates |= 1ull << 32; kept_bytes = v.bytes; if (length_kept != nullptr) length_kept[r] = (uint32_t) v.bytes; }
			}
		}
	}
	templates = wave_sum(templates); others = wave_sum(others); realign_bytes = wave_sum(realign_bytes); kept_bytes = wave_sum(kept_bytes);
	if ((threadIdx.x & 63) == 0) {
		for (int k = 0; k < 4; ++k) {
			const unsigned long long a = (templates >> (16 * k)) & 0xFFFFull, b = (others >> (16 * k)) & 0xFFFFull;
			if (a != 0) atomicAdd(&counters[COUNT_TEMPLATES + k], a);
			if (b != 0) atomicAdd(&counters[COUNT_DROPPED + k], b);
		}
		if (realign_bytes != 0) atomicAdd(&counters[COUNT_REALIGN_BYTES], realign_bytes);
		if (kept_bytes != 0) atomicAdd(&counters[COUNT_KEPT_BYTES], kept_bytes);
	}
}

// offset[0 .. n] ascends from 0, offset[n] >= upto > from.  out[0]: the record whose lines hold byte `from` (the last r with offset[r] <= from); out[1]: the first r with
// offset[r] >= upto
__global__ void realign_bound_kernel(const uint64_t* __restrict__ offset, uint64_t n, uint64_t from, uint64_t upto, uint64_t* out) {
	if (blockIdx.x != 0 || threadIdx.x != 0) return;
	uint64_t low = 0, high = n + 1; // the first index with offset > from
	while (low < high) { const uint64_t middle = low + (high - low) / 2; if (offset[middle] <= from) low = middle + 1; else high = middle; }
	out[0] = low > 0 ? low - 1 : 0;
	low = 0; high = n; // the first index with offset >= upto
	while (low < high) { const uint64_t middle = low + (high - low) / 2; if (offset[middle] < upto) low = middle + 1; else high = middle; }
	out[1] = low;
}

// byte `at` of the file goes to staging[at - from] if from <= at < upto (upto - from is at most the size of the staging window)
struct StagingPut {
	uint8_t* staging; uint64_t at, from, upto;
	__device__ __forceinline__ void operator()(uint8_t byte) { if (at >= from && at < upto) staging[at - from] = byte; ++at; }
};

// records [first, last): those whose template has lines in bytes [from, upto) of the file that `offset` belongs to
template <bool WAVE> __global__ void __launch_bounds__(BLOCK) realign_text_kernel(RealignInput in, const uint64_t* __restrict__ offset, const uint32_t* __restrict__ mate_of, uint64_t first, uint64_t last, uint64_t from, uint64_t upto,
		uint8_t* staging) {
	const uint64_t r = first + (uint64_t) blockIdx.x * BLOCK + threadIdx.x;
	bool mine = r < last;
	uint64_t begin = 0;
	if (mine) { begin = offset[r]; const uint64_t end = offset[r + 1]; mine = end > begin && end > from && begin < upto; }
	StagingPut put = { staging, begin, from, upto };
	if (!WAVE) {
		if (!mine) return;
		for (int slot = 0; slot < (in.paired ? 2 : 1); ++slot) {
			const RealignRecord record = realign_parse(in.stream, in.record_offset[slot == 0 ? r : mate_of[r]], in.stream_size, in.names.n_ref);
			if (record.valid) realign_line(in.stream, record, in.names, put);
		}
		return;
	}
	const uint32_t lane = threadIdx.x & 63u;
	for (int slot = 0; slot < (in.paired ? 2 : 1); ++slot) { // (in.paired is the same in every lane)
		RealignTail tail; tail.seq_at = 0; tail.l_seq = 0; tail.no_qual = 1;
		bool have = false;
		if (mine) {
			const RealignRecord record = realign_parse(in.stream, in.record_offset[slot == 0 ? r : mate_of[r]], in.stream_size, in.names.n_ref);
			if (record.valid) { realign_head(in.stream, record, in.names, put); tail = realign_tail_of(in.stream, record); have = true; }
		}
		const uint64_t tail_at = put.at;
		if (have) put.at += realign_tail_bytes(tail);
		unsigned long long todo = __ballot(have && tail_at < upto && put.at > from);
		while (todo != 0) { // (todo is the same in every lane)
			const int leader = __ffsll((long long) todo) - 1;
			RealignTail theirs;
			theirs.seq_at = __shfl((unsigned long long) tail.seq_at, leader); theirs.l_seq = __shfl(tail.l_seq, leader); theirs.no_qual = __shfl(tail.no_qual, leader);
			const uint64_t at = __shfl((unsigned long long) tail_at, leader), bytes = realign_tail_bytes(theirs);
			const uint64_t k_begin = at < from ? from - at : 0, k_end = at + bytes > upto ? upto - at : bytes;
			for (uint64_t k = k_begin + lane; k < k_end; k += 64) staging[at + k - from] = realign_tail_byte(in.stream, theirs, k);
			todo &= todo - 1;
		}
	}
}

void note_peak(RealignState& state) { state.stats.peak_bytes = std::max<uint64_t>(state.stats.peak_bytes, state.allocated()); }
// behind a hipStreamSynchronize: the milliseconds between the two events of the state go to seconds[part]
void add_seconds(RealignState& state, int part) { float ms = 0; if (hipEventElapsedTime(&ms, state.events[0], state.events[1]) == hipSuccess) state.stats.seconds[part] += ms / 1000.0; }

RealignInput input_of(agpu_ctx* ctx) {
	RealignState& state = ctx->realign;
	RealignInput in;
	in.stream = state.stream.stream; in.stream_size = state.stream.stream_size; in.record_offset = state.stream.record_offset; in.n = state.records;
	in.in_assembly = state.buffer("realign.in_assembly").as<uint8_t>();
	in.names.names = state.buffer("realign.names").as<char>(); in.names.name_offset = state.buffer("realign.name_offset").as<uint32_t>(); in.names.n_ref = state.n_ref;
	in.paired = state.paired;
	return in;
}

// the name pass, the verdict pass and the scans
int split(agpu_ctx* ctx, const uint8_t* in_assembly, const char* names, const uint32_t* name_offset, uint32_t n_ref) {
	hipStream_t s = ctx->stream;
	RealignState& state = ctx->realign;
	const uint64_t size = state.stream.stream_size, n = state.stream.records, name_bytes = n_ref > 0 ? name_offset[n_ref] : 0;
	const uint8_t* stream = state.stream.stream;
	const uint64_t* record_offset = state.stream.record_offset;
	state.records = n; state.n_ref = n_ref; state.paired = false;
	state.window = knob_of("ARRIBA_REALIGN_TEXT_WINDOW", DEFAULT_TEXT_WINDOW, 1ull << 31);
	state.launch_items = (knob_of("ARRIBA_REALIGN_LAUNCH_ITEMS", LAUNCH_ITEMS, LAUNCH_ITEMS) + BLOCK - 1) / BLOCK * BLOCK; // (whole blocks: no record is visited twice)
	{ const char* form = getenv("ARRIBA_REALIGN_TEXT_FORM"); state.wave_form = !(form != nullptr && strcmp(form, "lane") == 0); }
	state.total[0] = state.total[1] = state.flushed[0] = state.flushed[1] = 0;
	memset(&state.stats, 0, sizeof(state.stats));
	DeviceBuffer& assembly = state.buffer("realign.in_assembly"); DeviceBuffer& name_text = state.buffer("realign.names"); DeviceBuffer& name_at = state.buffer("realign.name_offset");
	DeviceBuffer& counters = state.buffer("realign.counters"); DeviceBuffer& bound = state.buffer("realign.bound"); DeviceBuffer& staging = state.buffer("realign.staging");
	DeviceBuffer& length_realign = state.buffer("realign.length_realign"); DeviceBuffer& length_kept = state.buffer("realign.length_kept");
	DeviceBuffer& offset_realign = state.buffer("realign.offset_realign"); DeviceBuffer& offset_kept = state.buffer("realign.offset_kept"); DeviceBuffer& mate_of = state.buffer("realign.mate_of");
	ALLOC(assembly, std::max<size_t>(n_ref, 1)); ALLOC(name_text, std::max<uint64_t>(name_bytes, 1)); ALLOC(name_at, ((size_t) n_ref + 1) * 4); ALLOC(counters, COUNT_WORDS * 8); ALLOC(bound, 16);
	ALLOC(staging, state.window); ALLOC(length_realign, (n + 1) * 4); ALLOC(offset_realign, (n + 1) * 8);
	if (state.want_kept) { ALLOC(length_kept, (n + 1) * 4); ALLOC(offset_kept, (n + 1) * 8); }
	// the layout: bit 0x1 of the first record
	if (n > 0) {
		uint64_t at = 0; uint8_t flag[2] = { 0, 0 };
		HIP_CHECK(hipMemcpyAsync(&at, record_offset, 8, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		if (at > size || size - at < 36) { set_last_error("agpu_realign_begin: failed to load alignments (the first record is cut short)"); return AGPU_ERR_INVALID; }
		HIP_CHECK(hipMemcpyAsync(flag, stream + at + 18, 2, hipMemcpyDeviceToHost, s));
		HIP_CHECK(hipStreamSynchronize(s));
		state.paired = (flag[0] & 1u) != 0;
	}
	if (state.paired) ALLOC(mate_of, n * 4);
	if (n_ref > 0) {
		HIP_CHECK(hipMemcpyAsync(assembly.ptr, in_assembly, n_ref, hipMemcpyHostToDevice, s));
		HIP_CHECK(hipMemcpyAsync(name_at.ptr, name_offset, ((size_t) n_ref + 1) * 4, hipMemcpyHostToDevice, s));
		if (name_bytes > 0) HIP_CHECK(hipMemcpyAsync(name_text.ptr, names, name_bytes, hipMemcpyHostToDevice, s));
	} else HIP_CHECK(hipMemsetAsync(name_at.ptr, 0, 4, s));
	HIP_CHECK(hipStreamSynchronize(s)); // (the sources are pageable memory of the caller)
	HIP_CHECK(hipMemsetAsync(counters.ptr, 0, COUNT_WORDS * 8, s));
	HIP_CHECK(hipMemsetAsync(length_realign.ptr, 0, (n + 1) * 4, s));
	if (state.want_kept) HIP_CHECK(hipMemsetAsync(length_kept.ptr, 0, (n + 1) * 4, s));
	note_peak(state);
	// the name pass
	DeviceBuffer& name_id = state.buffer("realign.name_id"); DeviceBuffer& slot_first = state.buffer("realign.slot_first"); DeviceBuffer& table = state.buffer("realign.table");
	HIP_CHECK(hipEventRecord(state.events[0], s));
	if (state.paired) {
		const uint64_t slots = support_table_slots(n);
		ALLOC(name_id, n * 4); ALLOC(slot_first, n * 8); ALLOC(table, slots * 8);
		note_peak(state);
		HIP_CHECK(hipMemsetAsync(slot_first.ptr, 0xFF, n * 8, s));
		HIP_CHECK(hipMemsetAsync(table.ptr, 0, slots * 8, s));
		KernelTimer timer(ctx, "realign_name_kernel", n * 64 + slots * 8);
		for (uint64_t first = 0; first < n; first += state.launch_items) {
			const uint64_t upto = std::min(n, first + state.launch_items);
			realign_name_kernel<<<grid_for(upto - first), BLOCK, 0, s>>>(stream, size, record_offset, first, upto, table.as<unsigned long long>(), slots, hash_bits_knob("ARRIBA_REALIGN_HASH_BITS"), name_id.as<uint32_t>(), slot_first.as<uint32_t>());
		}
	}
	HIP_CHECK(hipEventRecord(state.events[1], s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	add_seconds(state, 0);
	// the verdict pass
	const RealignInput in = input_of(ctx);
	HIP_CHECK(hipEventRecord(state.events[0], s));
	if (n > 0) { KernelTimer timer(ctx, "realign_verdict_kernel", n * 24 + n * 64);
	  for (uint64_t first = 0; first < n; first += state.launch_items) {
		const uint64_t upto = std::min(n, first + state.launch_items);
		realign_verdict_kernel<<<grid_for(upto - first), BLOCK, 0, s>>>(in, name_id.as<uint32_t>(), slot_first.as<uint32_t>(), first, upto, length_realign.as<uint32_t>(), state.want_kept ? length_kept.as<uint32_t>() : nullptr,
		  mate_of.as<uint32_t>(), counters.as<unsigned long long>());
	  } }
	HIP_CHECK(hipEventRecord(state.events[1], s));
	unsigned long long host_counters[COUNT_WORDS] = {};
	HIP_CHECK(hipMemcpyAsync(host_counters, counters.ptr, sizeof(host_counters), hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	add_seconds(state, 1);
	name_id.release(); slot_first.release(); table.release(); // (the claims live on in realign.mate_of)
	if (host_counters[COUNT_MALFORMED] != 0) { set_last_error("agpu_realign_begin: failed to load alignments (a record is cut short, has no name or names a reference the header does not have)"); return AGPU_ERR_INVALID; }
	// the scans
	HIP_CHECK(hipEventRecord(state.events[0], s));
	TRY(with_temporary(ctx, state.buffer("realign.rocprim"), "realign rocprim::exclusive_scan(realign bytes)", (n + 1) * 12, [&](void* t, size_t& b) { return rocprim::exclusive_scan(t, b, length_realign.as<uint32_t>(), offset_realign.as<uint64_t>(), (uint64_t) 0, (size_t) n + 1, rocprim::plus<uint64_t>(), s); }));
	if (state.want_kept) TRY(with_temporary(ctx, state.buffer("realign.rocprim"), "realign rocprim::exclusive_scan(kept bytes)", (n + 1) * 12, [&](void* t, size_t& b) { return rocprim::exclusive_scan(t, b, length_kept.as<uint32_t>(), offset_kept.as<uint64_t>(), (uint64_t) 0, (size_t) n + 1, rocprim::plus<uint64_t>(), s); }));
	note_peak(state);
	uint64_t totals[2] = { 0, 0 };
	HIP_CHECK(hipMemcpyAsync(&totals[0], offset_realign.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, s));
	if (state.want_kept) HIP_CHECK(hipMemcpyAsync(&totals[1], offset_kept.as<uint64_t>() + n, 8, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipEventRecord(state.events[1], s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	add_seconds(state, 2);
	length_realign.release(); length_kept.release(); state.buffer("realign.rocprim").release();
	agpu_realign_stats& stats = state.stats;
	stats.records = n; stats.templates = host_counters[COUNT_TEMPLATES]; stats.realign_templates = host_counters[COUNT_REALIGN]; stats.kept_templates = host_counters[COUNT_KEPT]; stats.orphans = host_counters[COUNT_ORPHANS];
	stats.dropped_secondary = host_counters[COUNT_DROPPED]; stats.extra = host_counters[COUNT_EXTRA]; stats.placeholder_cigar = host_counters[COUNT_PLACEHOLDER];
	stats.realign_bytes = host_counters[COUNT_REALIGN_BYTES]; stats.kept_bytes = host_counters[COUNT_KEPT_BYTES]; stats.layout = state.paired ? 1 : 0;
	if (totals[0] != stats.realign_bytes || (state.want_kept && totals[1] != stats.kept_bytes)) { set_last_error("agpu_realign_begin: the scanned line lengths and their sums differ"); return AGPU_ERR_DEVICE; }
	state.total[0] = totals[0]; state.total[1] = totals[1];
	return AGPU_OK;
}

void leave(agpu_ctx* ctx) {
	RealignState& state = ctx->realign;
	(void) hipStreamSynchronize(ctx->stream);
	for (int k = 0; k < 2; ++k) if (state.events[k]) { (void) hipEventDestroy(state.events[k]); state.events[k] = nullptr; }
	state.release_all();
	state.active = false;
}

}

extern "C" {

int agpu_realign_begin(agpu_ctx* ctx, const uint8_t* in_assembly, const char* names, const uint32_t* name_offset, uint32_t n_ref, int want_kept, agpu_realign_info* info) {
	if (!ctx || !info || (n_ref > 0 && (!in_assembly || !names || !name_offset))) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	memset(info, 0, sizeof(*info));
	ResidentStream resident;
	TRY(resident_stream(ctx, "agpu_realign_begin", "a split for realignment of one sample over several GPUs is not supported", ctx->realign.active ? "agpu_realign_end must run first" : nullptr, resident));
	if (n_ref != ctx->ingest_n_targets) { set_last_error("agpu_realign_begin: the references are not those of the header of the last ingest"); return AGPU_ERR_INVALID; }
	for (uint32_t t = 0; t < n_ref; ++t) if (name_offset[t + 1] < name_offset[t]) { set_last_error("agpu_realign_begin: the offsets of the names must ascend"); return AGPU_ERR_INVALID; }
	HIP_CHECK(hipSetDevice(ctx->device));
	ctx->realign.active = true; // (the stream is read from here on: nothing of this context is given back when an allocation fails)
	ctx->realign.want_kept = want_kept != 0; ctx->realign.stream = resident;
	struct Guard { agpu_ctx* ctx; bool keep; ~Guard() { if (!keep) leave(ctx); } } guard = { ctx, false };
	for (int k = 0; k < 2; ++k) HIP_CHECK(hipEventCreate(&ctx->realign.events[k]));
	const int status = split(ctx, in_assembly, names, name_offset, n_ref);
	collect_kernel_samples(ctx);
	if (status != AGPU_OK) return status;
	{ std::lock_guard<std::mutex> lock(ctx->profile_mutex); if (!ctx->failed_launch.empty()) { set_last_error("agpu_realign_begin: " + ctx->failed_launch); return AGPU_ERR_DEVICE; } }
	info->window_bytes = ctx->realign.window; info->realign_bytes = ctx->realign.stats.realign_bytes; info->kept_bytes = ctx->realign.stats.kept_bytes; info->layout = ctx->realign.stats.layout;
	guard.keep = true;
	return AGPU_OK;
}

int agpu_realign_next(agpu_ctx* ctx, int which, void* pinned, uint64_t capacity, uint64_t* bytes) {
	if (!ctx || !bytes) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	RealignState& state = ctx->realign;
	*bytes = 0;
	if (!state.active) { set_last_error("agpu_realign_begin must run first"); return AGPU_ERR_INVALID; }
	if (which != REALIGN_FILE_REALIGN && which != REALIGN_FILE_KEPT) { set_last_error("agpu_realign_next: the file is 0 (realign) or 1 (kept)"); return AGPU_ERR_INVALID; }
	if (which == REALIGN_FILE_KEPT && !state.want_kept) { set_last_error("agpu_realign_next: the kept templates were not asked for (want_kept of agpu_realign_begin)"); return AGPU_ERR_INVALID; }
	if (!pinned || capacity < state.window) { set_last_error("agpu_realign_next: the buffer is smaller than a window (agpu_realign_info.window_bytes)"); return AGPU_ERR_INVALID; }
	const uint64_t from = state.flushed[which], upto = std::min(state.total[which], from + state.window), n = state.records;
	if (from >= upto) return AGPU_OK;
	HIP_CHECK(hipSetDevice(ctx->device));
	hipStream_t s = ctx->stream;
	struct Collect { agpu_ctx* ctx; ~Collect() { collect_kernel_samples(ctx); } } collect = { ctx };
	const uint64_t* offset = state.buffer(which == REALIGN_FILE_REALIGN ? "realign.offset_realign" : "realign.offset_kept").as<uint64_t>();
	uint64_t range[2] = { 0, 0 };
	HIP_CHECK(hipEventRecord(state.events[0], s));
	{ KernelTimer timer(ctx, "realign_bound_kernel", 1024);
	  realign_bound_kernel<<<1, 64, 0, s>>>(offset, n, from, upto, state.buffer("realign.bound").as<uint64_t>()); }
	HIP_CHECK(hipMemcpyAsync(range, state.buffer("realign.bound").ptr, 16, hipMemcpyDeviceToHost, s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	if (range[0] > range[1] || range[1] > n) { set_last_error("agpu_realign_next: the records of a window of text are out of range"); return AGPU_ERR_DEVICE; }
	const RealignInput in = input_of(ctx);
	{ KernelTimer timer(ctx, state.wave_form ? "realign_text_kernel<wave>" : "realign_text_kernel<lane>", (range[1] - range[0]) * 24 + 2 * (upto - from));
	  for (uint64_t first = range[0]; first < range[1]; first += state.launch_items) {
		const uint64_t last = std::min(range[1], first + state.launch_items);
		if (state.wave_form) realign_text_kernel<true><<<grid_for(last - first), BLOCK, 0, s>>>(in, offset, state.buffer("realign.mate_of").as<uint32_t>(), first, last, from, upto, state.buffer("realign.staging").as<uint8_t>());
		else realign_text_kernel<false><<<grid_for(last - first), BLOCK, 0, s>>>(in, offset, state.buffer("realign.mate_of").as<uint32_t>(), first, last, from, upto, state.buffer("realign.staging").as<uint8_t>());
	  } }
	{ KernelTimer timer(ctx, "realign copy back", upto - from);
	  HIP_CHECK(hipMemcpyAsync(pinned, state.buffer("realign.staging").ptr, upto - from, hipMemcpyDeviceToHost, s)); }
	HIP_CHECK(hipEventRecord(state.events[1], s));
	HIP_CHECK(hipStreamSynchronize(s));
	HIP_CHECK(hipGetLastError());
	add_seconds(state, 3);
	state.flushed[which] = upto;
	*bytes = upto - from;
	return AGPU_OK;
}

int agpu_realign_end(agpu_ctx* ctx, agpu_realign_stats* stats) {
	if (!ctx) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	if (stats) memset(stats, 0, sizeof(*stats));
	if (!ctx->realign.active) return AGPU_OK;
	(void) hipSetDevice(ctx->device);
	if (stats) *stats = ctx->realign.stats;
	leave(ctx);
	collect_kernel_samples(ctx);
	return AGPU_OK;
}

int agpu_realign_allocated_bytes(agpu_ctx* ctx, uint64_t* bytes) {
	if (!ctx || !bytes) { set_last_error("null argument"); return AGPU_ERR_INVALID; }
	*bytes = ctx->realign.allocated();
	return AGPU_OK;
}

}
