// arriba_amd/csrc/device/agpu_context.hpp -- device context: owns every HBM buffer of the hot path.
#ifndef AGPU_CONTEXT_HPP
#define AGPU_CONTEXT_HPP 1

#include <hip/hip_runtime.h>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <utility>
#include <string>
#include <vector>
#include "../../../include/arriba_gpu.h"
#include "evalue_core.hpp"
#include "event_core.hpp"

namespace agpu {

void set_last_error(const std::string& message);

bool debug_allocation_fails(); // agpu_api.hip: a test asked for the next allocation inside agpu_ingest_finish to fail once (agpu_debug_fail_allocation_in_finish)
void note_failed_allocation(size_t bytes);
bool debug_finish_runs_out_of_memory(struct ::agpu_ctx* ctx); // agpu_api.hip: agpu_debug_exhaust_memory_in_finish // agpu_api.hip: the size asked for and what the device has free go into the next "hipMalloc failed" message of this thread
struct DeviceBuffer {
	void* ptr = nullptr;
	size_t bytes = 0;
	DeviceBuffer() {}
	DeviceBuffer(const DeviceBuffer&) = delete;
	DeviceBuffer& operator=(const DeviceBuffer&) = delete;
	~DeviceBuffer() { release(); }
	// grow-only: a buffer that is already large enough is reused, so that repeated passes over batches of the same size
	// (and the stage calls inside one pass) do not go back to hipMalloc/hipFree; `bytes` is the size asked for last
	size_t capacity = 0;
	bool allocate(size_t n) {
		if (n == 0) n = 16;
		if (ptr != nullptr && n <= capacity) { bytes = n; return true; }
		release();
		if (debug_allocation_fails() || hipMalloc(&ptr, n) != hipSuccess) {
			// out of memory: the contexts give back what they only keep for the next sample (the stream and the tables of the last ingest while the stages run, the
			// buffers of the stages while an ingest runs), then once more
			(void) hipGetLastError();
			ptr = nullptr;
			if (!release_idle_buffers() || hipMalloc(&ptr, n) != hipSuccess) { (void) hipGetLastError(); ptr = nullptr; note_failed_allocation(n); return false; }
		}
		bytes = n; capacity = n;
		return true;
	}
	static bool release_idle_buffers(); // agpu_api.hip; true if anything was given back
	// a view of a part of another buffer (find_fusions carves its working arrays out of a buffer that is idle at that point): nothing is freed with it
	bool borrowed = false;
	void borrow(void* memory, size_t n) { release(); ptr = memory; bytes = n; capacity = n; borrowed = true; }
	void release() {
		if (!ptr) return;
		if (!borrowed) (void) hipFree(ptr);
		ptr = nullptr; bytes = 0; capacity = 0; borrowed = false;
	}
	void swap(DeviceBuffer& other) { std::swap(ptr, other.ptr); std::swap(bytes, other.bytes); std::swap(capacity, other.capacity); std::swap(borrowed, other.borrowed); }
	template <class T> T* as() const { return (T*) ptr; }
};

// per-kernel timing with HIP events on the launch stream (agpu_set_profiling / agpu_get_kernel_profile)
struct KernelSample { const char* name; hipEvent_t start, stop; uint64_t bytes; float ms; unsigned int epoch; };

// The front of read_chimeric_alignments on the device while the pieces of the file are still arriving (agpu_ingest.hip, "the front as the pieces arrive"): the stream is
// cut into windows, one per pushed piece; a window goes through four steps on a stream of its own (record chain; offsets, record keys, active records; runs of one name;
// the loop body of the reference per name), each step behind the read-back of the few words the next one needs to size its launches.  The thread that pushes never waits
// for them: a step is enqueued when the words of the one before have arrived (hipEventQuery).
struct IngestWindow {
	uint64_t avail = 0;                     // bytes of the stream in HBM when the window was made: the size of the stream for its kernels
	uint64_t segment_begin = 0, segment_end = 0;
	bool last = false;                      // made by agpu_ingest_finish: reaches to the end of the stream
	int enqueued = 0, known = 0;            // steps enqueued / steps whose words were read
	hipEvent_t readback = nullptr;          // behind the read-back of the step enqueued last
	unsigned int slot = 0;                  // of the ring of read-back words
	uint64_t record_begin = 0, record_end = 0, active_begin = 0, active_end = 0, head_begin = 0, head_end = 0;
};
struct IngestProgress {
	bool on = false, abandoned = false, touched = false; // abandoned: something the windows cannot decide (a read name in two places, a record longer than the margin, ...): the whole stream is done again at the end
	hipStream_t work = nullptr;
	std::deque<IngestWindow> windows;
	std::vector<hipEvent_t> events;         // free ones
	uint32_t* host_words = nullptr;         // pinned, INGEST_WINDOW_RING x INGEST_WINDOW_WORDS
	unsigned int next_slot = 0;
	uint64_t window_bytes = 0;              // bytes of the stream the last window was made at
	uint64_t segments_done = 0, records = 0, active = 0, heads = 0, groups_done = 0, size_hint = 0;
	unsigned int windows_made = 0;
};

}

enum { AGPU_PIECE_SLOTS = 4 };
namespace agpu {
// The scratch buffers of a context, addressed by name, grow-only.  Two contexts of one device may share a pool (agpu_create_sibling): the lanes of a resident session that feeds
// the file of the next sample while the stages of the current one run (include/arriba_workflow.h: arriba_workflow_submit).  The two never use the same names at the same time -- one
// is between agpu_ingest_begin and agpu_ingest_finish ("ingest.*", the stream, the raw pieces), the other in its stages -- so ~150 GB of tables exist once, not twice.
struct ScratchPool {
	std::mutex mutex; // (of the map: buffers are looked up from the thread that feeds and from the thread that runs the stages)
	std::map<std::string, DeviceBuffer> buffers;
	DeviceBuffer& get(const char* name) { std::lock_guard<std::mutex> lock(mutex); return buffers[name]; }
};
struct PoolSlots { DeviceBuffer* slot[AGPU_PIECE_SLOTS]; DeviceBuffer& operator[](size_t k) { return *slot[k]; } };
// A view of the record stream that the last ingest left in HBM, as the guard in front of every consumer hands it out (resident_stream.hpp: resident_stream)
struct ResidentStream { const uint8_t* stream = nullptr; uint64_t stream_size = 0, first_record = 0, records = 0; const uint64_t* record_offset = nullptr; };
// What every consumer of that stream keeps with its context: buffers of its own, addressed by name -- not in the pool the lanes of a session share, not among the buffers that
// change hands between them (take_sample_buffers), not given back under memory pressure (release_ingest_buffers) -- and `active`: set while the consumer reads the stream, when
// nothing of the context may be given back (DeviceBuffer::release_idle_buffers asks every consumer of the context: each one enters itself in the list it is constructed with)
struct StreamConsumer {
	explicit StreamConsumer(std::vector<const StreamConsumer*>& of_context) { of_context.push_back(this); }
	StreamConsumer(const StreamConsumer&) = delete; StreamConsumer& operator=(const StreamConsumer&) = delete;
	std::map<std::string, DeviceBuffer> buffers;
	DeviceBuffer& buffer(const char* name) { return buffers[name]; }
	void release_all() { for (std::map<std::string, DeviceBuffer>::iterator b = buffers.begin(); b != buffers.end(); ++b) b->second.release(); }
	void release_prefix(const char* prefix) { for (std::map<std::string, DeviceBuffer>::iterator b = buffers.begin(); b != buffers.end(); ++b) if (b->first.compare(0, strlen(prefix), prefix) == 0) b->second.release(); }
	void release_all_but(const char* kept) { for (std::map<std::string, DeviceBuffer>::iterator b = buffers.begin(); b != buffers.end(); ++b) if (b->first != kept) b->second.release(); }
	uint64_t allocated() const { uint64_t sum = 0; for (std::map<std::string, DeviceBuffer>::const_iterator b = buffers.begin(); b != buffers.end(); ++b) sum += b->second.capacity; return sum; }
	bool active = false;
	uint64_t peak = 0;
	void note_peak() { const uint64_t now = allocated(); if (now > peak) peak = now; }
};
// --supporting-alignments (agpu_supporting.hip): the records of the listed read names, copied out of the stream behind the ingest, until the rows of fusions.tsv are known.  The
// pool of a sample ("support.*") lives until agpu_support_pool_release or the next build on the context.
struct SupportState : StreamConsumer {
	using StreamConsumer::StreamConsumer;
	void release_all() { StreamConsumer::release_all(); built = false; }
	bool built = false, strip_hit_index = false, index_ready = false;
	uint64_t n_names = 0, table_slots = 0, records = 0 /* of the pool */, bytes = 0; uint32_t hash_bits = 64;
	// between agpu_supporting_begin and agpu_supporting_end
	uint32_t n_rows = 0; uint64_t emissions = 0, blocks = 0, window_blocks = 0, next_block = 0, gathered_block = ~0ull, index_first = 0;
	std::vector<uint64_t> row_first, row_bytes, row_block_begin, row_out_offset; // [n_rows + 1]: first record, payload bytes, first block, first byte of the framed blocks
};
// --virus-expression (agpu_virus.hip): the "virus.*" buffers live inside one agpu_virus_expression; what the call returns stays in host memory here
struct VirusState : StreamConsumer {
	using StreamConsumer::StreamConsumer;
	std::vector<uint64_t> reads, covered, kmer_count, shared; std::vector<uint32_t> active_slots;
};
// --coverage (agpu_depth.hip): the "depth.*" buffers live from agpu_depth_begin to agpu_depth_end
struct DepthState : StreamConsumer {
	using StreamConsumer::StreamConsumer;
	uint32_t n_ref = 0;
	uint64_t slots = 0, window = 0, text_window = 0; // slots of the array of depths; positions per window of runs; bytes per window of text
	uint64_t next_slot = 0;                           // where the next window of positions begins
	bool carry = false;                               // a run is open at next_slot (its first slot is in "depth.carry")
	uint64_t batch_begin = 0, batch_end = 0, batch_runs = 0; // the text of the runs found last: bytes [batch_begin, batch_end) of the file
	uint64_t written = 0, flushed = 0;                // bytes of the file that are in the staging window or were fetched; bytes fetched
	agpu_depth_stats stats = {};
	hipEvent_t events[2] = { nullptr, nullptr };
};
// --mark-duplicates (agpu_markdup.hip): all of "markdup.*" but "markdup.flag" (one byte per record) is released before agpu_sorted_bam_begin allocates "sortedbam.*", that one
// by agpu_sorted_bam_end.  It runs inside agpu_sorted_bam_begin: sorted_bam_active of the context stands for its `active`
struct MarkdupState : StreamConsumer {
	using StreamConsumer::StreamConsumer;
	bool next = false, on = false; // agpu_sorted_bam_set_mark_duplicates: of the next agpu_sorted_bam_begin; of the begin ... end under way
	agpu_markdup_counts counts = {};
};
// --gene-counts (agpu_genecount.hip): the "genecount.*" buffers live inside one agpu_gene_counts
struct GenecountState : StreamConsumer {
	using StreamConsumer::StreamConsumer;
	agpu_gene_count_stats stats = {};
};
// --splice-junctions (agpu_junctions.hip): the "junction.*" buffers live inside one agpu_splice_junctions; the rows stay until the next call
struct JunctionState : StreamConsumer {
	using StreamConsumer::StreamConsumer;
	agpu_junction_stats stats = {};
	std::vector<agpu_junction_row> rows;
};
// --allele-counts (agpu_alleles.hip): the "allele.*" buffers live inside one agpu_allele_counts; the rows stay until the next call
struct AlleleState : StreamConsumer {
	using StreamConsumer::StreamConsumer;
	agpu_allele_stats stats = {};
	std::vector<agpu_allele_row> rows;
};
// --variant-sites (agpu_variants.hip): the "variant.*" buffers live inside one agpu_variant_sites; the rows stay until the next call
struct VariantState : StreamConsumer {
	using StreamConsumer::StreamConsumer;
	agpu_variant_stats stats = {};
	std::vector<agpu_variant_row> rows;
};
// --indel-sites (agpu_indels.hip): the "indel.*" buffers live inside one agpu_indel_sites; the rows stay until the next call
struct IndelState : StreamConsumer {
	using StreamConsumer::StreamConsumer;
	agpu_indel_stats stats = {};
	std::vector<agpu_indel_row> rows;
};
// --realign-reads (agpu_realign.hip): the "realign.*" buffers live between agpu_realign_begin and _end
struct RealignState : StreamConsumer {
	using StreamConsumer::StreamConsumer;
	ResidentStream stream; // of agpu_realign_begin, for the windows of text behind it
	bool paired = false, want_kept = false, wave_form = true;
	uint32_t n_ref = 0;
	uint64_t records = 0, window = 0, launch_items = 0; // records of the stream; bytes of a window of text; work-items of a launch
	uint64_t total[2] = { 0, 0 }, flushed[2] = { 0, 0 }; // bytes of the two files; bytes of them that were fetched
	agpu_realign_stats stats = {};
	hipEvent_t events[2] = { nullptr, nullptr };
};
// --rna-metrics (agpu_rnametrics.hip): the copy of the region track ("rnametrics.track.*") stays from the first agpu_rna_metrics that brings it until another track comes or the
// context goes; the counter block and the lengths live inside one call
struct RnametricsState : StreamConsumer {
	using StreamConsumer::StreamConsumer;
	uint64_t track_id = 0; // of the track on the device (0: none)
	agpu_region_track track = {}; // ... with device pointers
	agpu_rna_metrics_stats stats = {};
};
}
struct agpu_ctx {
	explicit agpu_ctx(std::shared_ptr<agpu::ScratchPool> shared = std::shared_ptr<agpu::ScratchPool>()) : pool(shared ? shared : std::make_shared<agpu::ScratchPool>()),
		ingest_stream(pool->get("ingest.stream")), coverage_windows32(pool->get("ingest.coverage_windows32")) {
		static const char* const raw[AGPU_PIECE_SLOTS] = { "ingest.raw0", "ingest.raw1", "ingest.raw2", "ingest.raw3" }; static const char* const blocks[AGPU_PIECE_SLOTS] = { "ingest.blocks0", "ingest.blocks1", "ingest.blocks2", "ingest.blocks3" };
		for (int k = 0; k < AGPU_PIECE_SLOTS; ++k) { ingest_raw.slot[k] = &pool->get(raw[k]); ingest_blocks.slot[k] = &pool->get(blocks[k]); }
	}
	agpu_ctx(const agpu_ctx&) = delete; agpu_ctx& operator=(const agpu_ctx&) = delete;
	int device = 0;
	hipStream_t stream = nullptr;
	hipEvent_t event_start = nullptr, event_stop = nullptr;
	float last_ms = 0;
	uint64_t last_bytes = 0;
	agpu_params params;
	bool profiling = false;
	// launches are timed from the thread that runs the stages and, in a session with two lanes, from the thread that feeds this context: profile_mutex guards the three vectors;
	// agpu_set_profiling starts a new epoch, samples of an older one are dropped when their events have completed
	std::mutex profile_mutex;
	unsigned int profile_epoch = 0;
	std::vector<agpu::KernelSample> samples_pending, samples_done;
	std::vector<hipEvent_t> event_pool;
	// scratch buffers of the stage calls, kept between calls (grow-only) and addressed by name
	std::shared_ptr<agpu::ScratchPool> pool;
	agpu::DeviceBuffer& scratch(const char* name) { return pool->get(name); }
	bool keeps_batch_buffers = false; // agpu_keep_batch_buffers: the lanes of a session do not hand the batch over (agpu_api.hip: take_sample_buffers)
	agpu_ctx* sibling = nullptr; // agpu_create_sibling: the other lane of a session (shares `pool`; the buffers of a sample change hands in agpu_ingest_finish: take_sample_buffers)

	// annotation
	uint32_t n_genes = 0, n_exons = 0, n_dummy = 0;
	agpu::DeviceBuffer gene_contig, gene_start, gene_end, gene_bits, gene_exonic_length;
	agpu::DeviceBuffer exon_start, exon_end, exon_gene, exon_previous, exon_next, exon_cds_start, exon_cds_end;
	agpu::DeviceBuffer exon_index_contig_offset, exon_index_keys, exon_index_member_offset, exon_index_members, exon_index_bins;
	agpu::DeviceBuffer gene_index_contig_offset, gene_index_keys, gene_index_member_offset, gene_index_members, gene_index_bins;
	agpu::DeviceBuffer dummy_start_key, dummy_end_key;
	agpu::AnnotationView annotation;
	bool have_annotation = false;

	// genome
	agpu::DeviceBuffer genome_contig_offset, genome_contig_bits, genome_bases;
	agpu::GenomeView genome;
	std::vector<uint8_t> host_contig_bits;
	std::vector<uint64_t> host_contig_offset;
	bool have_genome = false;

	// batch
	uint64_t n = 0;
	agpu::DeviceBuffer n_aln, fbits, filter, group;
	agpu::DeviceBuffer pristine_fbits, pristine_abits[3]; // state as uploaded, restored by agpu_reset
	agpu::DeviceBuffer contig[3], start[3], end[3], abits[3], cigar_offset[3], cigar_count[3], cigar_pool;
	agpu::DeviceBuffer seq_offset[2], seq_length[2], seq_pool;
	agpu::DeviceBuffer gene_count[3], genes[3], gene_pool, counters;
	std::string failed_launch; // the first kernel launch of the sample that the runtime refused (KernelTimer), or empty
	agpu::BatchView batch;
	uint64_t batch_input_bytes = 0;
	uint32_t max_read_length = 0;
	bool have_batch = false, annotated = false, stage1_done = false, stage2_done = false, annotate_begun = false;
	uint32_t n_unmapped = 0;
	// the read lists of the candidates this rank built, kept when the replicated table is imported (agpu_import_candidates)
	agpu::DeviceBuffer owned_list_offset, owned_read_lists, owned_global_index;
	uint32_t n_owned = 0; uint64_t n_owned_list_entries = 0;
	bool candidates_imported = false, owned_index_set = false, multimappers_begun = false;
	uint64_t n_multimappers_global = 0;
	// coverage_t (agpu_upload_coverage)
	agpu::DeviceBuffer coverage_window_offset, coverage_windows, coverage_fragment_starts, coverage_fragment_ends;
	agpu::CoverageView coverage = { 0, nullptr, nullptr, nullptr, nullptr };
	bool have_coverage = false;
	// read_chimeric_alignments on the device (agpu_ingest.hip): the uncompressed BAM stream while it is being pushed, and what stays behind the pack
	agpu::DeviceBuffer& ingest_stream; agpu::PoolSlots ingest_raw, ingest_blocks; agpu::DeviceBuffer& coverage_windows32; // (in the pool: shared by the lanes of a session)
	agpu::DeviceBuffer ingest_tid_to_contig, ingest_viral_counts;
	agpu::DeviceBuffer names, name_offset; // "QNAME,HI" of every fragment of a batch built on the device
	uint64_t ingest_stream_size = 0, ingest_first_record = 0, names_size = 0;
	uint32_t ingest_n_targets = 0, ingest_max_itd_length = 100, ingest_pushes = 0, ingest_host_buffers = 2;
	uint8_t ingest_external_duplicate_marking = 0;
	bool ingest_active = false, ingest_finishing = false /* inside agpu_ingest_finish: its tables are in use although the feed is over */, batch_from_ingest = false, ingest_part_of_sample = false, ingest_verify_crc = false, ingest_deflated_pieces = false /* a piece of this ingest went through bgzf_inflate_kernel */;
	bool ingest_sam = false; uint32_t sam_n_targets = 0, sam_table_mask = 0; // the pieces of this ingest are SAM text (agpu_sam.hip: agpu_ingest_sam_targets uploaded the @SQ names to "sam.names" / "sam.name_offset" / "sam.table")
	agpu::DeviceBuffer ingest_qname_keys; uint64_t ingest_qname_runs = 0; // a part of a sample: 128-bit keys of the runs of read names in its stream
	// -c (agpu_separate_adopt / agpu_separate_merge): the role of the ingest under way; the batch of pass C as the block agpu_shard_export makes of it, the name keys of its fragments
	// (ascending) and the fragment of every key; what pass C reported
	uint8_t ingest_role = 0; bool separate_adopted = false;
	agpu::DeviceBuffer separate_block, separate_keys, separate_rows; uint64_t separate_block_bytes = 0, separate_n = 0, separate_names_at = 0, separate_name_offset_at = 0;
	agpu_ingest_result separate_result;
	agpu_ingest_result ingest_result; uint64_t ingest_pool_sizes[2] = { 0, 0 }; // what the last ingest (or merge of parts) reported; CIGAR words and sequence bytes of its pools
	agpu::IngestProgress ingest_progress;
	// --sorted-bam (agpu_sorted_bam.hip): the stream of the last ingest as agpu_ingest_finish left it (it zeroes ingest_stream_size) -- valid until the next agpu_ingest_begin on this
	// context or its sibling; and where the output is between agpu_sorted_bam_begin and agpu_sorted_bam_end
	uint64_t last_ingest_stream_size = 0, last_ingest_first_record = 0, last_ingest_records = 0;
	bool last_ingest_kept = false, last_ingest_part_of_sample = false, sorted_bam_active = false, sorted_bam_index_ready = false;
	uint64_t sorted_bam_records = 0, sorted_bam_bytes = 0, sorted_bam_blocks = 0, sorted_bam_window_blocks = 0, sorted_bam_next_block = 0, sorted_bam_gathered_block = ~0ull, sorted_bam_index_first = 0;
	uint64_t sorted_bam_chunks = 0, sorted_bam_intervals = 0, sorted_bam_no_coor = 0; uint32_t sorted_bam_n_ref = 0;
	int sorted_bam_level_next = 0, sorted_bam_level = 0; // agpu_sorted_bam_set_compression: of the next agpu_sorted_bam_begin; of the begin ... end under way
	uint64_t sorted_bam_compressed_bytes = 0;            // of the windows fetched so far
	agpu::ResidentStream sorted_bam_stream;              // of agpu_sorted_bam_begin, for the gathers behind it
	// the other consumers of that stream: each enters itself in `consumers` (which therefore stands in front of them)
	std::vector<const agpu::StreamConsumer*> consumers;
	bool consumer_active() const { for (size_t k = 0; k < consumers.size(); ++k) if (consumers[k]->active) return true; return false; }
	agpu::SupportState support{consumers};       // --supporting-alignments (agpu_supporting.hip)
	agpu::VirusState virus{consumers};           // --virus-expression (agpu_virus.hip)
	agpu::DepthState depth{consumers};           // --coverage (agpu_depth.hip)
	agpu::MarkdupState markdup{consumers};       // --mark-duplicates (agpu_markdup.hip)
	agpu::GenecountState genecount{consumers};   // --gene-counts (agpu_genecount.hip)
	agpu::JunctionState junction{consumers};     // --splice-junctions (agpu_junctions.hip)
	agpu::AlleleState allele{consumers};         // --allele-counts (agpu_alleles.hip)
	agpu::RnametricsState rnametrics{consumers}; // --rna-metrics (agpu_rnametrics.hip)
	agpu::VariantState variant{consumers};       // --variant-sites (agpu_variants.hip)
	agpu::IndelState indel{consumers};           // --indel-sites (agpu_indels.hip)
	agpu::RealignState realign{consumers};       // --realign-reads (agpu_realign.hip)
	// A pushed piece: copied on the context's stream (piece_copied: the caller's buffer is free), unwrapped and CRC-checked on a stream of its own (piece_stream; piece_ready: its
	// bytes are in the stream, piece_done: the raw bytes are not needed any more), so that the copy of the next piece never waits for a kernel; AGPU_PIECE_SLOTS raw buffers in turn
	hipStream_t piece_stream = nullptr, piece_stream2 = nullptr /* deflated pieces take the two in turn */; hipEvent_t piece_copied[AGPU_PIECE_SLOTS] = {}, piece_ready[AGPU_PIECE_SLOTS] = {}, piece_done[AGPU_PIECE_SLOTS] = {};
	std::vector<uint64_t> host_coverage_window_offset;
	agpu::DeviceBuffer gather_ids, gather_cigar_base, gather_seq_base, gather_name_base; // agpu_gather_rows_begin -> _copy
	uint64_t gather_n = 0, gather_sizes[3] = { 0, 0, 0 };
	bool gather_all = false;
	// closest genomic breakpoints per candidate (agpu_mark_genomic_support); not marked: every candidate -1
	agpu::DeviceBuffer cand_closest1, cand_closest2;
	bool genomic_support_marked = false;
	uint32_t n_selected = 0, selected_of_candidates = 0xFFFFFFFFu; // agpu_select_candidates: how many, and of which table (scratch "select.ids" holds them)
	uint32_t confidence_candidates = 0xFFFFFFFFu; // n_candidates of the last agpu_assign_confidence (its result stays in scratch "events.confidence")
	agpu::GenomicSupport genomic_support() { agpu::GenomicSupport wgs = { genomic_support_marked ? cand_closest1.as<int32_t>() : nullptr, genomic_support_marked ? cand_closest2.as<int32_t>() : nullptr }; return wgs; }
	uint64_t annotation_serial = 1, gene_read_counts_of_annotation = 0; // every annotate of a batch takes a new serial; scratch "events.gene_read_count" holds the counts of that one
	std::vector<uint32_t> host_gene_read_counts;
	uint64_t global_n = 0; // fragments of the whole sample when this context holds one shard of it (agpu_set_shard); 0 = not sharded
	// One sample over the GPUs of a node with the reads sharded (agpu_shard_keep, include/arriba_gpu.h): the candidate table and every read list are here (global name ranks), the reads
	// of the other ranks are not; what a walk over read lists asks of a read is replicated, one byte per fragment of the SAMPLE (agpu_read_state_import): scratch "sharded.filter"
	// (the filter ids) and "sharded.bits" (WALK_MULTIMAPPER | WALK_EXONIC) -- agpu_api.hip: candidate_walk_batch
	bool read_sharded = false, state_imported = false, sample_gene_read_counts_set = false;
	uint32_t n_clipped_entries = 0; // agpu_in_vitro_clipped_mates -> agpu_copy_in_vitro_clipped_mates (scratch "sharded.clipped_entries")

	// scratch
	agpu::DeviceBuffer unmapped_keys, sort_scratch, sorted_keys, scan_flags, scan_ids;
	agpu::DeviceBuffer viral_pairs;
	uint64_t viral_pair_capacity = 0;
	agpu::DeviceBuffer duplicate_keys, duplicate_slots, duplicate_entries;
	uint32_t n_duplicate_entries = 0;
	agpu::DeviceBuffer sample_flags, sample_values, samples;
	agpu::DeviceBuffer stage_counts;

	// find_fusions
	agpu::DeviceBuffer emissions, discordant_swapped;
	agpu::DeviceBuffer cand_gene1, cand_gene2, cand_contigs, cand_breakpoint1, cand_breakpoint2, cand_flags, cand_filter, cand_split_reads1, cand_split_reads2, cand_discordant_mates;
	agpu::DeviceBuffer cand_anchor1, cand_anchor2, cand_list_offset, cand_read_lists, cand_evalue, cand_iteration_rank, cand_votes, cand_first_occurrence, cand_extra_split_list;
	agpu::DeviceBuffer evalue_support_scale, evalue_intragenic_support, evalue_intergenic_support, evalue_distance_tables;
	agpu::EvalueGlobals evalue_globals;
	bool evalue_done = false, iteration_order_done = false;

	// k-mer index + splice sites (filter_mismappers)
	agpu::DeviceBuffer kmer_contig_table, kmer_offsets, kmer_positions, splice_offset, splice_sites, splice_bits;
	uint32_t kmer_positions_count = 0, splice_sites_for_dummy = 0, mismapper_jobs = 0, mismapper_heavy = 0, mismapper_leftover = 0;
	bool kmer_index_done = false, have_splice_sites = false, mismapper_jobs_ready = false;
	agpu::CandidateTable candidates;
	uint32_t n_emissions = 0, n_candidates = 0, n_queued_buckets = 0, n_discordant_emissions = 0; uint64_t n_list_entries = 0;
	// implicit discordant-mate lists (fusion_core.hpp: CandidateTable::discordant_before): where the windows of candidates are cut, what the expansion of a list needs again
	bool lists_implicit = false; std::vector<uint32_t> list_window_cuts; uint64_t list_window_entries = 0; int32_t lists_max_mate_gap = 0; uint32_t lists_n_bucket_rows = 0;
	bool fusions_done = false;

	// tables
	agpu::DeviceBuffer mismatch_verdict, kmer_threshold, filter_enabled, viral_verdict_top, viral_verdict_low;
	agpu::FilterTables tables;
	uint64_t genome_size = 0;
};

namespace agpu {

// agpu_ingest.hip: the stream and the per-record tables of the last ingest given back to the device (they are kept for the next sample as long as memory allows); true if there were any
bool release_ingest_buffers(agpu_ctx* ctx);
// agpu_ingest.hip, for the pushes of agpu_sam.hip: room for `needed` bytes in the stream (it moves when it grows), and what every push ends with (the caller's buffer of the push
// before is free, the windows of the front go on over what has arrived)
int ingest_grow_stream(agpu_ctx* ctx, uint64_t needed);
int ingest_piece_pushed(agpu_ctx* ctx);
// agpu_sam.hip, for agpu_ingest_finish: AGPU_ERR_INVALID with "failed to load alignments: SAM line N: <reason>" if a line of the SAM text of this ingest was malformed
int sam_ingest_verdict(agpu_ctx* ctx);
// agpu_markdup.hip, for agpu_sorted_bam_begin: one byte per record of the stream of the last ingest (MDUP_FLAG_MASK or 0) into "markdup.flag", everything else of "markdup.*" released
int markdup_find(agpu_ctx* ctx, const ResidentStream& stream);
// agpu_api.hip: the buffers that hold a sample (batch, gene sets, candidates, read lists, k-mer index, ...) change hands between the lanes of a session: `ctx`, about to build
// its batch, takes what its sibling -- whose sample is done on the device -- holds wherever that is the larger buffer; the sibling's sample is gone afterwards
void take_sample_buffers(agpu_ctx* ctx, bool batch_group = true, bool stage_group = true);
// agpu_api.hip: what follows the columns of a batch, whoever filled them (agpu_upload_batch, or the ingest on the device: agpu_ingest.hip)
int finish_batch_setup(agpu_ctx* ctx);
// agpu_api.hip: the batch a stage sees that judges CANDIDATES by their read lists.  One context with all reads: its own batch (with walk bytes made now, if asked for).  The reads
// sharded over the ranks: a view of the global_n fragments of the sample that holds the replicated filters (and the walk bytes made from them) and NOTHING else -- a stage that
// wants more of a read runs where the read is.  pull_filters_of_own_reads: behind a stage that changed filters of reads through that view (the same on every rank).
int candidate_walk_batch(agpu_ctx* ctx, BatchView& batch, bool with_walk_bytes);
int pull_filters_of_own_reads(agpu_ctx* ctx);

// Brackets one kernel launch (or library call) with HIP events when profiling is on.  Usage:
//   { KernelTimer timer(ctx, "stage2_kernel", bytes); stage2_kernel<<<...>>>(...); }
struct KernelTimer {
	agpu_ctx* ctx; bool armed;
	hipStream_t stream;
	KernelSample sample;
	const char* launched;
	KernelTimer(agpu_ctx* c, const char* name, uint64_t bytes, hipStream_t on = nullptr) : ctx(c), armed(false), stream(on ? on : c->stream), launched(name) {
		if (!ctx->profiling) return;
		sample.name = name; sample.bytes = bytes; sample.ms = 0; sample.start = nullptr; sample.stop = nullptr;
		{ std::lock_guard<std::mutex> lock(ctx->profile_mutex);
		  sample.epoch = ctx->profile_epoch;
		  hipEvent_t* events[2] = { &sample.start, &sample.stop };
		  for (int k = 0; k < 2; ++k) if (!ctx->event_pool.empty()) { *events[k] = ctx->event_pool.back(); ctx->event_pool.pop_back(); } }
		if ((sample.start == nullptr && hipEventCreate(&sample.start) != hipSuccess) || (sample.stop == nullptr && hipEventCreate(&sample.stop) != hipSuccess)) return;
		(void) hipEventRecord(sample.start, stream);
		armed = true;
	}
	~KernelTimer() {
		// a launch that the runtime refused (a grid of more than 2^32 work-items, too much LDS) says so only here: noted with the context, and the sample fails where its results are
		// picked (agpu_select_candidates) instead of going on with whatever the kernel's output buffer held
		const hipError_t refused = hipGetLastError();
		if (refused != hipSuccess) { std::lock_guard<std::mutex> lock(ctx->profile_mutex); if (ctx->failed_launch.empty()) ctx->failed_launch = std::string(launched) + ": " + hipGetErrorString(refused); }
		if (!armed) return;
		(void) hipEventRecord(sample.stop, stream);
		std::lock_guard<std::mutex> lock(ctx->profile_mutex);
		ctx->samples_pending.push_back(sample);
	}
};
// the stages that walk the read lists of the candidates (agpu_fusions.hip: implicit discordant lists)
// whose lists a stage reads: an expansion of implicit lists skips the candidates the stage does not look at (their part of the window holds nothing, or zeros with zero_fill --
// for a stage that strides over the entries of a window without asking whose they are)
enum { LISTS_OF_ALL = 0, LISTS_OF_UNFILTERED = 1, LISTS_OF_IN_VITRO = 2 /* in_vitro_looks_at */, LISTS_OF_BOTH_SPLICED = 3 /* both_spliced_is_member */ };
int for_each_list_window(agpu_ctx* ctx, const std::function<int(const CandidateTable&, uint32_t, uint32_t)>& stage, int lists_of = LISTS_OF_ALL, bool zero_fill = false);
int recut_list_windows(agpu_ctx* ctx);
// resolve the pending samples whose events have completed (the caller has synchronised the streams it launched on; what another thread launched meanwhile stays pending)
inline void collect_kernel_samples(agpu_ctx* ctx) {
	std::lock_guard<std::mutex> lock(ctx->profile_mutex);
	size_t kept = 0;
	for (size_t k = 0; k < ctx->samples_pending.size(); ++k) {
		KernelSample sample = ctx->samples_pending[k];
		if (hipEventQuery(sample.stop) == hipErrorNotReady) { ctx->samples_pending[kept++] = sample; continue; }
		if (hipEventElapsedTime(&sample.ms, sample.start, sample.stop) != hipSuccess) sample.ms = 0;
		ctx->event_pool.push_back(sample.start); ctx->event_pool.push_back(sample.stop);
		if (sample.epoch == ctx->profile_epoch) ctx->samples_done.push_back(sample);
	}
	ctx->samples_pending.resize(kept);
}

}

#endif
