// arriba_amd/csrc/host/host_capi.cpp -- C ABI of the host driver library (include/arriba_host.h) and the
// sequential scalar stages that sit between the device stages of the hot path.
#include "../../../include/arriba_host.h"
#include "arriba_host.h"
#include "output.h"
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <atomic>
#include <cstdio>
#include <cstring>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <iostream>
#include <list>
#include <map>
#include <memory>
#include <set>
#include <stdexcept>
#include <tuple>
#include <unordered_map>

#include "../device/sorted_bam_core.hpp"
using namespace arriba;

namespace {
thread_local std::string g_error;
const char* const DEFAULT_GTF_FEATURES = "gene_name=gene_name|gene_id gene_id=gene_id transcript_id=transcript_id feature_exon=exon feature_CDS=CDS";
}

struct ahost_session {
	IngestOptions options;
	Contigs contigs;
	Assembly assembly;
	Annotation annotation;
	FlatIndex exon_index, gene_index;
	IngestResult ingest;
	bool have_batch = false;
	Tags tags; std::vector<ProteinDomain> protein_domains; FlatIndex protein_domain_index;
	std::vector<agpu_genomic_breakpoint> genomic_breakpoints;
	std::vector<agpu_range_rule> range_rules[2]; // [0] known fusions, [1] blacklist (keywords allowed)

	// flattened tables backing the views
	std::vector<uint16_t> gene_contig; std::vector<int32_t> gene_start, gene_end, gene_exonic_length; std::vector<uint8_t> gene_bits;
	std::vector<int32_t> exon_start, exon_end, exon_previous, exon_next, exon_cds_start, exon_cds_end; std::vector<uint32_t> exon_gene;
	std::vector<uint64_t> genome_offset; std::vector<uint8_t> contig_bits; std::string genome_bases;
	agpu_annotation_view annotation_view;
	agpu_genome_view genome_view;
	agpu_coverage_view coverage_view;
	std::vector<uint64_t> coverage_offset; std::vector<uint16_t> coverage_windows; std::vector<uint8_t> coverage_starts, coverage_ends;
	void build_coverage_view() { // coverage_t of the ingest, the windows of all contigs concatenated
		const Coverage& c = ingest.coverage;
		const size_t n = c.coverage.size();
		coverage_offset.assign(n + 1, 0); coverage_windows.clear(); coverage_starts.clear(); coverage_ends.clear();
		for (size_t contig = 0; contig < n; ++contig) {
			coverage_offset[contig] = coverage_windows.size();
			coverage_windows.insert(coverage_windows.end(), c.coverage[contig].begin(), c.coverage[contig].end());
			coverage_starts.insert(coverage_starts.end(), c.fragment_starts[contig].begin(), c.fragment_starts[contig].end());
			coverage_ends.insert(coverage_ends.end(), c.fragment_ends[contig].begin(), c.fragment_ends[contig].end());
			if (coverage_starts.size() != coverage_windows.size() || coverage_ends.size() != coverage_windows.size()) throw std::runtime_error("coverage_t: windows and flags differ in length");
		}
		coverage_offset[n] = coverage_windows.size();
		coverage_view.n_contigs = (uint32_t) n; coverage_view.window_offset = coverage_offset.data(); coverage_view.coverage = coverage_windows.data();
		coverage_view.fragment_starts = coverage_starts.data(); coverage_view.fragment_ends = coverage_ends.data();
	}
	agpu_batch_view batch_view, slice_view;
	// device ingest: the open file and what agpu_ingest_begin needs from its header
	BamFeed* feed = nullptr;
	bool device_batch = false;           // the fragments live on the device (ahost_adopt_device_ingest)
	std::vector<std::string> last_target_names; // the reference names of the header of the last ahost_bam_open
	std::vector<std::string> separate_target_names; // -c: the reference names of the separate chimeric file, which those of the main alignments must equal (ahost_bam_open_role)
	Batch spare_rows;                    // the vectors of the last sample's rows (ahost_set_batch_rows), kept over ahost_bam_open for the next sample's
	// ahost_detach_sample: a writer thread holds what a sample left behind while the session reads the next one.  It shares the reference data of the session that no sample changes
	// (annotation, assembly, tags, protein domains) and takes a copy of `contigs` -- ahost_bam_open stores the names of the next header there
	std::mutex detached_mutex; std::condition_variable detached_changed; unsigned int detached_samples = 0; // (the mutex also guards spare_rows; ahost_close waits for the count)
	bool sample_was_detached = false;    // ... and the session holds no sample until its next ingest
	std::string formatted_rows;          // ahost_format_fusions: the rows of this rank's share of an output file, until the next call
	std::vector<uint32_t> row_fragments; // device ingest: the fragment of every row of ingest.batch (ascending); empty = the batch holds every fragment
	bool rows_in_list_order = false;     // ... or row k holds the fragment of entry k of the read lists of the table written next (ahost_set_batch_rows without fragments)
	std::vector<uint32_t> tid_to_contig;
	std::vector<uint64_t> window_offset;
	std::vector<WrittenRow> written_rows; std::vector<uint32_t> written_candidate; std::vector<int32_t> written_ref, written_breakpoint; // --supporting-alignments: the data rows of the last fusions file (not the discarded one) in their order
	std::vector<uint8_t> input_header, sorted_bam_header_framed; std::vector<uint32_t> sorted_bam_ref_length; // --sorted-bam: the head of the file of the last ahost_bam_open; what ahost_sorted_bam_header made of it
	~ahost_session() { if (feed) close_bam_feed(feed); }
	std::map<std::pair<contig_t, contig_t>, bool> related_viruses;
	std::string name_scratch;
	size_t contigs_at_open = 0; // the contigs of the assembly and the annotation: ids below this were not learnt from the header of an input
	std::map<std::string, std::unique_ptr<RegionTrack> > region_tracks; std::mutex region_track_mutex; // --rna-metrics: a track per interval file ("" = none), built when first asked for

	void build_reference_views() {
		size_t G = annotation.genes.size(), E = annotation.exons.size();
		gene_contig.resize(G); gene_start.resize(G); gene_end.resize(G); gene_exonic_length.resize(G); gene_bits.resize(G);
		for (size_t g = 0; g < G; ++g) {
			const GeneRecord& r = annotation.genes[g];
			gene_contig[g] = r.contig; gene_start[g] = r.start; gene_end[g] = r.end; gene_exonic_length[g] = r.exonic_length;
			gene_bits[g] = (r.strand ? AGPU_GBIT_STRAND : 0) | (r.is_dummy ? AGPU_GBIT_DUMMY : 0) | (r.is_protein_coding ? AGPU_GBIT_PROTEIN_CODING : 0);
		}
		exon_start.resize(E); exon_end.resize(E); exon_previous.resize(E); exon_next.resize(E); exon_cds_start.resize(E); exon_cds_end.resize(E); exon_gene.resize(E);
		for (size_t e = 0; e < E; ++e) {
			const ExonRecord& r = annotation.exons[e];
			exon_start[e] = r.start; exon_end[e] = r.end; exon_previous[e] = r.previous_exon; exon_next[e] = r.next_exon;
			exon_cds_start[e] = r.coding_region_start; exon_cds_end[e] = r.coding_region_end; exon_gene[e] = r.gene;
		}
		agpu_annotation_view& v = annotation_view;
		v.n_genes = G; v.gene_contig = gene_contig.data(); v.gene_start = gene_start.data(); v.gene_end = gene_end.data(); v.gene_bits = gene_bits.data(); v.gene_exonic_length = gene_exonic_length.data();
		v.n_exons = E; v.exon_start = exon_start.data(); v.exon_end = exon_end.data(); v.exon_gene = exon_gene.data(); v.exon_previous = exon_previous.data(); v.exon_next = exon_next.data();
		v.exon_cds_start = exon_cds_start.data(); v.exon_cds_end = exon_cds_end.data();
		fill_index_view(exon_index, v.exon_index);
		fill_index_view(gene_index, v.gene_index);
	}
	static void fill_index_view(const FlatIndex& index, agpu_flat_index& view) {
		view.n_contigs = index.n_contigs(); view.contig_offset = index.contig_offset.data();
		view.n_keys = index.keys.size(); view.keys = index.keys.data();
		view.member_offset = index.member_offset.data(); view.n_members = index.members.size(); view.members = index.members.data();
	}
	void build_genome_view() { // contigs may have been added by the BAM header
		size_t C = contigs.size();
		genome_offset.assign(C + 1, 0); contig_bits.assign(C, 0); genome_bases.clear();
		std::vector<std::string> name_by_id(C);
		for (std::map<std::string, contig_t>::const_iterator c = contigs.by_name.begin(); c != contigs.by_name.end(); ++c) name_by_id[c->second] = c->first;
		for (size_t c = 0; c < C; ++c) {
			genome_offset[c] = genome_bases.size();
			if (assembly.has(c)) genome_bases += assembly.sequence[c];
			contig_bits[c] = (is_interesting_contig(name_by_id[c], options.interesting_contigs) ? AGPU_CBIT_INTERESTING : 0) | (is_interesting_contig(name_by_id[c], options.viral_contigs) ? AGPU_CBIT_VIRAL : 0);
		}
		genome_offset[C] = genome_bases.size();
		genome_bases.append(16, '\0'); // padding behind the last base (not part of the view): consumers may read the genome several bases at a time
		genome_view.n_contigs = C; genome_view.contig_offset = genome_offset.data(); genome_view.contig_bits = contig_bits.data(); genome_view.bases = genome_bases.data();
	}
	void build_batch_view() {
		const Batch& b = ingest.batch;
		agpu_batch_view& v = batch_view;
		v.n = b.n; v.n_aln = b.n_aln.data(); v.fbits = b.fbits.data(); v.group = b.group.data();
		for (int s = 0; s < 3; ++s) {
			v.contig[s] = b.contig[s].data(); v.start[s] = b.start[s].data(); v.end[s] = b.end[s].data(); v.abits[s] = b.abits[s].data();
			v.cigar_offset[s] = b.cigar_offset[s].data(); v.cigar_count[s] = b.cigar_count[s].data();
		}
		v.cigar_pool_size = b.cigar_pool.size(); v.cigar_pool = b.cigar_pool.data();
		for (int s = 0; s < 2; ++s) { v.seq_offset[s] = b.seq_offset[s].data(); v.seq_length[s] = b.seq_length[s].data(); }
		v.seq_pool_size = b.seq_pool.size(); v.seq_pool = b.seq_pool.data();
	}
};

namespace {

int ingest(ahost_session* session, ByteSource* source_raw, int external_duplicate_marking, unsigned int max_itd_length) {
	std::unique_ptr<ByteSource> source(source_raw);
	try {
		session->options.external_duplicate_marking = external_duplicate_marking != 0;
		session->options.max_itd_length = max_itd_length;
		session->ingest = IngestResult(); session->sample_was_detached = false;
		session->row_fragments.clear(); session->device_batch = false; session->rows_in_list_order = false;
		read_chimeric_alignments(*source, session->assembly, session->contigs, session->annotation, session->gene_index, session->options, session->ingest);
		session->build_genome_view();
		session->build_batch_view();
		session->have_batch = true;
		return 0;
	} catch (const std::exception& e) {
		g_error = e.what();
		return -1;
	}
}

// reference: kmer_to_int, source/filter_mismappers.cpp:33-45
unsigned int kmer_to_int(const std::string& sequence, size_t position, int kmer_length) {
	unsigned int result = 0;
	for (int base = 0; base < kmer_length; ++base) {
		result = result << 2;
		switch (sequence.c_str()[position + base]) {
			case 'T': result += 0; break;
			case 'G': result += 1; break;
			case 'C': result += 2; break;
			default: result += 3; break;
		}
	}
	return result;
}

// reference: source/filter_top_expressed_viral_contigs.cpp:22-49
bool related_viral_strains(const std::string& virus1, const std::string& virus2) {
	const std::string* small_virus = &virus1;
	const std::string* big_virus = &virus2;
	if (small_virus->size() > big_virus->size()) std::swap(small_virus, big_virus);
	const char kmer_length = 12;
	std::map<unsigned int, unsigned int> small_virus_kmers;
	for (size_t i = 0; i + kmer_length <= small_virus->size(); i++)
		small_virus_kmers[kmer_to_int(*small_virus, i, kmer_length)] = 0;
	unsigned int shared_kmers = 0;
	const unsigned int min_shared_kmers = small_virus_kmers.size() / 10;
	for (size_t i = 0; i + kmer_length <= big_virus->size(); i++) {
		std::map<unsigned int, unsigned int>::iterator hit = small_virus_kmers.find(kmer_to_int(*big_virus, i, kmer_length));
		if (hit != small_virus_kmers.end() && hit->second++ == 0)
			if (++shared_kmers >= min_shared_kmers)
				return true;
	}
	return false;
}

}

// ---- the ingest result as a file (tooling: repeated benchmark / profiling runs over the same batch skip the parse) ----------------------
namespace {
const char INGEST_MAGIC[8] = { 'A', 'R', 'I', 'B', 'I', 'N', 'G', '2' };
template <class T> void write_vector(FILE* file, const std::vector<T>& values) {
	uint64_t n = values.size();
	if (fwrite(&n, sizeof(n), 1, file) != 1 || (n > 0 && fwrite(values.data(), sizeof(T), n, file) != n)) throw std::runtime_error("failed to write the ingest file");
}
template <class T> void read_vector(FILE* file, std::vector<T>& values) {
	uint64_t n = 0;
	if (fread(&n, sizeof(n), 1, file) != 1) throw std::runtime_error("truncated ingest file");
	values.resize(n);
	if (n > 0 && fread(values.data(), sizeof(T), n, file) != n) throw std::runtime_error("truncated ingest file");
}
void write_string(FILE* file, const std::string& text) { write_vector(file, std::vector<char>(text.begin(), text.end())); }
void read_string(FILE* file, std::string& text) { std::vector<char> bytes; read_vector(file, bytes); text.assign(bytes.begin(), bytes.end()); }
template <class Visit> void visit_ingest(IngestResult& r, Visit& visit) { // the same member order for writing and reading
	Batch& b = r.batch;
	visit(b.n_aln); visit(b.fbits); visit(b.filter); visit(b.group);
	for (int s = 0; s < 3; ++s) { visit(b.contig[s]); visit(b.start[s]); visit(b.end[s]); visit(b.abits[s]); visit(b.cigar_offset[s]); visit(b.cigar_count[s]); }
	visit(b.cigar_pool);
	for (int s = 0; s < 2; ++s) { visit(b.seq_offset[s]); visit(b.seq_length[s]); }
	visit(b.seq_pool); visit(b.name_offset);
	visit(r.mapped_viral_reads_by_contig);
}
}

extern "C" {

const char* ahost_last_error(void) { return g_error.c_str(); }
unsigned int ahost_cpu_budget(void) { return cpu_budget(); }
void ahost_limit_threads_of_this_thread(unsigned int n) { limit_threads_of_this_thread(n); }

// what ahost_write_fusions reads of a SAMPLE (as opposed to the reference data): coverage_t, the rows of the supporting reads and how they are numbered
struct SampleView { const Contigs* contigs; const Coverage* coverage; const Batch* batch; const std::vector<uint32_t>* row_fragments; bool rows_in_list_order, device_batch, have_batch; };
struct ahost_detached_sample { ahost_session* session; Contigs contigs; Coverage coverage; Batch batch; std::vector<uint32_t> row_fragments; bool rows_in_list_order, device_batch, have_batch; };
static SampleView sample_of(const ahost_session* session) {
	SampleView v = { &session->contigs, &session->ingest.coverage, &session->ingest.batch, &session->row_fragments, session->rows_in_list_order, session->device_batch, session->have_batch };
	return v;
}

int ahost_load_genomic_breakpoints(ahost_session* session, const char* path, const agpu_genomic_breakpoint** variants, uint32_t* n_variants) {
	if (!session || !path || !variants || !n_variants) { g_error = "null argument"; return -1; }
	try {
		load_genomic_breakpoints(path, session->contigs, session->genomic_breakpoints);
		*variants = session->genomic_breakpoints.empty() ? nullptr : session->genomic_breakpoints.data();
		*n_variants = (uint32_t) session->genomic_breakpoints.size();
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_load_tags(ahost_session* session, const char* path) {
	if (!session || !path) { g_error = "null argument"; return -1; }
	try { load_tags(path, session->contigs, session->annotation, session->tags); return 0; }
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_load_protein_domains(ahost_session* session, const char* path) {
	if (!session || !path) { g_error = "null argument"; return -1; }
	try { load_protein_domains(path, session->contigs, session->annotation, session->protein_domains, session->protein_domain_index); return 0; }
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}

static int write_or_format_fusions(ahost_session* session, const SampleView& sample, const ahost_fusion_table* table, const char* path, int write_discarded, int print_extra_info, unsigned int max_itd_length, int max_mate_gap, int fill_sequence_gaps,
                                   unsigned int part, unsigned int parts, std::string* text_of_part);

int ahost_write_fusions(ahost_session* session, const ahost_fusion_table* table, const char* path, int write_discarded, int print_extra_info, unsigned int max_itd_length, int max_mate_gap, int fill_sequence_gaps) {
	if (!path) { g_error = "null argument"; return -1; }
	if (!session) { g_error = "null argument"; return -1; }
	return write_or_format_fusions(session, sample_of(session), table, path, write_discarded, print_extra_info, max_itd_length, max_mate_gap, fill_sequence_gaps, 0, 1, NULL);
}

// The last output file of a sample written while the session reads the next sample (arriba_workflow_defer_output): the sample's coverage_t and rows leave the session ...
ahost_detached_sample* ahost_detach_sample(ahost_session* session) {
	if (!session) { g_error = "null argument"; return NULL; }
	try {
		std::unique_ptr<ahost_detached_sample> sample(new ahost_detached_sample());
		sample->session = session;
		sample->contigs = session->contigs;
		sample->coverage = std::move(session->ingest.coverage); sample->batch = std::move(session->ingest.batch); sample->row_fragments = std::move(session->row_fragments);
		sample->rows_in_list_order = session->rows_in_list_order; sample->device_batch = session->device_batch; sample->have_batch = session->have_batch;
		session->ingest.coverage = Coverage(); session->ingest.batch = Batch(); session->row_fragments.clear(); session->rows_in_list_order = false; session->have_batch = false; session->sample_was_detached = true; // (the session has no sample until the next ingest; its counters stay)
		{ std::lock_guard<std::mutex> lock(session->detached_mutex); ++session->detached_samples; }
		return sample.release();
	} catch (const std::exception& e) { g_error = e.what(); return NULL; }
}
// ... are written from where they are, by any thread ...
int ahost_write_fusions_of(ahost_detached_sample* sample, const ahost_fusion_table* table, const char* path, int write_discarded, int print_extra_info, unsigned int max_itd_length, int max_mate_gap, int fill_sequence_gaps) {
	if (!sample || !path) { g_error = "null argument"; return -1; }
	const SampleView view = { &sample->contigs, &sample->coverage, &sample->batch, &sample->row_fragments, sample->rows_in_list_order, sample->device_batch, sample->have_batch };
	return write_or_format_fusions(sample->session, view, table, path, write_discarded, print_extra_info, max_itd_length, max_mate_gap, fill_sequence_gaps, 0, 1, NULL);
}
// ... and given back: the vectors of the rows go to the session for the rows of a later sample (a gigabyte of fresh vectors per sample costs 0.3 s: ahost_set_batch_rows)
void ahost_release_sample(ahost_detached_sample* sample) {
	if (!sample) return;
	ahost_session* session = sample->session;
	{
		std::lock_guard<std::mutex> lock(session->detached_mutex);
		if (sample->device_batch && sample->batch.seq_pool.capacity() > session->spare_rows.seq_pool.capacity()) session->spare_rows = std::move(sample->batch);
		--session->detached_samples;
	}
	session->detached_changed.notify_all();
	delete sample;
}

int ahost_format_fusions(ahost_session* session, const ahost_fusion_table* table, int write_discarded, int print_extra_info, unsigned int max_itd_length, int max_mate_gap, int fill_sequence_gaps,
                         unsigned int part, unsigned int parts, const char** text, uint64_t* bytes) {
	if (!session || !text || !bytes || parts == 0 || part >= parts) { g_error = "null argument"; return -1; }
	session->formatted_rows.clear();
	const int status = write_or_format_fusions(session, sample_of(session), table, "", write_discarded, print_extra_info, max_itd_length, max_mate_gap, fill_sequence_gaps, part, parts, &session->formatted_rows);
	*text = session->formatted_rows.data(); *bytes = session->formatted_rows.size();
	return status;
}

static int write_or_format_fusions(ahost_session* session, const SampleView& sample, const ahost_fusion_table* table, const char* path, int write_discarded, int print_extra_info, unsigned int max_itd_length, int max_mate_gap, int fill_sequence_gaps,
                                   unsigned int part, unsigned int parts, std::string* text_of_part) {
	if (!session || !table || !path) { g_error = "null argument"; return -1; }
	if (!sample.have_batch) { g_error = "no BAM ingested yet"; return -1; }
	try {
		const std::chrono::steady_clock::time_point profile_start = std::chrono::steady_clock::now();
		FusionTable t;
		t.n_candidates = table->n_candidates; t.gene1 = table->gene1; t.gene2 = table->gene2; t.contigs = table->contigs; t.breakpoint1 = table->breakpoint1; t.breakpoint2 = table->breakpoint2;
		t.flags = table->flags; t.filter = table->filter; t.split_reads1 = table->split_reads1; t.split_reads2 = table->split_reads2; t.discordant_mates = table->discordant_mates;
		t.list_offset = table->list_offset; t.read_lists = table->read_lists; t.evalue = table->evalue; t.confidence = table->confidence; t.iteration_rank = table->iteration_rank;
		t.read_filter = table->read_filter; t.closest_genomic_breakpoint1 = table->closest_genomic_breakpoint1; t.closest_genomic_breakpoint2 = table->closest_genomic_breakpoint2; t.n_genes = table->n_genes; t.gene_contig = table->gene_contig; t.gene_start = table->gene_start; t.gene_end = table->gene_end;
		OutputExtras extras = { &session->tags, &session->protein_domains, &session->protein_domain_index, max_mate_gap, fill_sequence_gaps != 0 };
		extras.part = part; extras.parts = parts; extras.text_of_part = text_of_part;
		if (!write_discarded && text_of_part == NULL) extras.rows_written = &session->written_rows;
		// device ingest: the batch of the session holds only the rows fetched for this table (ahost_set_batch_rows); the read lists of the candidates
		// that get written and the filter column are translated from fragments to rows
		std::vector<uint32_t> lists_as_rows; std::vector<uint8_t> filter_of_rows;
		if (print_extra_info && sample.device_batch && t.n_candidates > 0 && sample.rows_in_list_order) {
			// the rows came in the order of the read lists: entry k of the lists is row k, and the reads of a candidate lie next to each other in every column of the batch
			// (the pile-ups of the writer walk them one after the other: with rows in fragment order every read is a cache miss in a dozen columns)
			const size_t n_entries = t.list_offset[3 * (size_t) t.n_candidates];
			if (n_entries >= 0xFFFFFFFFull) throw std::runtime_error("the candidates to be written list more than 2^32 supporting reads: rows are numbered with 32 bits");
			if (sample.batch->n != n_entries || table->read_filter_of_rows == NULL) throw std::runtime_error("rows in list order: one row and one filter per entry of the read lists expected (ahost_set_batch_rows, read_filter_of_rows)");
			lists_as_rows.resize(n_entries);
			for (size_t k = 0; k < n_entries; ++k) lists_as_rows[k] = (uint32_t) k;
			t.read_lists = lists_as_rows.data(); t.read_filter = table->read_filter_of_rows;
		} else if (print_extra_info && sample.device_batch && t.n_candidates > 0) {
			const std::vector<uint32_t>& fragments = *sample.row_fragments; // ascending
			const size_t n_entries = t.list_offset[3 * (size_t) t.n_candidates];
			lists_as_rows.resize(n_entries);
			filter_of_rows.resize(fragments.size() + 1);
			if (table->read_filter_of_rows != NULL) memcpy(filter_of_rows.data(), table->read_filter_of_rows, fragments.size()); // (the device picked them: agpu_get_filters_of)
			else { if (t.read_filter == NULL) throw std::runtime_error("the table holds neither read_filter nor read_filter_of_rows"); for (size_t row = 0; row < fragments.size(); ++row) filter_of_rows[row] = t.read_filter[fragments[row]]; }
			// fragment -> row: a bit per fragment and the number of set bits in front of every word (the row of a fragment is its rank among the fragments handed over);
			// the lists are translated by all threads (10^6 entries of the written candidates of a 10^7-fragment sample; a binary search per entry on one thread took 0.25 s)
			const size_t words = fragments.empty() ? 1 : (size_t) fragments.back() / 64 + 1;
			std::vector<uint64_t> bits(words, 0); std::vector<uint32_t> rank(words + 1, 0);
			for (size_t row = 0; row < fragments.size(); ++row) bits[fragments[row] / 64] |= (uint64_t) 1 << (fragments[row] % 64);
			for (size_t w = 0; w < words; ++w) rank[w + 1] = rank[w] + (uint32_t) __builtin_popcountll(bits[w]);
			std::atomic<bool> missing(false);
			const FusionTable* table_view = &t;
			unsigned int n_threads = std::max(1u, std::min(cpu_budget(), 64u));
			if (n_entries < (1u << 16)) n_threads = 1;
			std::vector<std::thread> threads;
			auto translate = [&](uint32_t first_candidate, uint32_t last_candidate) {
				for (uint32_t c = first_candidate; c < last_candidate; ++c) {
					const bool written = (write_discarded != 0) != (table_view->filter[c] == 0);
					for (uint64_t k = table_view->list_offset[3 * (size_t) c]; k < table_view->list_offset[3 * (size_t) c + 3]; ++k) {
						if (!written) { lists_as_rows[k] = 0; continue; }
						const uint32_t fragment = table_view->read_lists[k];
						if ((size_t) fragment / 64 >= words || !(bits[fragment / 64] >> (fragment % 64) & 1)) { missing = true; lists_as_rows[k] = 0; continue; }
						lists_as_rows[k] = rank[fragment / 64] + (uint32_t) __builtin_popcountll(bits[fragment / 64] & (((uint64_t) 1 << (fragment % 64)) - 1));
					}
				}
			};
			for (unsigned int thread = 0; thread < n_threads; ++thread) {
				const uint32_t first_candidate = (uint32_t) ((uint64_t) t.n_candidates * thread / n_threads), last_candidate = (uint32_t) ((uint64_t) t.n_candidates * (thread + 1) / n_threads);
				if (n_threads == 1) translate(first_candidate, last_candidate); else threads.push_back(std::thread(translate, first_candidate, last_candidate));
			}
			for (size_t thread = 0; thread < threads.size(); ++thread) threads[thread].join();
			if (missing) throw std::runtime_error("a supporting read of a written candidate is not among the rows handed over (ahost_fusion_table_reads / ahost_set_batch_rows)");
			t.read_lists = lists_as_rows.data(); t.read_filter = filter_of_rows.data();
		}
		if (getenv("ARRIBA_WRITER_PROFILE")) fprintf(stderr, "[writer] lists translated to rows: %.3f s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - profile_start).count());
		const bool no_rows = sample.device_batch && !print_extra_info;
		write_fusions_to_file(session->annotation, session->exon_index, *sample.contigs, session->assembly, *sample.coverage, no_rows ? NULL : sample.batch, t, path, write_discarded != 0, print_extra_info != 0, max_itd_length, extras);
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}

int ahost_fusion_table_reads(const ahost_fusion_table* table, int write_discarded, uint32_t* fragments, uint64_t capacity, uint64_t* count) {
	if (!table || !count) { g_error = "null argument"; return -1; }
	try {
		// ascending and without repeats: a bit per fragment instead of a sort of 10^6 list entries
		uint32_t highest = 0; bool any = false;
		for (uint32_t c = 0; c < table->n_candidates; ++c)
			if ((write_discarded != 0) != (table->filter[c] == 0))
				for (uint64_t k = table->list_offset[3 * (size_t) c]; k < table->list_offset[3 * (size_t) c + 3]; ++k) { highest = std::max(highest, table->read_lists[k]); any = true; }
		std::vector<uint64_t> bits(any ? (size_t) highest / 64 + 1 : 0, 0);
		for (uint32_t c = 0; c < table->n_candidates; ++c)
			if ((write_discarded != 0) != (table->filter[c] == 0))
				for (uint64_t k = table->list_offset[3 * (size_t) c]; k < table->list_offset[3 * (size_t) c + 3]; ++k) bits[table->read_lists[k] / 64] |= (uint64_t) 1 << (table->read_lists[k] % 64);
		uint64_t total = 0;
		for (size_t w = 0; w < bits.size(); ++w) total += (uint64_t) __builtin_popcountll(bits[w]);
		*count = total;
		if (fragments) {
			if (capacity < total) { g_error = "capacity too small"; return -1; }
			uint64_t at = 0;
			for (size_t w = 0; w < bits.size(); ++w)
				for (uint64_t word = bits[w]; word != 0; word &= word - 1) fragments[at++] = (uint32_t) (w * 64 + (size_t) __builtin_ctzll(word));
		}
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}

float ahost_read_length_sum_of(float running_sum, const uint32_t* mate1_lengths, const uint32_t* mate2_lengths, uint64_t count) {
	for (uint64_t i = 0; i < count; ++i) // sequential float accumulation in name order, hazard H4
		running_sum += ((size_t) mate1_lengths[i] + (size_t) mate2_lengths[i]) / 2;
	return running_sum;
}

int ahost_load_range_rules(ahost_session* session, const char* path, int allow_keywords, const agpu_range_rule** rules, uint32_t* n_rules) {
	if (!session || !path || !rules || !n_rules) { g_error = "null argument"; return -1; }
	try {
		std::vector<agpu_range_rule>& slot = session->range_rules[allow_keywords ? 1 : 0];
		load_range_rules(path, session->contigs, session->annotation, allow_keywords != 0, slot);
		*rules = slot.empty() ? nullptr : slot.data();
		*n_rules = (uint32_t) slot.size();
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}

ahost_session* ahost_open(const char* fasta_path, const char* gtf_path, const char* interesting_contigs, const char* viral_contigs, const char* gtf_features) {
	std::unique_ptr<ahost_session> session(new ahost_session());
	try {
		if (interesting_contigs) session->options.interesting_contigs = interesting_contigs;
		if (viral_contigs) session->options.viral_contigs = viral_contigs;
		load_assembly(session->assembly, fasta_path, session->contigs, session->options.interesting_contigs);
		read_annotation_gtf(session->annotation, gtf_path, gtf_features ? gtf_features : DEFAULT_GTF_FEATURES, session->contigs, session->assembly);
		// the reference sizes its index by the number of features (source/annotation.t.hpp:26), i.e. every contig id is in range
		make_flat_index(session->annotation.exons, std::max(session->annotation.exons.size(), session->contigs.size()), session->exon_index);
		make_flat_index(session->annotation.genes, std::max(session->annotation.genes.size(), session->contigs.size()), session->gene_index);
		compute_exonic_length(session->annotation, session->exon_index);
		session->build_reference_views();
		session->build_genome_view();
		session->contigs_at_open = session->contigs.size();
		return session.release();
	} catch (const std::exception& e) {
		g_error = e.what();
		return NULL;
	}
}

void ahost_close(ahost_session* session) {
	if (!session) return;
	{ std::unique_lock<std::mutex> lock(session->detached_mutex); session->detached_changed.wait(lock, [session] { return session->detached_samples == 0; }); } // (a writer still holds a sample of this session)
	delete session;
}

int ahost_ingest_bam_file(ahost_session* session, const char* bam_path, int external_duplicate_marking, unsigned int max_itd_length) {
	try { return ingest(session, open_bam_file(bam_path), external_duplicate_marking, max_itd_length); }
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_ingest_separate(ahost_session* session, const char* chimeric_path, const char* rna_path, int external_duplicate_marking, unsigned int max_itd_length, uint64_t* chimeric_fragments, uint64_t* chimeric_malformed) {
	if (!session || !chimeric_path || !rna_path) { g_error = "null argument"; return -1; }
	try {
		std::unique_ptr<ByteSource> chimeric(open_bam_file(chimeric_path)), rna(open_bam_file(rna_path));
		session->options.external_duplicate_marking = external_duplicate_marking != 0;
		session->options.max_itd_length = max_itd_length;
		session->ingest = IngestResult(); session->sample_was_detached = false;
		session->row_fragments.clear(); session->device_batch = false; session->rows_in_list_order = false;
		read_chimeric_alignments_separate(*chimeric, *rna, session->assembly, session->contigs, session->annotation, session->gene_index, session->options, session->ingest);
		if (chimeric_fragments) *chimeric_fragments = session->ingest.separate_fragments;
		if (chimeric_malformed) *chimeric_malformed = session->ingest.separate_malformed_count;
		session->build_genome_view();
		session->build_batch_view();
		session->have_batch = true;
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_save_ingest(ahost_session* session, const char* path) {
	if (!session || !session->have_batch) { g_error = "no BAM ingested yet"; return -1; }
	FILE* file = fopen(path, "wb");
	if (!file) { g_error = std::string("cannot write ") + path; return -1; }
	try {
		IngestResult& r = session->ingest;
		uint64_t scalars[6] = { r.batch.n, r.mapped_reads, r.malformed_count, r.missing_hi_tag, r.records, session->contigs.size() };
		if (fwrite(INGEST_MAGIC, 8, 1, file) != 1 || fwrite(scalars, sizeof(scalars), 1, file) != 1) throw std::runtime_error("failed to write the ingest file");
		std::vector<std::string> name_by_id(session->contigs.size());
		for (std::map<std::string, contig_t>::const_iterator c = session->contigs.by_name.begin(); c != session->contigs.by_name.end(); ++c) name_by_id[c->second] = c->first;
		for (size_t c = 0; c < name_by_id.size(); ++c) write_string(file, name_by_id[c]);
		auto write = [file](auto& values) { write_vector(file, values); };
		visit_ingest(r, write);
		write_string(file, r.batch.names);
		uint64_t n_coverage = r.coverage.coverage.size();
		if (fwrite(&n_coverage, 8, 1, file) != 1) throw std::runtime_error("failed to write the ingest file");
		for (size_t c = 0; c < n_coverage; ++c) { write_vector(file, r.coverage.coverage[c]); write_vector(file, r.coverage.fragment_starts[c]); write_vector(file, r.coverage.fragment_ends[c]); }
		if (fclose(file) != 0) { file = NULL; throw std::runtime_error("failed to write the ingest file"); }
		return 0;
	} catch (const std::exception& e) {
		if (file) fclose(file);
		g_error = e.what();
		return -1;
	}
}

int ahost_load_ingest(ahost_session* session, const char* path) {
	if (!session) { g_error = "null session"; return -1; }
	FILE* file = fopen(path, "rb");
	if (!file) { g_error = std::string("cannot read ") + path; return -1; }
	try {
		char magic[8]; uint64_t scalars[6];
		if (fread(magic, 8, 1, file) != 1 || memcmp(magic, INGEST_MAGIC, 8) != 0 || fread(scalars, sizeof(scalars), 1, file) != 1) throw std::runtime_error("not an ingest file of this version");
		session->ingest = IngestResult(); session->sample_was_detached = false;
		IngestResult& r = session->ingest;
		r.batch.n = scalars[0]; r.mapped_reads = scalars[1]; r.malformed_count = (unsigned int) scalars[2]; r.missing_hi_tag = (unsigned int) scalars[3]; r.records = scalars[4];
		for (uint64_t c = 0; c < scalars[5]; ++c) { // the contigs the BAM header added behind those of the assembly, in the same order
			std::string name; read_string(file, name);
			const contig_t id = session->contigs.add(name);
			if (id != c) throw std::runtime_error("the ingest file was written with another assembly (contig '" + name + "')");
		}
		auto read = [file](auto& values) { read_vector(file, values); };
		visit_ingest(r, read);
		read_string(file, r.batch.names);
		uint64_t n_coverage = 0;
		if (fread(&n_coverage, 8, 1, file) != 1) throw std::runtime_error("truncated ingest file");
		r.coverage.coverage.resize(n_coverage); r.coverage.fragment_starts.resize(n_coverage); r.coverage.fragment_ends.resize(n_coverage);
		for (size_t c = 0; c < n_coverage; ++c) { read_vector(file, r.coverage.coverage[c]); read_vector(file, r.coverage.fragment_starts[c]); read_vector(file, r.coverage.fragment_ends[c]); }
		fclose(file);
		if (r.batch.n_aln.size() != r.batch.n || r.batch.name_offset.size() != r.batch.n + 1) throw std::runtime_error("inconsistent ingest file");
		session->build_genome_view();
		session->build_batch_view();
		session->have_batch = true;
		return 0;
	} catch (const std::exception& e) {
		g_error = e.what();
		return -1;
	}
}

int ahost_bam_open(ahost_session* session, const char* bam_path, int external_duplicate_marking, unsigned int max_itd_length, agpu_ingest_config* config) {
	if (!session || !bam_path || !config) { g_error = "null argument"; return -1; }
	try {
		if (session->feed) { close_bam_feed(session->feed); session->feed = nullptr; }
		session->options.external_duplicate_marking = external_duplicate_marking != 0;
		session->options.max_itd_length = max_itd_length;
		{ std::lock_guard<std::mutex> lock(session->detached_mutex); if (session->device_batch && session->ingest.batch.seq_pool.capacity() > session->spare_rows.seq_pool.capacity()) session->spare_rows = std::move(session->ingest.batch); } // (the rows of the last sample's writer: their memory is taken again by ahost_set_batch_rows)
		session->ingest = IngestResult();
		session->have_batch = false; session->sample_was_detached = false;
		session->feed = open_bam_feed(bam_path);
		std::vector<std::string> target_names;
		const uint64_t header_size = bam_feed_header(session->feed, target_names);
		session->input_header = bam_feed_header_bytes(session->feed);
		session->last_target_names = target_names;
		// reference: source/read_chimeric_alignments.cpp:566-582 (contigs of the header join contigs_t; interesting contigs need a sequence)
		session->tid_to_contig.resize(target_names.size());
		for (size_t target = 0; target < target_names.size(); ++target) session->tid_to_contig[target] = session->contigs.add(target_names[target]);
		session->ingest.coverage.resize(session->contigs, session->assembly);
		for (std::map<std::string, contig_t>::const_iterator contig = session->contigs.by_name.begin(); contig != session->contigs.by_name.end(); ++contig)
			if (!session->assembly.has(contig->second) && is_interesting_contig(contig->first, session->options.interesting_contigs))
				throw std::runtime_error("could not find sequence of contig '" + contig->first + "'");
		if (session->genome_view.n_contigs != session->contigs.size() || session->genome_view.bases == NULL) session->build_genome_view(); // only when the header brought new contigs
		const Coverage& coverage = session->ingest.coverage;
		session->window_offset.assign(session->contigs.size() + 1, 0);
		for (size_t contig = 0; contig < session->contigs.size(); ++contig)
			session->window_offset[contig + 1] = session->window_offset[contig] + (contig < coverage.coverage.size() ? coverage.coverage[contig].size() : 0);
		memset(config, 0, sizeof(*config));
		config->n_targets = (uint32_t) session->tid_to_contig.size(); config->tid_to_contig = session->tid_to_contig.data();
		config->first_record_offset = header_size; config->stream_size_hint = bam_feed_size_hint(session->feed);
		config->n_contigs = (uint32_t) session->contigs.size(); config->coverage_window_offset = session->window_offset.data();
		config->external_duplicate_marking = external_duplicate_marking != 0; config->max_itd_length = max_itd_length;
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}

int ahost_bam_open_role(ahost_session* session, const char* bam_path, int external_duplicate_marking, unsigned int max_itd_length, int role, agpu_ingest_config* config) {
	if (role < AGPU_ROLE_WHOLE || role > AGPU_ROLE_SEPARATE_RNA) { g_error = "ahost_bam_open_role: role must be AGPU_ROLE_WHOLE, AGPU_ROLE_SEPARATE_CHIMERIC or AGPU_ROLE_SEPARATE_RNA"; return -1; }
	if (ahost_bam_open(session, bam_path, external_duplicate_marking, max_itd_length, config) != 0) return -1;
	try {
		const std::vector<std::string>& target_names = session->last_target_names;
		if (role == AGPU_ROLE_SEPARATE_RNA && target_names != session->separate_target_names) {
			close_bam_feed(session->feed); session->feed = nullptr;
			throw std::runtime_error("the headers of the separate chimeric file (-c) and of the main alignments (-x) do not list the same reference sequences in the same order");
		}
		if (role == AGPU_ROLE_SEPARATE_CHIMERIC) session->separate_target_names = target_names; else session->separate_target_names.clear();
		config->role = (uint8_t) role;
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}

int ahost_bam_open_part(ahost_session* session, const char* bam_path, int external_duplicate_marking, unsigned int max_itd_length, unsigned int part, unsigned int parts, agpu_ingest_config* config) {
	if (ahost_bam_open(session, bam_path, external_duplicate_marking, max_itd_length, config) != 0) return -1;
	try {
		config->first_record_offset = bam_feed_take_part(session->feed, part, parts);
		config->part_of_sample = 1;
		if (config->stream_size_hint > 0 && parts > 0) config->stream_size_hint = config->stream_size_hint / parts + (64u << 20);
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}

int ahost_bam_next(ahost_session* session, void* buffer, size_t capacity, agpu_bgzf_block* blocks, uint32_t block_capacity, ahost_bam_piece* piece) {
	if (!session || !session->feed || !buffer || !piece) { g_error = "ahost_bam_open must run first"; return -1; }
	try { return bam_feed_next(session->feed, (uint8_t*) buffer, capacity, blocks, block_capacity, *piece) ? 1 : 0; }
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}

int ahost_bam_sam_targets(ahost_session* session, const char** names, const uint32_t** name_offset, uint32_t* n_targets) {
	if (!session || !session->feed || !names || !name_offset || !n_targets) { g_error = "ahost_bam_open must run first"; return -1; }
	const SamTargetTable* table = bam_feed_sam_targets(session->feed);
	if (table == NULL) return 0;
	*names = table->names.data(); *name_offset = table->offsets.data(); *n_targets = (uint32_t) table->offsets.size() - 1;
	return 1;
}

int ahost_sam_transcode(const void* text, size_t size, const char* names, const uint32_t* name_offset, uint32_t n_targets, void* out, size_t capacity, uint64_t* out_bytes, uint64_t* n_records, uint64_t* bad_line) {
	if ((!text && size > 0) || !name_offset || !out_bytes || !n_records || !bad_line) { g_error = "null argument"; return -1; }
	try {
		*out_bytes = 0; *n_records = 0; *bad_line = 0;
		SamTargetTable targets;
		targets.build(names ? names : "", name_offset, n_targets);
		const uint8_t* bytes = (const uint8_t*) text;
		size_t at = 0; uint64_t header_lines = 0;
		while (at < size && bytes[at] == '@') { const uint8_t* feed = (const uint8_t*) memchr(bytes + at, '\n', size - at); at = feed ? (size_t) (feed - bytes) + 1 : size; ++header_lines; }
		std::vector<uint8_t> records;
		uint64_t lines = 0; uint32_t reason = 0;
		sam_transcode_lines(bytes + at, size - at, targets.view(), header_lines + 1, records, *n_records, lines, *bad_line, reason);
		*out_bytes = records.size();
		if (records.size() > capacity) { g_error = "the buffer is too small for the records"; return -1; }
		if (!records.empty()) memcpy(out, records.data(), records.size());
		if (*bad_line != 0) { g_error = sam_line_error(*bad_line, reason); return -1; }
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}

// ---- --sorted-bam (include/arriba_host.h) ----
namespace {
inline uint32_t le32(const uint8_t* p) { return (uint32_t) p[0] | (uint32_t) p[1] << 8 | (uint32_t) p[2] << 16 | (uint32_t) p[3] << 24; }
thread_local std::vector<uint8_t> g_sorted_header; thread_local std::vector<uint32_t> g_sorted_ref_length; thread_local SortedBam g_sorted_bam;
void frame_header(const uint8_t* input, size_t size, std::vector<uint8_t>& framed, std::vector<uint32_t>& ref_length) {
	std::vector<uint8_t> header;
	sorted_bam_header(input, size, header, ref_length);
	framed.clear();
	sorted_bam_frame(header.data(), header.size(), framed);
}
}
int ahost_sorted_bam_header(ahost_session* session, const uint8_t** framed, uint64_t* framed_bytes, const uint32_t** ref_length, uint32_t* n_ref) {
	if (!session || !framed || !framed_bytes || !ref_length || !n_ref) { g_error = "null argument"; return -1; }
	if (session->input_header.empty()) { g_error = "ahost_bam_open must run first"; return -1; }
	try {
		frame_header(session->input_header.data(), session->input_header.size(), session->sorted_bam_header_framed, session->sorted_bam_ref_length);
		*framed = session->sorted_bam_header_framed.data(); *framed_bytes = session->sorted_bam_header_framed.size(); *ref_length = session->sorted_bam_ref_length.data(); *n_ref = (uint32_t) session->sorted_bam_ref_length.size();
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_sorted_bam_header_of(const void* input_header, size_t size, const uint8_t** framed, uint64_t* framed_bytes, const uint32_t** ref_length, uint32_t* n_ref) {
	if (!input_header || !framed || !framed_bytes || !ref_length || !n_ref) { g_error = "null argument"; return -1; }
	try {
		frame_header((const uint8_t*) input_header, size, g_sorted_header, g_sorted_ref_length);
		*framed = g_sorted_header.data(); *framed_bytes = g_sorted_header.size(); *ref_length = g_sorted_ref_length.data(); *n_ref = (uint32_t) g_sorted_ref_length.size();
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_sorted_bam(const void* records, size_t size, uint64_t first_block_file_offset, const uint32_t* ref_length, uint32_t n_ref, const uint8_t** blocks, agpu_sorted_bam_info* info, agpu_sorted_bam_index_arrays* index) {
	return ahost_sorted_bam_level(records, size, first_block_file_offset, ref_length, n_ref, 0, blocks, info, index);
}
int ahost_sorted_bam_level(const void* records, size_t size, uint64_t first_block_file_offset, const uint32_t* ref_length, uint32_t n_ref, int level, const uint8_t** blocks, agpu_sorted_bam_info* info, agpu_sorted_bam_index_arrays* index) {
	if ((!records && size > 0) || !blocks || !info) { g_error = "null argument"; return -1; }
	try {
		sorted_bam_of((const uint8_t*) records, size, first_block_file_offset, index != NULL ? ref_length : NULL, n_ref, g_sorted_bam, level);
		*blocks = g_sorted_bam.blocks.data(); *info = g_sorted_bam.info;
		if (index != NULL) *index = g_sorted_bam.view(n_ref);
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_sorted_bam_write_index(const agpu_sorted_bam_index_arrays* index, const char* path) {
	if (!index || !path) { g_error = "null argument"; return -1; }
	try {
		std::vector<uint8_t> bai;
		sorted_bam_bai(*index, bai);
		FILE* file = fopen(path, "wb");
		if (file == NULL) throw std::runtime_error(std::string("failed to open '") + path + "' for writing");
		const bool written = fwrite(bai.data(), 1, bai.size(), file) == bai.size();
		if (fclose(file) != 0 || !written) { remove(path); throw std::runtime_error(std::string("failed to write '") + path + "'"); }
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}
void ahost_sorted_bam_eof(uint8_t* block) { for (uint32_t i = 0; i < agpu::SBAM_EOF_BYTES; ++i) block[i] = agpu::sbam_eof_byte(i); }
int ahost_sorted_bam_write(const void* input_header, size_t header_size, const void* records, size_t size, const char* path, agpu_sorted_bam_info* info) {
	return ahost_sorted_bam_write_level(input_header, header_size, records, size, path, 0, info);
}
int ahost_sorted_bam_write_level(const void* input_header, size_t header_size, const void* records, size_t size, const char* path, int level, agpu_sorted_bam_info* info) {
	if (!input_header || (!records && size > 0) || !path) { g_error = "null argument"; return -1; }
	try { sorted_bam_write((const uint8_t*) input_header, header_size, (const uint8_t*) records, size, path, info, level); return 0; }
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}
namespace {
// a file (BAM in BGZF, gzip or raw; SAM text) read whole into host memory as the uncompressed BAM stream; returns where its records begin
uint64_t read_whole_bam(const char* input_path, std::vector<uint8_t>& stream) {
	std::unique_ptr<ByteSource> source(text_or_bam_source(open_bam_file(input_path))); // (BGZF, gzip or raw; SAM text comes out as the BAM stream of its alignments)
	stream.clear();
	for (size_t got = 1; got > 0; ) { const size_t at = stream.size(); stream.resize(at + (16u << 20)); got = source->read(&stream[at], stream.size() - at); stream.resize(at + got); }
	if (stream.size() < 12 || memcmp(stream.data(), "BAM\1", 4) != 0) throw std::runtime_error("failed to read SAM header");
	uint64_t at = 8 + (uint64_t) le32(&stream[4]);
	if (stream.size() < at + 4) throw std::runtime_error("failed to read SAM header");
	const uint32_t n_ref = le32(&stream[at]);
	at += 4;
	for (uint32_t t = 0; t < n_ref; ++t) { if (stream.size() < at + 4) throw std::runtime_error("failed to read SAM header"); at += 8 + (uint64_t) le32(&stream[at]); if (stream.size() < at) throw std::runtime_error("failed to read SAM header"); }
	return at;
}
}
int ahost_sorted_bam_file(const char* input_path, const char* path, agpu_sorted_bam_info* info) { return ahost_sorted_bam_file_level(input_path, path, 0, info); }
int ahost_sorted_bam_file_level(const char* input_path, const char* path, int level, agpu_sorted_bam_info* info) {
	if (!input_path || !path) { g_error = "null argument"; return -1; }
	if (level != 0 && level != 1) { g_error = "the compression level of a sorted BAM file is 0 (stored) or 1"; return -1; }
	try {
		std::vector<uint8_t> stream;
		const uint64_t at = read_whole_bam(input_path, stream);
		sorted_bam_write(stream.data(), at, stream.data() + at, stream.size() - at, path, info, level);
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}
// --mark-duplicates (include/arriba_host.h)
int ahost_sorted_bam_file_marked(const char* input_path, const char* path, int level, int mark_duplicates, agpu_sorted_bam_info* info) { return ahost_sorted_bam_file_marked_counts(input_path, path, level, mark_duplicates, info, NULL); }
int ahost_sorted_bam_file_marked_counts(const char* input_path, const char* path, int level, int mark_duplicates, agpu_sorted_bam_info* info, agpu_markdup_counts* counts) {
	if (!input_path || !path) { g_error = "null argument"; return -1; }
	if (level != 0 && level != 1) { g_error = "the compression level of a sorted BAM file is 0 (stored) or 1"; return -1; }
	try {
		std::vector<uint8_t> stream;
		const uint64_t at = read_whole_bam(input_path, stream);
		sorted_bam_write(stream.data(), at, stream.data() + at, stream.size() - at, path, info, level, mark_duplicates != 0, counts);
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_markdup(const void* records, size_t size, uint8_t* flag, uint64_t n_records, agpu_markdup_counts* counts) {
	if ((!records && size > 0) || (!flag && n_records > 0)) { g_error = "null argument"; return -1; }
	try {
		std::vector<uint8_t> bytes; agpu_markdup_counts counted;
		markdup_flags((const uint8_t*) records, size, bytes, counted);
		if (bytes.size() != n_records) throw std::runtime_error("ahost_markdup: the stream holds " + std::to_string(bytes.size()) + " records, not " + std::to_string(n_records));
		if (n_records > 0) memcpy(flag, bytes.data(), n_records);
		if (counts) *counts = counted;
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}

// ---- --supporting-alignments (include/arriba_host.h) ----
struct ahost_supporting_writer { SupportingWriter writer; ahost_supporting_writer(const char* prefix, const uint8_t* header, uint64_t bytes, uint32_t n_rows, const uint64_t* row_file_bytes) : writer(prefix, header, bytes, n_rows, row_file_bytes) {} };
ahost_supporting_writer* ahost_supporting_writer_open(const char* prefix, const void* framed_header, uint64_t framed_bytes, uint32_t n_rows, const uint64_t* row_file_bytes) {
	if (!prefix || (!framed_header && framed_bytes > 0) || (!row_file_bytes && n_rows > 0)) { g_error = "null argument"; return NULL; }
	try { return new ahost_supporting_writer(prefix, (const uint8_t*) framed_header, framed_bytes, n_rows, row_file_bytes); }
	catch (const std::exception& e) { g_error = e.what(); return NULL; }
}
int ahost_supporting_writer_push(ahost_supporting_writer* writer, const void* bytes, uint64_t size) {
	if (!writer || (!bytes && size > 0)) { g_error = "null argument"; return -1; }
	try { writer->writer.push((const uint8_t*) bytes, size); return 0; }
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_supporting_writer_index(ahost_supporting_writer* writer, const agpu_supporting_index_arrays* index, const uint32_t* ref_length, uint32_t n_ref) {
	if (!writer || !index || (!ref_length && n_ref > 0)) { g_error = "null argument"; return -1; }
	try { writer->writer.index(*index, ref_length, n_ref); return 0; }
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_supporting_writer_close(ahost_supporting_writer* writer, int commit) {
	if (!writer) return 0;
	int status = 0;
	try { if (commit) writer->writer.commit(); else writer->writer.abandon(); }
	catch (const std::exception& e) { g_error = e.what(); status = -1; writer->writer.abandon(); }
	delete writer;
	return status;
}
int ahost_supporting_alignments(const void* input_header, size_t header_size, const void* records, size_t size, const char* names, const uint64_t* name_offset, uint64_t n_names,
                                const agpu_supporting_rows* rows, int64_t window, const char* prefix, agpu_supporting_info* info) {
	if (!input_header || (!records && size > 0) || (n_names > 0 && (!names || !name_offset)) || !rows || !prefix) { g_error = "null argument"; return -1; }
	try { supporting_alignments((const uint8_t*) input_header, header_size, (const uint8_t*) records, size, names, name_offset, n_names, false, *rows, window, prefix, info); return 0; }
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}
namespace {
// the contig of a breakpoint is the reference sequence of the BAM file of that name: the first tid of the header that joined contigs_t under it (-1: none)
void written_rows_of(ahost_session* session, const std::vector<uint32_t>& tid_to_contig) {
	std::vector<int32_t> contig_to_tid(session->contigs.size() + 1, -1);
	for (size_t tid = tid_to_contig.size(); tid-- > 0; ) if (tid_to_contig[tid] < contig_to_tid.size()) contig_to_tid[tid_to_contig[tid]] = (int32_t) tid;
	const size_t n = session->written_rows.size();
	session->written_candidate.resize(n); session->written_ref.resize(2 * n); session->written_breakpoint.resize(2 * n);
	for (size_t r = 0; r < n; ++r) {
		const WrittenRow& row = session->written_rows[r];
		session->written_candidate[r] = row.candidate;
		for (int k = 0; k < 2; ++k) { session->written_ref[2 * r + k] = row.contig[k] < contig_to_tid.size() ? contig_to_tid[row.contig[k]] : -1; session->written_breakpoint[2 * r + k] = row.breakpoint[k]; }
	}
}
}
int ahost_written_fusion_rows(ahost_session* session, uint32_t* n_rows, const uint32_t** candidate, const int32_t** ref, const int32_t** breakpoint) {
	if (!session || !n_rows || !candidate || !ref || !breakpoint) { g_error = "null argument"; return -1; }
	try {
		written_rows_of(session, session->tid_to_contig); // (of the file the last ahost_bam_open opened)
		*n_rows = (uint32_t) session->written_rows.size(); *candidate = session->written_candidate.data(); *ref = session->written_ref.data(); *breakpoint = session->written_breakpoint.data();
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}
// --host-ingest: the rows of the fusions file the session wrote last, the names of their supporting fragments from the batch of the session ("QNAME,HI"), the records of the file
int ahost_supporting_alignments_file(ahost_session* session, const ahost_fusion_table* table, const char* input_path, int64_t window, const char* prefix, agpu_supporting_info* info) {
	if (!session || !table || !input_path || !prefix) { g_error = "null argument"; return -1; }
	try {
		if (!session->have_batch || session->device_batch) throw std::runtime_error("the supporting alignments of a file need the batch of a host ingest");
		std::vector<uint8_t> stream;
		const uint64_t at = read_whole_bam(input_path, stream);
		// (the host ingest read the file by itself: the references of its header are looked up in contigs_t, which they joined then)
		std::vector<uint8_t> framed; std::vector<uint32_t> ref_length; std::vector<uint32_t> tid_to_contig;
		{ uint64_t name_at = 12 + (uint64_t) le32(&stream[4]); const uint32_t n_ref = le32(&stream[name_at - 4]);
		  for (uint32_t t = 0; t < n_ref; ++t) { const uint32_t l_name = le32(&stream[name_at]); tid_to_contig.push_back(session->contigs.add(std::string((const char*) &stream[name_at + 4], l_name > 0 ? l_name - 1 : 0))); name_at += 8 + (uint64_t) l_name; } }
		written_rows_of(session, tid_to_contig);
		const uint32_t n_rows = (uint32_t) session->written_rows.size(); const uint32_t* candidate = session->written_candidate.data(); const int32_t* ref = session->written_ref.data(); const int32_t* breakpoint = session->written_breakpoint.data();
		const Batch& batch = session->ingest.batch;
		std::vector<uint64_t> name_begin(1, 0), name_offset(1, 0); std::vector<uint32_t> entries; std::string names;
		for (uint32_t r = 0; r < n_rows; ++r) {
			if (candidate[r] >= table->n_candidates) throw std::runtime_error("the table is not the one the fusions file was written from");
			for (uint64_t k = table->list_offset[3 * (size_t) candidate[r]]; k < table->list_offset[3 * (size_t) candidate[r] + 3]; ++k) {
				const uint32_t read = table->read_lists[k];
				if (read >= batch.n) throw std::runtime_error("the table is not the one the fusions file was written from");
				entries.push_back((uint32_t) (name_offset.size() - 1));
				names.append(batch.names, batch.name_offset[read], batch.name_offset[read + 1] - batch.name_offset[read]);
				name_offset.push_back(names.size());
			}
			name_begin.push_back(entries.size());
		}
		const agpu_supporting_rows rows = { n_rows, ref, breakpoint, name_begin.data(), entries.data() };
		supporting_alignments(stream.data(), at, stream.data() + at, stream.size() - at, names.data(), name_offset.data(), name_offset.size() - 1, true, rows, window, prefix, info);
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}

// ---- --virus-expression (include/arriba_host.h) ----
namespace {
thread_local VirusContigs g_virus_contigs; thread_local VirusCounters g_virus_counters; thread_local std::string g_virus_text;
}
int ahost_virus_contigs_of_session(ahost_session* session, ahost_virus_contigs* contigs) {
	if (!session || !contigs) { g_error = "null argument"; return -1; }
	if (session->input_header.empty()) { g_error = "ahost_bam_open must run first"; return -1; }
	try { virus_contigs_of(session->input_header.data(), session->input_header.size(), session->options.viral_contigs, g_virus_contigs); *contigs = g_virus_contigs.view(); return 0; }
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_virus_contigs_of(const void* input_header, size_t size, const char* viral_contigs, ahost_virus_contigs* contigs) {
	if (!input_header || !contigs) { g_error = "null argument"; return -1; }
	try { virus_contigs_of((const uint8_t*) input_header, size, viral_contigs ? viral_contigs : IngestOptions().viral_contigs, g_virus_contigs); *contigs = g_virus_contigs.view(); return 0; }
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_virus_expression(const void* records, size_t size, const ahost_virus_contigs* contigs, agpu_virus_counters* counters) {
	if ((!records && size > 0) || !contigs || !counters) { g_error = "null argument"; return -1; }
	try { virus_expression((const uint8_t*) records, size, contigs->viral_ref, contigs->viral_length, contigs->n_viruses, contigs->n_ref, g_virus_counters); *counters = g_virus_counters.view(); return 0; }
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_virus_expression_table(const agpu_virus_counters* counters, const ahost_virus_contigs* contigs, const char** text, uint64_t* bytes) {
	if (!counters || !contigs || !text || !bytes) { g_error = "null argument"; return -1; }
	try { g_virus_text = virus_expression_table(*counters, *contigs); *text = g_virus_text.data(); *bytes = g_virus_text.size(); return 0; }
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_virus_expression_write(const agpu_virus_counters* counters, const ahost_virus_contigs* contigs, const char* path) {
	if (!counters || !contigs || !path) { g_error = "null argument"; return -1; }
	try { virus_expression_write(virus_expression_table(*counters, *contigs), path); return 0; }
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_virus_expression_file(ahost_session* session, const char* input_path, const char* path) {
	if (!session || !input_path || !path) { g_error = "null argument"; return -1; }
	try {
		std::vector<uint8_t> stream;
		const uint64_t at = read_whole_bam(input_path, stream); // (SAM text comes out as the BAM stream of its alignments, behind a BAM header)
		VirusContigs contigs; VirusCounters counters;
		virus_contigs_of(stream.data(), at, session->options.viral_contigs, contigs);
		virus_expression(stream.data() + at, stream.size() - at, contigs.ref.data(), contigs.length.data(), (uint32_t) contigs.ref.size(), contigs.n_ref, counters);
		virus_expression_write(virus_expression_table(counters.view(), contigs.view()), path);
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}

// ---- --coverage (include/arriba_host.h) ----
namespace {
thread_local DepthContigs g_depth_contigs; thread_local std::string g_depth_text;
}
int ahost_depth_contigs_of_session(ahost_session* session, ahost_depth_contigs* contigs) {
	if (!session || !contigs) { g_error = "null argument"; return -1; }
	if (session->input_header.empty()) { g_error = "ahost_bam_open must run first"; return -1; }
	try { depth_contigs_of(session->input_header.data(), session->input_header.size(), g_depth_contigs); *contigs = g_depth_contigs.view(); return 0; }
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_depth_contigs_of(const void* input_header, size_t size, ahost_depth_contigs* contigs) {
	if (!input_header || !contigs) { g_error = "null argument"; return -1; }
	try { depth_contigs_of((const uint8_t*) input_header, size, g_depth_contigs); *contigs = g_depth_contigs.view(); return 0; }
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_depth_track(const void* records, size_t size, const ahost_depth_contigs* contigs, const char** text, uint64_t* bytes, agpu_depth_stats* stats) {
	if ((!records && size > 0) || !contigs || !text || !bytes || !stats) { g_error = "null argument"; return -1; }
	try { depth_track((const uint8_t*) records, size, *contigs, g_depth_text, *stats); *text = g_depth_text.data(); *bytes = g_depth_text.size(); return 0; }
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_depth_line(const char* name, uint32_t start, uint32_t end, uint32_t depth, char* out, uint32_t capacity, uint32_t* bytes) {
	if (!name || !out || !bytes) { g_error = "null argument"; return -1; }
	const std::string line = depth_line_text(name, start, end, depth);
	*bytes = (uint32_t) line.size();
	if (line.size() > capacity) { g_error = "ahost_depth_line: the line does not fit the buffer"; return -1; }
	memcpy(out, line.data(), line.size());
	return 0;
}
int ahost_depth_write(const void* text, uint64_t bytes, const char* path) {
	if ((!text && bytes > 0) || !path) { g_error = "null argument"; return -1; }
	try { virus_expression_write(std::string((const char*) text, bytes), path); return 0; } // (the writer of a text through path.tmp)
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_depth_file(const char* input_path, const char* path, agpu_depth_stats* stats) {
	if (!input_path || !path) { g_error = "null argument"; return -1; }
	try {
		std::vector<uint8_t> stream;
		const uint64_t at = read_whole_bam(input_path, stream); // (SAM text comes out as the BAM stream of its alignments, behind a BAM header)
		DepthContigs contigs; std::string text; agpu_depth_stats counted;
		depth_contigs_of(stream.data(), at, contigs);
		depth_track(stream.data() + at, stream.size() - at, contigs.view(), text, counted);
		virus_expression_write(text, path);
		if (stats) *stats = counted;
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}

// ---- --gene-counts (include/arriba_host.h) ----
namespace {
thread_local std::string g_gene_count_text, g_gene_ids;
GeneCountAnnotation gene_count_annotation(ahost_session* session) {
	if (session->annotation.real_genes == 0) throw std::runtime_error("gene counts need the annotation of the session");
	if (session->gene_bits.size() < session->annotation.real_genes || session->exon_gene.size() != session->annotation.exons.size()) throw std::runtime_error("gene counts: the views of the annotation are not built");
	GeneCountAnnotation annotation; annotation.view = agpu::AnnotationView(); // (every pointer null)
	agpu::AnnotationView& v = annotation.view;
	v.n_genes = (uint32_t) session->annotation.real_genes; v.n_dummy = (uint32_t) (session->annotation.genes.size() - session->annotation.real_genes);
	v.gene_bits = session->gene_bits.data(); v.n_exons = (uint32_t) session->exon_gene.size(); v.exon_gene = session->exon_gene.data();
	const FlatIndex& index = session->exon_index;
	v.exon_index.n_contigs = (uint32_t) index.n_contigs(); v.exon_index.contig_offset = index.contig_offset.data(); v.exon_index.keys = index.keys.data();
	v.exon_index.member_offset = index.member_offset.data(); v.exon_index.members = index.members.data(); v.exon_index.bins = nullptr;
	return annotation;
}
std::vector<std::string> gene_count_ids(ahost_session* session) {
	std::vector<std::string> ids;
	for (size_t g = 0; g < session->annotation.real_genes; ++g) ids.push_back(session->annotation.genes[g].gene_id);
	return ids;
}
// the references of a header against the contigs of the session (which is not changed: a name it does not know gets no contig, and so no exon)
void gene_count_references(ahost_session* session, const uint8_t* header, size_t size, std::vector<uint32_t>& tid_to_contig, std::vector<uint32_t>& ref_length) {
	std::vector<std::string> names;
	header_contigs(header, size, names, ref_length);
	tid_to_contig.assign(names.size(), 0xFFFFFFFFu);
	for (size_t t = 0; t < names.size(); ++t) { std::map<std::string, contig_t>::const_iterator known = session->contigs.by_name.find(remove_chr(names[t])); if (known != session->contigs.by_name.end()) tid_to_contig[t] = known->second; }
}
void gene_counts_checked(ahost_session* session, const uint64_t* counts, uint64_t n_counts) {
	if (n_counts != 3 * ((uint64_t) session->annotation.real_genes + 4)) throw std::runtime_error("gene counts: the table has 3 x (n_genes + 4) numbers, n_genes = " + std::to_string(session->annotation.real_genes));
}
}
int ahost_gene_counts_genes(ahost_session* session, uint32_t* n_genes, const char** ids, uint64_t* bytes) {
	if (!session || !n_genes) { g_error = "null argument"; return -1; }
	*n_genes = (uint32_t) session->annotation.real_genes;
	g_gene_ids.clear();
	for (size_t g = 0; g < session->annotation.real_genes; ++g) { g_gene_ids += session->annotation.genes[g].gene_id; g_gene_ids += '\n'; }
	if (ids) *ids = g_gene_ids.data();
	if (bytes) *bytes = g_gene_ids.size();
	return 0;
}
int ahost_gene_counts_of(ahost_session* session, const void* input_header, size_t header_size, const void* records, size_t size, uint64_t* counts, uint64_t n_counts, agpu_gene_count_stats* stats) {
	if (!session || (!input_header && header_size > 0) || (!records && size > 0) || !counts) { g_error = "null argument"; return -1; }
	try {
		gene_counts_checked(session, counts, n_counts);
		std::vector<uint32_t> tid_to_contig, ref_length; std::vector<uint64_t> counted; agpu_gene_count_stats counted_stats;
		gene_count_references(session, (const uint8_t*) input_header, header_size, tid_to_contig, ref_length);
		gene_counts_of(gene_count_annotation(session), tid_to_contig, ref_length, (const uint8_t*) records, size, counted, counted_stats);
		memcpy(counts, counted.data(), counted.size() * 8);
		if (stats) *stats = counted_stats;
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_gene_counts_text(ahost_session* session, const uint64_t* counts, uint64_t n_counts, const char** text, uint64_t* bytes) {
	if (!session || !counts || !text || !bytes) { g_error = "null argument"; return -1; }
	try { gene_counts_checked(session, counts, n_counts); g_gene_count_text = gene_counts_text(gene_count_ids(session), counts); *text = g_gene_count_text.data(); *bytes = g_gene_count_text.size(); return 0; }
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_gene_counts_write(ahost_session* session, const uint64_t* counts, uint64_t n_counts, const char* path) {
	if (!session || !counts || !path) { g_error = "null argument"; return -1; }
	try { gene_counts_checked(session, counts, n_counts); virus_expression_write(gene_counts_text(gene_count_ids(session), counts), path); return 0; } // (the writer of a text through path.tmp)
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_gene_counts_file(ahost_session* session, const char* input_path, const char* path, agpu_gene_count_stats* stats) {
	if (!session || !input_path || !path) { g_error = "null argument"; return -1; }
	try {
		std::vector<uint8_t> stream;
		const uint64_t at = read_whole_bam(input_path, stream); // (SAM text comes out as the BAM stream of its alignments, behind a BAM header)
		std::vector<uint32_t> tid_to_contig, ref_length; std::vector<uint64_t> counted; agpu_gene_count_stats counted_stats;
		gene_count_references(session, stream.data(), at, tid_to_contig, ref_length);
		gene_counts_of(gene_count_annotation(session), tid_to_contig, ref_length, stream.data() + at, stream.size() - at, counted, counted_stats);
		virus_expression_write(gene_counts_text(gene_count_ids(session), counted.data()), path);
		if (stats) *stats = counted_stats;
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}

// ---- --splice-junctions (include/arriba_host.h) ----
namespace {
thread_local std::vector<agpu_junction_row> g_junction_rows; thread_local std::string g_junction_text;
JunctionReferences junction_references(ahost_session* session) {
	if (session->gene_bits.size() < session->annotation.real_genes || session->gene_contig.size() < session->annotation.real_genes || session->exon_gene.size() != session->annotation.exons.size()
	    || session->exon_next.size() != session->annotation.exons.size()) throw std::runtime_error("splice junctions: the views of the annotation are not built");
	JunctionReferences references; references.view = agpu::AnnotationView(); // (every pointer null)
	agpu::AnnotationView& v = references.view;
	v.n_genes = (uint32_t) session->annotation.real_genes; v.n_dummy = (uint32_t) (session->annotation.genes.size() - session->annotation.real_genes);
	v.gene_bits = session->gene_bits.data(); v.gene_contig = session->gene_contig.data();
	v.n_exons = (uint32_t) session->exon_gene.size(); v.exon_gene = session->exon_gene.data(); v.exon_start = session->exon_start.data(); v.exon_end = session->exon_end.data(); v.exon_next = session->exon_next.data();
	// the assembly as the genome view holds it: the contigs the view was built with (a contig the session learnt of later has no bases)
	agpu::GenomeView& g = references.genome;
	g.n_contigs = session->genome_offset.empty() ? 0 : (uint32_t) (session->genome_offset.size() - 1); g.contig_offset = session->genome_offset.data(); g.contig_bits = session->contig_bits.data(); g.bases = session->genome_bases.data();
	return references;
}
void splice_junctions_with_header(ahost_session* session, const uint8_t* header, size_t header_size, const uint8_t* records, size_t size, std::vector<agpu_junction_row>& rows, agpu_junction_stats& stats) {
	std::vector<uint32_t> tid_to_contig, ref_length;
	gene_count_references(session, header, header_size, tid_to_contig, ref_length);
	splice_junctions_of(junction_references(session), tid_to_contig, ref_length, records, size, rows, stats);
}
}
int ahost_splice_junctions_of(ahost_session* session, const void* input_header, size_t header_size, const void* records, size_t size, const agpu_junction_row** rows, uint64_t* n_rows, agpu_junction_stats* stats) {
	if (!session || (!input_header && header_size > 0) || (!records && size > 0) || !rows || !n_rows) { g_error = "null argument"; return -1; }
	try {
		agpu_junction_stats counted;
		splice_junctions_with_header(session, (const uint8_t*) input_header, header_size, (const uint8_t*) records, size, g_junction_rows, counted);
		*rows = g_junction_rows.data(); *n_rows = g_junction_rows.size();
		if (stats) *stats = counted;
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_splice_junctions_text(const ahost_depth_contigs* contigs, const agpu_junction_row* rows, uint64_t n_rows, const char** text, uint64_t* bytes) {
	if (!contigs || (!rows && n_rows > 0) || !text || !bytes) { g_error = "null argument"; return -1; }
	try { g_junction_text = splice_junctions_text(*contigs, rows, n_rows); *text = g_junction_text.data(); *bytes = g_junction_text.size(); return 0; }
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_splice_junctions_write(const ahost_depth_contigs* contigs, const agpu_junction_row* rows, uint64_t n_rows, const char* path) {
	if (!contigs || (!rows && n_rows > 0) || !path) { g_error = "null argument"; return -1; }
	try { virus_expression_write(splice_junctions_text(*contigs, rows, n_rows), path); return 0; } // (the writer of a text through path.tmp)
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_splice_junctions_file(ahost_session* session, const char* input_path, const char* path, agpu_junction_stats* stats) {
	if (!session || !input_path || !path) { g_error = "null argument"; return -1; }
	try {
		std::vector<uint8_t> stream;
		const uint64_t at = read_whole_bam(input_path, stream); // (SAM text comes out as the BAM stream of its alignments, behind a BAM header)
		std::vector<agpu_junction_row> rows; agpu_junction_stats counted;
		splice_junctions_with_header(session, stream.data(), at, stream.data() + at, stream.size() - at, rows, counted);
		DepthContigs contigs;
		depth_contigs_of(stream.data(), at, contigs);
		virus_expression_write(splice_junctions_text(contigs.view(), rows.data(), rows.size()), path);
		if (stats) *stats = counted;
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}

// ---- --allele-counts (include/arriba_host.h) ----
namespace {
thread_local std::vector<agpu_allele_row> g_allele_rows; thread_local std::string g_allele_text;
agpu::GenomeView allele_genome(ahost_session* session) { // the assembly as the genome view holds it (a contig the session learnt of later has no bases)
	agpu::GenomeView g;
	g.n_contigs = session->genome_offset.empty() ? 0 : (uint32_t) (session->genome_offset.size() - 1); g.contig_offset = session->genome_offset.data(); g.contig_bits = session->contig_bits.data(); g.bases = session->genome_bases.data();
	return g;
}
void allele_sites_view(AlleleSiteList* list, ahost_allele_sites* sites) {
	sites->n_sites = list->sites.size(); sites->placed = list->placed; sites->sites = list->sites.data(); sites->names = list->names.data(); sites->name_offset = list->name_offset.data(); sites->owner = list;
}
const AlleleSiteList& allele_list_of(const ahost_allele_sites* sites) {
	if (!sites->owner) throw std::runtime_error("allele counts: the list of sites was not loaded by ahost_allele_sites_load");
	return *(const AlleleSiteList*) sites->owner;
}
void allele_counts_with_header(ahost_session* session, const uint8_t* header, size_t header_size, const uint8_t* records, size_t size, const AlleleSiteList& list, uint32_t min_mapq, uint32_t min_baseq,
                               std::vector<agpu_allele_row>& rows, agpu_allele_stats& stats) {
	std::vector<uint32_t> tid_to_contig, ref_length;
	if (header_size > 0) gene_count_references(session, header, header_size, tid_to_contig, ref_length);
	allele_counts_of(allele_genome(session), tid_to_contig, ref_length, list.sites.data(), list.sites.size(), records, size, min_mapq, min_baseq, rows, stats);
}
}
int ahost_allele_sites_load(const char* path, const void* input_header, size_t header_size, ahost_allele_sites* sites) {
	if (!path || !sites || (!input_header && header_size > 0)) { g_error = "null argument"; return -1; }
	memset(sites, 0, sizeof(*sites));
	try {
		std::unique_ptr<AlleleSiteList> list(new AlleleSiteList());
		allele_sites_parse(path, *list);
		list->place((const uint8_t*) input_header, header_size);
		allele_sites_view(list.release(), sites);
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_allele_sites_place_session(ahost_session* session, ahost_allele_sites* sites) {
	if (!session || !sites || !sites->owner) { g_error = "null argument"; return -1; }
	if (session->input_header.empty()) { g_error = "ahost_bam_open must run first"; return -1; }
	try { AlleleSiteList* list = (AlleleSiteList*) sites->owner; list->place(session->input_header.data(), session->input_header.size()); allele_sites_view(list, sites); return 0; }
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}
void ahost_allele_sites_free(ahost_allele_sites* sites) { if (sites) { delete (AlleleSiteList*) sites->owner; memset(sites, 0, sizeof(*sites)); } }
int ahost_allele_counts_of(ahost_session* session, const void* input_header, size_t header_size, const void* records, size_t size, const ahost_allele_sites* sites, uint32_t min_mapq, uint32_t min_baseq,
                           const agpu_allele_row** rows, agpu_allele_stats* stats) {
	if (!session || (!input_header && header_size > 0) || (!records && size > 0) || !sites || !rows) { g_error = "null argument"; return -1; }
	try {
		agpu_allele_stats counted;
		allele_counts_with_header(session, (const uint8_t*) input_header, header_size, (const uint8_t*) records, size, allele_list_of(sites), min_mapq, min_baseq, g_allele_rows, counted);
		*rows = g_allele_rows.data();
		if (stats) *stats = counted;
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_allele_counts_text(const ahost_allele_sites* sites, const agpu_allele_row* rows, uint64_t n_rows, const char** text, uint64_t* bytes) {
	if (!sites || (!rows && n_rows > 0) || !text || !bytes) { g_error = "null argument"; return -1; }
	try { g_allele_text = allele_counts_text(allele_list_of(sites), rows, n_rows); *text = g_allele_text.data(); *bytes = g_allele_text.size(); return 0; }
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_allele_counts_write(const ahost_allele_sites* sites, const agpu_allele_row* rows, uint64_t n_rows, const char* path) {
	if (!sites || (!rows && n_rows > 0) || !path) { g_error = "null argument"; return -1; }
	try { virus_expression_write(allele_counts_text(allele_list_of(sites), rows, n_rows), path); return 0; } // (the writer of a text through path.tmp)
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_allele_counts_file(ahost_session* session, const char* input_path, const char* sites_path, const char* path, uint32_t min_mapq, uint32_t min_baseq, agpu_allele_stats* stats) {
	if (!session || !input_path || !sites_path || !path) { g_error = "null argument"; return -1; }
	try {
		AlleleSiteList list;
		allele_sites_parse(sites_path, list); // (refused before the input is read)
		std::vector<uint8_t> stream;
		const uint64_t at = read_whole_bam(input_path, stream); // (SAM text comes out as the BAM stream of its alignments, behind a BAM header)
		list.place(stream.data(), at);
		std::vector<agpu_allele_row> rows; agpu_allele_stats counted;
		allele_counts_with_header(session, stream.data(), at, stream.data() + at, stream.size() - at, list, min_mapq, min_baseq, rows, counted);
		virus_expression_write(allele_counts_text(list, rows.data(), rows.size()), path);
		if (stats) *stats = counted;
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}

// ---- --variant-sites (include/arriba_host.h) ----
namespace {
thread_local std::vector<agpu_variant_row> g_variant_rows; thread_local std::string g_variant_text;
void variant_sites_with_header(ahost_session* session, const uint8_t* header, size_t header_size, const uint8_t* records, size_t size, uint32_t min_mapq, uint32_t min_baseq, uint32_t min_alt, uint32_t min_percent,
                               std::vector<agpu_variant_row>& rows, agpu_variant_stats& stats) {
	std::vector<uint32_t> tid_to_contig, ref_length;
	if (header_size > 0) gene_count_references(session, header, header_size, tid_to_contig, ref_length);
	variant_sites_of(allele_genome(session), tid_to_contig, ref_length, records, size, min_mapq, min_baseq, min_alt, min_percent, rows, stats);
}
}
int ahost_variant_sites_of(ahost_session* session, const void* input_header, size_t header_size, const void* records, size_t size, uint32_t min_mapq, uint32_t min_baseq, uint32_t min_alt, uint32_t min_percent,
                           const agpu_variant_row** rows, uint64_t* n_rows, agpu_variant_stats* stats) {
	if (!session || (!input_header && header_size > 0) || (!records && size > 0) || !rows || !n_rows) { g_error = "null argument"; return -1; }
	try {
		agpu_variant_stats found;
		variant_sites_with_header(session, (const uint8_t*) input_header, header_size, (const uint8_t*) records, size, min_mapq, min_baseq, min_alt, min_percent, g_variant_rows, found);
		*rows = g_variant_rows.data(); *n_rows = g_variant_rows.size();
		if (stats) *stats = found;
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_variant_sites_text(const ahost_depth_contigs* contigs, const agpu_variant_row* rows, uint64_t n_rows, const char** text, uint64_t* bytes) {
	if (!contigs || (!rows && n_rows > 0) || !text || !bytes) { g_error = "null argument"; return -1; }
	try { g_variant_text = variant_sites_text(*contigs, rows, n_rows); *text = g_variant_text.data(); *bytes = g_variant_text.size(); return 0; }
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_variant_sites_write(const ahost_depth_contigs* contigs, const agpu_variant_row* rows, uint64_t n_rows, const char* path) {
	if (!contigs || (!rows && n_rows > 0) || !path) { g_error = "null argument"; return -1; }
	try { virus_expression_write(variant_sites_text(*contigs, rows, n_rows), path); return 0; } // (the writer of a text through path.tmp)
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_variant_sites_file(ahost_session* session, const char* input_path, const char* path, uint32_t min_mapq, uint32_t min_baseq, uint32_t min_alt, uint32_t min_percent, agpu_variant_stats* stats) {
	if (!session || !input_path || !path) { g_error = "null argument"; return -1; }
	try {
		std::vector<uint8_t> stream;
		const uint64_t at = read_whole_bam(input_path, stream); // (SAM text comes out as the BAM stream of its alignments, behind a BAM header)
		std::vector<agpu_variant_row> rows; agpu_variant_stats found;
		variant_sites_with_header(session, stream.data(), at, stream.data() + at, stream.size() - at, min_mapq, min_baseq, min_alt, min_percent, rows, found);
		DepthContigs contigs;
		depth_contigs_of(stream.data(), at, contigs);
		virus_expression_write(variant_sites_text(contigs.view(), rows.data(), rows.size()), path);
		if (stats) *stats = found;
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}

// ---- --indel-sites (include/arriba_host.h) ----
namespace {
thread_local std::vector<agpu_indel_row> g_indel_rows; thread_local std::string g_indel_text;
void indel_sites_with_header(ahost_session* session, const uint8_t* header, size_t header_size, const uint8_t* records, size_t size, uint32_t min_mapq, uint32_t min_alt, uint32_t min_percent,
                             std::vector<agpu_indel_row>& rows, agpu_indel_stats& stats) {
	std::vector<uint32_t> tid_to_contig, ref_length;
	if (header_size > 0) gene_count_references(session, header, header_size, tid_to_contig, ref_length);
	indel_sites_of(allele_genome(session), tid_to_contig, ref_length, records, size, min_mapq, min_alt, min_percent, rows, stats);
}
// the text of a row table whose references are `contigs`: they are looked up among the contigs of the session by name, as gene_count_references looks up those of a header
std::string indel_sites_text_of(ahost_session* session, const ahost_depth_contigs& contigs, const agpu_indel_row* rows, uint64_t n_rows) {
	std::vector<uint32_t> tid_to_contig(contigs.n_ref, 0xFFFFFFFFu);
	for (uint32_t t = 0; t < contigs.n_ref; ++t) {
		std::map<std::string, contig_t>::const_iterator known = session->contigs.by_name.find(remove_chr(std::string(contigs.names + contigs.name_offset[t], contigs.name_offset[t + 1] - contigs.name_offset[t])));
		if (known != session->contigs.by_name.end()) tid_to_contig[t] = known->second;
	}
	return indel_sites_text(allele_genome(session), tid_to_contig, contigs, rows, n_rows);
}
}
int ahost_indel_sites_of(ahost_session* session, const void* input_header, size_t header_size, const void* records, size_t size, uint32_t min_mapq, uint32_t min_alt, uint32_t min_percent,
                         const agpu_indel_row** rows, uint64_t* n_rows, agpu_indel_stats* stats) {
	if (!session || (!input_header && header_size > 0) || (!records && size > 0) || !rows || !n_rows) { g_error = "null argument"; return -1; }
	try {
		agpu_indel_stats found;
		indel_sites_with_header(session, (const uint8_t*) input_header, header_size, (const uint8_t*) records, size, min_mapq, min_alt, min_percent, g_indel_rows, found);
		*rows = g_indel_rows.data(); *n_rows = g_indel_rows.size();
		if (stats) *stats = found;
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_indel_sites_text(ahost_session* session, const ahost_depth_contigs* contigs, const agpu_indel_row* rows, uint64_t n_rows, const char** text, uint64_t* bytes) {
	if (!session || !contigs || (!rows && n_rows > 0) || !text || !bytes) { g_error = "null argument"; return -1; }
	try { g_indel_text = indel_sites_text_of(session, *contigs, rows, n_rows); *text = g_indel_text.data(); *bytes = g_indel_text.size(); return 0; }
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_indel_sites_write(ahost_session* session, const ahost_depth_contigs* contigs, const agpu_indel_row* rows, uint64_t n_rows, const char* path) {
	if (!session || !contigs || (!rows && n_rows > 0) || !path) { g_error = "null argument"; return -1; }
	try { virus_expression_write(indel_sites_text_of(session, *contigs, rows, n_rows), path); return 0; } // (the writer of a text through path.tmp)
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_indel_sites_file(ahost_session* session, const char* input_path, const char* path, uint32_t min_mapq, uint32_t min_alt, uint32_t min_percent, agpu_indel_stats* stats) {
	if (!session || !input_path || !path) { g_error = "null argument"; return -1; }
	try {
		std::vector<uint8_t> stream;
		const uint64_t at = read_whole_bam(input_path, stream); // (SAM text comes out as the BAM stream of its alignments, behind a BAM header)
		std::vector<agpu_indel_row> rows; agpu_indel_stats found;
		indel_sites_with_header(session, stream.data(), at, stream.data() + at, stream.size() - at, min_mapq, min_alt, min_percent, rows, found);
		DepthContigs contigs;
		depth_contigs_of(stream.data(), at, contigs);
		virus_expression_write(indel_sites_text_of(session, contigs.view(), rows.data(), rows.size()), path);
		if (stats) *stats = found;
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}

// ---- --realign-reads (include/arriba_host.h) ----
namespace {
thread_local RealignPlan g_realign_plan; thread_local std::string g_realign_text, g_realign_kept;
void realign_plan_view(ahost_realign_plan* plan) {
	plan->n_ref = (uint32_t) g_realign_plan.in_assembly.size(); plan->in_assembly = g_realign_plan.in_assembly.data(); plan->header = g_realign_plan.header.data(); plan->header_bytes = g_realign_plan.header.size();
}
// both files of a stream through NAME.tmp: on a failure neither is left behind
void realign_write(const std::string& realign, const std::string& kept, const char* realign_path, const char* kept_path) {
	virus_expression_write(realign, realign_path); // (the writer of a text through path.tmp)
	if (kept_path) { try { virus_expression_write(kept, kept_path); } catch (...) { remove(realign_path); throw; } }
}
}
int ahost_realign_plan_of(ahost_session* session, const void* input_header, size_t header_size, ahost_realign_plan* plan) {
	if (!session || !plan || (!input_header && header_size > 0)) { g_error = "null argument"; return -1; }
	try { realign_plan_of(session->assembly, (const uint8_t*) input_header, header_size, g_realign_plan); realign_plan_view(plan); return 0; }
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_realign_plan_of_session(ahost_session* session, ahost_realign_plan* plan) {
	if (!session || !plan) { g_error = "null argument"; return -1; }
	if (session->input_header.empty()) { g_error = "ahost_bam_open must run first"; return -1; }
	return ahost_realign_plan_of(session, session->input_header.data(), session->input_header.size(), plan);
}
int ahost_realign_split_of(ahost_session* session, const void* input_header, size_t header_size, const void* records, size_t size, int want_kept, const char** realign, uint64_t* realign_bytes, const char** kept, uint64_t* kept_bytes,
                           agpu_realign_stats* stats) {
	if (!session || (!input_header && header_size > 0) || (!records && size > 0) || !realign || !realign_bytes || (want_kept && (!kept || !kept_bytes))) { g_error = "null argument"; return -1; }
	try {
		DepthContigs contigs; std::string lines; agpu_realign_stats counted;
		realign_plan_of(session->assembly, (const uint8_t*) input_header, header_size, g_realign_plan);
		if (header_size > 0) depth_contigs_of((const uint8_t*) input_header, header_size, contigs); else contigs.name_offset.push_back(0);
		realign_split_of(g_realign_plan.in_assembly.data(), contigs.view(), (const uint8_t*) records, size, want_kept != 0, g_realign_text, lines, counted);
		*realign = g_realign_text.data(); *realign_bytes = g_realign_text.size();
		if (want_kept) { g_realign_kept = g_realign_plan.header + lines; *kept = g_realign_kept.data(); *kept_bytes = g_realign_kept.size(); }
		if (stats) *stats = counted;
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_realign_split_file(ahost_session* session, const char* input_path, const char* realign_path, const char* kept_path, agpu_realign_stats* stats) {
	if (!session || !input_path || !realign_path) { g_error = "null argument"; return -1; }
	try {
		std::vector<uint8_t> stream;
		const uint64_t at = read_whole_bam(input_path, stream); // (SAM text comes out as the BAM stream of its alignments, behind a BAM header)
		RealignPlan plan; DepthContigs contigs; std::string realign, kept; agpu_realign_stats counted;
		realign_plan_of(session->assembly, stream.data(), at, plan);
		depth_contigs_of(stream.data(), at, contigs);
		realign_split_of(plan.in_assembly.data(), contigs.view(), stream.data() + at, stream.size() - at, kept_path != nullptr, realign, kept, counted);
		realign_write(realign, plan.header + kept, realign_path, kept_path);
		if (stats) *stats = counted;
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}

// ---- --rna-metrics (include/arriba_host.h) ----
namespace {
thread_local std::string g_rna_metrics_text;
// the track of the session for an interval file (NULL or "": no rRNA intervals), built and kept when it is asked for first
const RegionTrack& region_track_of(ahost_session* session, const char* rrna_intervals_path) {
	const std::string key = rrna_intervals_path ? rrna_intervals_path : "";
	std::lock_guard<std::mutex> lock(session->region_track_mutex);
	std::unique_ptr<RegionTrack>& slot = session->region_tracks[key];
	if (!slot) {
		try {
			std::vector<RrnaInterval> intervals;
			if (!key.empty()) rrna_intervals_parse(key, intervals);
			std::unique_ptr<RegionTrack> built(new RegionTrack());
			region_track_build(session->annotation, session->contigs, session->contigs_at_open, intervals, *built);
			slot = std::move(built);
		} catch (...) { session->region_tracks.erase(key); throw; }
	}
	return *slot;
}
void rna_metrics_checked(uint64_t n_counters) { if (n_counters != AGPU_RNA_METRICS_WORDS) throw std::runtime_error("rna metrics: a counter block has " + std::to_string((unsigned) AGPU_RNA_METRICS_WORDS) + " words"); }
}
int ahost_rrna_intervals_load(const char* path, uint64_t* n_intervals) {
	if (!path) { g_error = "null argument"; return -1; }
	try { std::vector<RrnaInterval> intervals; rrna_intervals_parse(path, intervals); if (n_intervals) *n_intervals = intervals.size(); return 0; }
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_region_track(ahost_session* session, const char* rrna_intervals_path, agpu_region_track* track, ahost_region_track_info* info) {
	if (!session || !track) { g_error = "null argument"; return -1; }
	try {
		const RegionTrack& built = region_track_of(session, rrna_intervals_path);
		*track = built.view();
		if (info) {
			info->n_contigs = track->n_contigs; info->runs = track->n_runs; info->intervals = built.intervals; info->intervals_unknown_contig = built.intervals_unknown_contig;
			info->bytes = (uint64_t) (track->n_contigs + 1) * 4 + (uint64_t) track->n_runs * 13 + (uint64_t) track->n_genes * 4;
		}
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_rna_metrics_of(ahost_session* session, const char* rrna_intervals_path, const void* input_header, size_t header_size, const void* records, size_t size, uint64_t* counters, uint64_t n_counters, agpu_rna_metrics_stats* stats) {
	if (!session || (!input_header && header_size > 0) || (!records && size > 0) || !counters) { g_error = "null argument"; return -1; }
	try {
		rna_metrics_checked(n_counters);
		const RegionTrack& track = region_track_of(session, rrna_intervals_path);
		std::vector<uint32_t> tid_to_contig, ref_length; std::vector<uint64_t> counted; agpu_rna_metrics_stats counted_stats;
		if (header_size > 0) gene_count_references(session, (const uint8_t*) input_header, header_size, tid_to_contig, ref_length);
		rna_metrics_of(track.view(), tid_to_contig, ref_length, (const uint8_t*) records, size, counted, counted_stats);
		memcpy(counters, counted.data(), counted.size() * 8);
		if (stats) *stats = counted_stats;
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_rna_metrics_text(const uint64_t* counters, uint64_t n_counters, const char** text, uint64_t* bytes) {
	if (!counters || !text || !bytes) { g_error = "null argument"; return -1; }
	try { rna_metrics_checked(n_counters); g_rna_metrics_text = rna_metrics_text(counters); *text = g_rna_metrics_text.data(); *bytes = g_rna_metrics_text.size(); return 0; }
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_rna_metrics_write(const uint64_t* counters, uint64_t n_counters, const char* path) {
	if (!counters || !path) { g_error = "null argument"; return -1; }
	try { rna_metrics_checked(n_counters); virus_expression_write(rna_metrics_text(counters), path); return 0; } // (the writer of a text through path.tmp)
	catch (const std::exception& e) { g_error = e.what(); return -1; }
}
int ahost_rna_metrics_file(ahost_session* session, const char* input_path, const char* rrna_intervals_path, const char* path, agpu_rna_metrics_stats* stats) {
	if (!session || !input_path || !path) { g_error = "null argument"; return -1; }
	try {
		const RegionTrack& track = region_track_of(session, rrna_intervals_path); // (an interval file that does not parse is refused before the input is read)
		std::vector<uint8_t> stream;
		const uint64_t at = read_whole_bam(input_path, stream); // (SAM text comes out as the BAM stream of its alignments, behind a BAM header)
		std::vector<uint32_t> tid_to_contig, ref_length; std::vector<uint64_t> counted; agpu_rna_metrics_stats counted_stats;
		gene_count_references(session, stream.data(), at, tid_to_contig, ref_length);
		rna_metrics_of(track.view(), tid_to_contig, ref_length, stream.data() + at, stream.size() - at, counted, counted_stats);
		virus_expression_write(rna_metrics_text(counted.data()), path);
		if (stats) *stats = counted_stats;
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}

void ahost_bam_close(ahost_session* session) { if (session && session->feed) { close_bam_feed(session->feed); session->feed = nullptr; } }

int ahost_adopt_device_ingest(ahost_session* session, const agpu_ingest_result* result, const uint64_t* viral_read_counts, const uint16_t* coverage, const uint8_t* fragment_starts, const uint8_t* fragment_ends) {
	if (!session || !result) { g_error = "null argument"; return -1; }
	try {
		IngestResult& r = session->ingest;
		r.records = result->records; r.mapped_reads = result->mapped_reads; r.malformed_count = (unsigned int) result->malformed_count; r.missing_hi_tag = (unsigned int) result->missing_hi_tag;
		r.mapped_viral_reads_by_contig.assign(session->contigs.size(), 0);
		if (viral_read_counts) for (size_t contig = 0; contig < session->contigs.size(); ++contig) r.mapped_viral_reads_by_contig[contig] = viral_read_counts[contig];
		// reference: source/read_chimeric_alignments.cpp:759-771
		if (r.mapped_reads == 0) throw std::runtime_error("no normal reads found");
		if (r.malformed_count > 0) std::cerr << "WARNING: " << r.malformed_count << " SAM records were malformed and ignored" << std::endl;
		if (result->no_chimeric_reads) throw std::runtime_error("no split reads or discordant mates found (STAR must either be run with '--chimOutType WithinBAM' or the file 'Chimeric.out.sam' must be passed to Arriba via the argument -c)");
		if (r.missing_hi_tag > 0) std::cerr << "WARNING: " << r.missing_hi_tag << " secondary alignments lack the 'HI' tag and were ignored (STAR must be run with '--outSAMattributes HI' for Arriba to make use of multi-mapping reads for fusion detection)" << std::endl;
		Coverage& c = r.coverage;
		for (size_t contig = 0; contig < c.coverage.size() && contig + 1 < session->window_offset.size(); ++contig) {
			const uint64_t begin = session->window_offset[contig], size = session->window_offset[contig + 1] - begin;
			if (size != c.coverage[contig].size()) throw std::runtime_error("coverage_t: the windows of the device do not match the session's");
			if (size == 0) continue; // (a contig without sequence has no windows)
			if (coverage) memcpy(c.coverage[contig].data(), coverage + begin, size * sizeof(uint16_t));
			if (fragment_starts) memcpy(c.fragment_starts[contig].data(), fragment_starts + begin, size);
			if (fragment_ends) memcpy(c.fragment_ends[contig].data(), fragment_ends + begin, size);
		}
		r.batch = Batch();
		r.batch.n = 0;
		session->row_fragments.clear(); session->rows_in_list_order = false;
		session->device_batch = true;
		session->have_batch = true; // (an empty host batch: the fragments live on the device; ahost_set_batch_rows brings the rows the writer needs)
		session->build_batch_view();
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}

int ahost_set_batch_rows(ahost_session* session, const agpu_batch_rows* rows, const uint32_t* fragments) {
	if (!session || !rows) { g_error = "null argument"; return -1; }
	if (session->sample_was_detached) { g_error = "the sample of this session was detached for its writer (ahost_detach_sample): nothing to set rows of until the next ingest"; return -1; }
	try {
		Batch& b = session->ingest.batch;
		// every member is assigned below.  The vectors of the last sample's rows come back first (ahost_bam_open put them aside): a gigabyte of fresh vectors per sample is mapped,
		// zero-filled by resize() and faulted in page by page -- 0.34 s for the 9.3 M rows of a 10^8-fragment sample, of which the copy itself is a tenth (profiles/r03p_writer_laps.txt)
		{ std::lock_guard<std::mutex> lock(session->detached_mutex); if (session->spare_rows.seq_pool.capacity() > b.seq_pool.capacity()) b = std::move(session->spare_rows); }
		const size_t n = rows->n;
		b.n = n;
		// the columns and pools of 10^7 rows are more than a gigabyte: the vectors are sized first, the bytes then copied by all threads the process may use
		struct Copy { void* to; const void* from; size_t bytes; };
		std::vector<Copy> copies;
		auto take = [&copies](auto& column, const void* from, size_t count) {
			column.resize(count);
			if (count > 0) { Copy copy = { &column[0], from, count * sizeof(column[0]) }; copies.push_back(copy); }
		};
		take(b.n_aln, rows->n_aln, n); take(b.fbits, rows->fbits, n); b.filter.assign(n, 0); take(b.group, rows->group, n);
		for (int s = 0; s < 3; ++s) {
			take(b.contig[s], rows->contig[s], n); take(b.start[s], rows->start[s], n); take(b.end[s], rows->end[s], n); take(b.abits[s], rows->abits[s], n);
			take(b.cigar_offset[s], rows->cigar_offset[s], n); take(b.cigar_count[s], rows->cigar_count[s], n);
		}
		take(b.cigar_pool, rows->cigar_pool, rows->cigar_pool_size);
		for (int s = 0; s < 2; ++s) { take(b.seq_offset[s], rows->seq_offset[s], n); take(b.seq_length[s], rows->seq_length[s], n); }
		take(b.seq_pool, rows->seq_pool, rows->seq_pool_size);
		take(b.name_offset, rows->name_offset, n + 1);
		take(b.names, rows->names, rows->names_size);
		size_t total = 0;
		for (size_t k = 0; k < copies.size(); ++k) total += copies[k].bytes;
		const unsigned int n_threads = total < (64u << 20) ? 1u : std::max(1u, std::min(cpu_budget(), 32u));
		if (n_threads == 1) for (size_t k = 0; k < copies.size(); ++k) memcpy(copies[k].to, copies[k].from, copies[k].bytes);
		else { // every thread takes the same share of the bytes, across the boundaries of the columns
			std::vector<std::thread> threads;
			for (unsigned int t = 0; t < n_threads; ++t)
				threads.push_back(std::thread([&copies, total, n_threads, t] {
					const size_t first = total / n_threads * t, last = t + 1 == n_threads ? total : total / n_threads * (t + 1);
					size_t at = 0;
					for (size_t k = 0; k < copies.size() && at < last; at += copies[k].bytes, ++k) {
						const size_t from = std::max(first, at), to = std::min(last, at + copies[k].bytes);
						if (from < to) memcpy((char*) copies[k].to + (from - at), (const char*) copies[k].from + (from - at), to - from);
					}
				}));
			for (size_t t = 0; t < threads.size(); ++t) threads[t].join();
		}
		session->rows_in_list_order = fragments == NULL;
		if (fragments != NULL) {
			session->row_fragments.assign(fragments, fragments + n);
			for (size_t k = 1; k < n; ++k) if (fragments[k] <= fragments[k - 1]) throw std::runtime_error("fragments of the rows must ascend");
		} else session->row_fragments.clear();
		session->have_batch = true;
		session->build_batch_view();
		return 0;
	} catch (const std::exception& e) { g_error = e.what(); return -1; }
}

int ahost_ingest_bam_memory(ahost_session* session, const uint8_t* data, size_t size, int external_duplicate_marking, unsigned int max_itd_length) {
	return ingest(session, text_or_bam_source(open_memory_source(data, size)), external_duplicate_marking, max_itd_length);
}

const agpu_annotation_view* ahost_annotation_view(ahost_session* session) { return &session->annotation_view; }
const agpu_genome_view* ahost_genome_view(ahost_session* session) { return &session->genome_view; }
const agpu_coverage_view* ahost_coverage_view(ahost_session* session) {
	if (!session->have_batch) return NULL;
	try { session->build_coverage_view(); } catch (const std::exception& e) { g_error = e.what(); return NULL; }
	return &session->coverage_view;
}
const agpu_batch_view* ahost_batch_view(ahost_session* session) { return session->have_batch ? &session->batch_view : NULL; }
uint64_t ahost_shard_boundary(ahost_session* session, uint64_t target) {
	const agpu_batch_view& v = session->batch_view;
	if (!session->have_batch || target >= v.n) return session->have_batch ? v.n : 0;
	while (target > 0 && target < v.n && v.group[target - 1] == v.group[target]) ++target; // fragments of one read name (multi-mappers) stay together
	return target;
}
const agpu_batch_view* ahost_batch_slice_view(ahost_session* session, uint64_t first, uint64_t count) {
	if (!session->have_batch || first > session->batch_view.n || count > session->batch_view.n - first) { g_error = "slice out of range"; return NULL; }
	agpu_batch_view& v = session->slice_view;
	v = session->batch_view; // the CIGAR and sequence pools are shared, the per-fragment columns are offset
	v.n = count; v.n_aln += first; v.fbits += first; v.group += first;
	for (int k = 0; k < 3; ++k) { v.contig[k] += first; v.start[k] += first; v.end[k] += first; v.abits[k] += first; v.cigar_offset[k] += first; v.cigar_count[k] += first; }
	for (int k = 0; k < 2; ++k) { v.seq_offset[k] += first; v.seq_length[k] += first; }
	return &v;
}
uint64_t ahost_fragment_count(ahost_session* session) { return session->ingest.batch.n; }
uint64_t ahost_mapped_reads(ahost_session* session) { return session->ingest.mapped_reads; }
uint64_t ahost_viral_read_total(ahost_session* session) { uint64_t total = 0; for (size_t c = 0; c < session->ingest.mapped_viral_reads_by_contig.size(); ++c) total += session->ingest.mapped_viral_reads_by_contig[c]; return total; }
uint64_t ahost_coverage_checksum(ahost_session* session) {
	uint64_t hash = 1469598103934665603ull;
	auto mix = [&hash](const uint8_t* bytes, size_t n) { for (size_t i = 0; i < n; ++i) hash = (hash ^ bytes[i]) * 1099511628211ull; };
	const Coverage& coverage = session->ingest.coverage;
	for (size_t contig = 0; contig < coverage.coverage.size(); ++contig) {
		mix((const uint8_t*) coverage.coverage[contig].data(), coverage.coverage[contig].size() * sizeof(uint16_t));
		if (contig < coverage.fragment_starts.size()) mix(coverage.fragment_starts[contig].data(), coverage.fragment_starts[contig].size());
		if (contig < coverage.fragment_ends.size()) mix(coverage.fragment_ends[contig].data(), coverage.fragment_ends[contig].size());
	}
	return hash;
}
uint32_t ahost_contig_count(ahost_session* session) { return session->contigs.size(); }
const char* ahost_contig_name(ahost_session* session, uint32_t contig) { return contig < session->contigs.original_names.size() ? session->contigs.original_names[contig].c_str() : ""; }
const char* ahost_fragment_name(ahost_session* session, uint64_t i, uint32_t* length) {
	const Batch& b = session->ingest.batch;
	if (i >= b.n) { if (length) *length = 0; return ""; }
	if (length) *length = b.name_offset[i + 1] - b.name_offset[i];
	return b.names.data() + b.name_offset[i];
}

// reference: source/read_stats.cpp:94-143
int ahost_detect_strandedness(ahost_session* session) {
	const Batch& b = session->ingest.batch;
	const unsigned int sample_size = 100;
	const float threshold = 0.95;
	unsigned int count = 0, matching_strand = 0;
	std::vector<uint32_t> genes;
	for (size_t i = 0; i < b.n; ++i) {
		if (b.n_aln[i] != 3) continue;
		bool split_strand = b.abits[SPLIT_READ][i] & ABIT_STRAND, supp_strand = b.abits[SUPPLEMENTARY][i] & ABIT_STRAND;
		if (b.contig[SPLIT_READ][i] == b.contig[SUPPLEMENTARY][i] && split_strand == supp_strand && abs(b.start[SPLIT_READ][i] - b.start[SUPPLEMENTARY][i]) < 400000) {
			get_annotation_by_coordinate(b.contig[SPLIT_READ][i], b.start[SPLIT_READ][i], b.end[SPLIT_READ][i], genes, session->gene_index);
			if (genes.size() == 1) {
				bool upstream = split_strand;
				position_t position = split_strand ? b.start[SPLIT_READ][i] : b.end[SPLIT_READ][i];
				if (is_breakpoint_spliced(genes[0], upstream, position, session->annotation, session->exon_index)) {
					bool gene_strand = session->annotation.genes[genes[0]].strand;
					bool mate1_strand = b.abits[MATE1][i] & ABIT_STRAND;
					if ((b.abits[SPLIT_READ][i] & ABIT_FIRST_IN_PAIR) && split_strand == gene_strand || (b.abits[MATE1][i] & ABIT_FIRST_IN_PAIR) && mate1_strand == gene_strand)
						matching_strand++;
					count++;
					if (count >= sample_size) break;
				}
			}
		}
	}
	if (count < sample_size) return 0;
	if (matching_strand < (1 - threshold) * count) return 2;
	if (matching_strand > threshold * count) return 1;
	return 0;
}

int ahost_viral_verdicts(ahost_session* session, const uint32_t* pairs, uint64_t n_pairs, const uint8_t* gene_bits, uint32_t n_genes,
                         unsigned int top_count, float min_covered_fraction, uint8_t* top_verdict, uint8_t* low_verdict) {
	const size_t C = session->contigs.size();
	const std::vector<uint64_t>& mapped = session->ingest.mapped_viral_reads_by_contig;
	const Assembly& assembly = session->assembly;
	std::vector<bool> viral(C);
	for (size_t c = 0; c < C; ++c) viral[c] = session->contig_bits[c] & AGPU_CBIT_VIRAL;

	// ---- filter_top_expressed_viral_contigs, source/filter_top_expressed_viral_contigs.cpp:51-127
	std::vector<float> expression;
	expression.reserve(mapped.size());
	for (size_t c = 0; c < mapped.size(); ++c)
		expression.push_back(assembly.has(c) ? 1.0 * mapped[c] / assembly.sequence[c].size() : 0);
	std::vector<contig_t> sorted;
	for (size_t c = 0; c < expression.size(); ++c) sorted.push_back(c);
	std::sort(sorted.begin(), sorted.end(), [&](contig_t x, contig_t y) { return (expression[x] != expression[y]) ? expression[x] > expression[y] : x > y; });
	unsigned int corrected_top_count = 0;
	for (unsigned int i = 1; i < sorted.size() && expression[sorted[i]] > 0 && top_count > 0; ++i) {
		corrected_top_count++;
		bool related = false;
		if (assembly.has(sorted[i]) && assembly.has(sorted[i - 1])) {
			// relatedness of two viral genomes is a property of the assembly alone: computed once per pair and session
			std::pair<contig_t, contig_t> pair(sorted[i], sorted[i - 1]);
			std::map<std::pair<contig_t, contig_t>, bool>::const_iterator known = session->related_viruses.find(pair);
			if (known == session->related_viruses.end())
				known = session->related_viruses.insert(std::make_pair(pair, related_viral_strains(assembly.sequence[sorted[i]], assembly.sequence[sorted[i - 1]]))).first;
			related = known->second;
		}
		if (!related)
			top_count--;
	}
	if (corrected_top_count != 0) corrected_top_count--;
	float min_expression_threshold = sorted.empty() ? 0 : expression[sorted[corrected_top_count]];
	float min_fraction_intergenic = 0.33;
	unsigned int top_intergenic = 50;
	if (top_intergenic > mapped.size()) top_intergenic = mapped.size();
	top_intergenic = mapped.size() - top_intergenic;
	float min_expression_threshold_intergenic = sorted.empty() ? 0 : expression[sorted[top_intergenic]];
	// distinct host genes hit per viral contig, split into intergenic (dummy) and genic ones (:95-112); one bitmap per viral contig that occurs
	std::vector<std::vector<uint8_t> > seen(C);
	std::vector<unsigned int> intergenic_sites(C, 0), genic_sites(C, 0);
	for (uint64_t p = 0; p < n_pairs; ++p) {
		const uint32_t contig = pairs[2 * p], gene = pairs[2 * p + 1];
		if (contig >= C || gene >= n_genes) continue;
		if (seen[contig].empty()) seen[contig].assign(n_genes, 0);
		if (seen[contig][gene]) continue;
		seen[contig][gene] = 1;
		if (gene_bits[gene] & AGPU_GBIT_DUMMY) intergenic_sites[contig]++; else genic_sites[contig]++;
	}
	std::vector<float> fraction_intergenic(C);
	for (size_t c = 0; c < C; ++c)
		if (intergenic_sites[c] > 0) fraction_intergenic[c] = 1.0 * intergenic_sites[c] / (genic_sites[c] + intergenic_sites[c]);
	for (size_t c = 0; c < C; ++c) {
		bool verdict = false;
		if (viral[c] && c < expression.size())
			if (expression[c] == 0 || expression[c] < min_expression_threshold)
				if (fraction_intergenic[c] < min_fraction_intergenic || expression[c] == 0 || expression[c] < min_expression_threshold_intergenic)
					verdict = true;
		top_verdict[c] = verdict;
	}

	// ---- filter_low_coverage_viral_contigs, source/filter_low_coverage_viral_contigs.cpp:11-43
	const Coverage& coverage = session->ingest.coverage;
	const float min_covered_bases = 100;
	for (size_t c = 0; c < C; ++c) {
		bool verdict = false;
		if (viral[c] && c < coverage.coverage.size()) {
			const std::vector<uint16_t>& windows = coverage.coverage[c];
			float average = 0;
			for (size_t w = 0; w < windows.size(); ++w) average += windows[w];
			average /= windows.size();
			float sufficient = 0;
			for (size_t w = 0; w < windows.size(); ++w)
				if (windows[w] > 0.05 * average) sufficient++;
			if (sufficient / windows.size() < min_covered_fraction || COVERAGE_RESOLUTION * sufficient <= min_covered_bases)
				verdict = true;
		}
		low_verdict[c] = verdict;
	}
	return 0;
}

// reference: source/read_stats.cpp:11-92 and source/arriba.cpp:352-364
float ahost_read_length_sum(ahost_session* session, float running_sum, uint64_t first, uint64_t count) {
	const Batch& b = session->ingest.batch;
	if (first > b.n) first = b.n;
	if (count > b.n - first) count = b.n - first;
	for (uint64_t i = first; i < first + count; ++i) // sequential float accumulation in name order, hazard H4
		running_sum += ((size_t) b.seq_length[MATE1][i] + (size_t) b.seq_length[MATE2][i]) / 2;
	return running_sum;
}

int ahost_estimate_fragment_length(ahost_session* session, const int32_t* mate_gaps_in, uint32_t n_samples, uint64_t fragments_visited, unsigned int default_fragment_length,
                                   float* mate_gap_mean_out, float* mate_gap_stddev_out, float* read_length_mean_out, int32_t* max_mate_gap_out) {
	if (fragments_visited > session->ingest.batch.n) fragments_visited = session->ingest.batch.n;
	return ahost_estimate_fragment_length_from_sums(mate_gaps_in, n_samples, ahost_read_length_sum(session, 0, 0, fragments_visited), fragments_visited, default_fragment_length,
	                                                mate_gap_mean_out, mate_gap_stddev_out, read_length_mean_out, max_mate_gap_out);
}

int ahost_estimate_fragment_length_from_sums(const int32_t* mate_gaps_in, uint32_t n_samples, float read_length_sum, uint64_t fragments_visited, unsigned int default_fragment_length,
                                             float* mate_gap_mean_out, float* mate_gap_stddev_out, float* read_length_mean_out, int32_t* max_mate_gap_out) {
	float read_length_mean = read_length_sum;
	unsigned int read_length_count = (unsigned int) fragments_visited;
	unsigned int mate_gap_count = n_samples;
	if (mate_gap_count < 10000) {
		std::cerr << "WARNING: not enough chimeric reads to estimate mate gap distribution, using default values" << std::endl;
		*max_mate_gap_out = default_fragment_length;
		*read_length_mean_out = default_fragment_length;
		*mate_gap_mean_out = 0; *mate_gap_stddev_out = 0;
		return 0;
	}
	read_length_mean = read_length_mean / read_length_count;
	std::vector<int> mate_gaps(mate_gaps_in, mate_gaps_in + n_samples); // (the reference uses a std::list; a vector compacted in place keeps the same order and sums)
	float mate_gap_mean = 0, mate_gap_stddev = 0;
	bool no_more_outliers = false;
	while (true) {
		mate_gap_mean = 0;
		for (std::vector<int>::iterator i = mate_gaps.begin(); i != mate_gaps.end(); i++) mate_gap_mean += *i;
		mate_gap_mean /= mate_gap_count;
		mate_gap_stddev = 0;
		for (std::vector<int>::iterator i = mate_gaps.begin(); i != mate_gaps.end(); i++) mate_gap_stddev += (*i - mate_gap_mean) * (*i - mate_gap_mean);
		mate_gap_stddev = sqrt(1.0 / (mate_gap_count - 1) * mate_gap_stddev);
		unsigned int within_range = 0;
		for (std::vector<int>::iterator i = mate_gaps.begin(); i != mate_gaps.end(); ++i)
			if (*i > mate_gap_mean - mate_gap_stddev || *i < mate_gap_mean + mate_gap_stddev) // sic (hazard H6)
				within_range++;
		if (1.0 * within_range / mate_gap_count < 0.683 || no_more_outliers)
			break;
		no_more_outliers = true;
		size_t kept = 0;
		for (size_t i = 0; i < mate_gaps.size(); ++i) {
			if (mate_gaps[i] < mate_gap_mean - 3 * mate_gap_stddev || mate_gaps[i] > mate_gap_mean + 3 * mate_gap_stddev) {
				mate_gap_count--;
				no_more_outliers = false;
			} else {
				mate_gaps[kept++] = mate_gaps[i];
			}
		}
		mate_gaps.resize(kept);
	}
	*mate_gap_mean_out = mate_gap_mean; *mate_gap_stddev_out = mate_gap_stddev; *read_length_mean_out = read_length_mean;
	*max_mate_gap_out = std::max(0, (int) (mate_gap_mean + 3 * mate_gap_stddev));
	return 1;
}

} // extern "C"

// ---- iteration order of the reference's candidate container (hazard H2) ---------------------------------------------------

namespace {
// the reference's tuple hash (source/common.hpp:294-314): h(element k) ^ (hash of the remaining elements << 4), std::hash of an integer = its value
typedef std::tuple<unsigned int, unsigned int, unsigned short, unsigned short, int, int, bool, bool> CandidateKey;
struct CandidateKeyHash {
	size_t operator()(const CandidateKey& key) const {
		size_t h7 = (size_t) std::get<7>(key);
		size_t h6 = (size_t) std::get<6>(key) ^ h7 << 4;
		size_t h5 = (size_t) std::get<5>(key) ^ h6 << 4; // int -> size_t sign-extends, as std::hash<int> does
		size_t h4 = (size_t) std::get<4>(key) ^ h5 << 4;
		size_t h3 = (size_t) std::get<3>(key) ^ h4 << 4;
		size_t h2 = (size_t) std::get<2>(key) ^ h3 << 4;
		size_t h1 = (size_t) std::get<1>(key) ^ h2 << 4;
		return (size_t) std::get<0>(key) ^ h1 << 4;
	}
};
}

extern "C" int ahost_candidate_iteration_order(uint64_t n, const uint32_t* gene1, const uint32_t* gene2, const uint32_t* contigs, const int32_t* breakpoint1, const int32_t* breakpoint2, const uint32_t* flags, uint32_t* iteration_rank) {
	// The reference keeps its candidates in std::unordered_map<8-tuple, fusion_t> (source/common.hpp:286) and several stages depend on
	// the order in which that container iterates.  The order is a function of the insertion order (== candidate index here) and the
	// hash values only, so the very same container type, filled in the same order, reproduces it.
	if (!gene1 || !gene2 || !contigs || !breakpoint1 || !breakpoint2 || !flags || !iteration_rank) { g_error = "null argument"; return -1; }
	std::unordered_map<CandidateKey, uint32_t, CandidateKeyHash> container;
	for (uint64_t c = 0; c < n; ++c) {
		CandidateKey key((unsigned int) gene1[c], (unsigned int) gene2[c], (unsigned short) (contigs[c] >> 16), (unsigned short) (contigs[c] & 0xFFFF), breakpoint1[c], breakpoint2[c],
		                 (flags[c] & AGPU_CFLAG_UPSTREAM1) != 0, (flags[c] & AGPU_CFLAG_UPSTREAM2) != 0);
		if (!container.insert(std::make_pair(key, (uint32_t) c)).second) { g_error = "duplicate candidate key"; return -1; }
	}
	uint32_t rank = 0;
	for (auto entry = container.begin(); entry != container.end(); ++entry) iteration_rank[entry->second] = rank++;
	return 0;
}
