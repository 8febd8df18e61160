// arriba_amd/csrc/host/arriba_host.h -- host side of the MI355X-native fusion caller.
//
// The host driver reads the reference data (FASTA, GTF) and the STAR BAM once, restates the
// record classification of the reference's ingest (reference: source/read_chimeric_alignments.cpp)
// and packs everything into structure-of-arrays column buffers that are handed to the HIP
// kernels through the C ABI in include/arriba_gpu.h.  Nothing here does per-read filtering or
// candidate clustering -- that is the device's job.
#ifndef ARRIBA_HOST_H
#define ARRIBA_HOST_H 1

#include <cstdint>
#include "../../../include/arriba_host.h"
#include "../device/sam_core.hpp"
#include "../device/views.hpp"
#include <cstdio>
#include <functional>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

namespace arriba {

// The processors this process may actually use at once: the hardware threads it sees, less what its CPU affinity and the CPU quota of its container (cgroup cpu.max /
// cfs_quota_us) allow.  A host with 256 hardware threads behind a quota of 16 CPUs runs 128 busy threads for 12 ms of every 100 ms and stalls them for the rest
// (profiles/r03g_probe.txt): every pool of worker threads of the host library sizes itself by this number.
unsigned int cpu_budget();
void limit_threads_of_this_thread(unsigned int n); // (0: no limit)
// called by a thread that only reads a file or formats rows: nice 10 (ARRIBA_WORKER_NICE, 0 = as its parent).  In a session with two lanes a dozen of these run beside the one
// thread that launches the kernels of the stages and waits for their words; with all at one priority that thread took 1.10 s for stages it does in 0.75 s alone, with four
// readers instead of eight 0.96 s (profiles/r04q_*) -- it should not queue behind memcpy.
void worker_thread_starts();

typedef int32_t position_t;
typedef uint16_t contig_t;

// filter ids: the position in the reference's registry (source/common.hpp:29-67) is the id
enum : uint8_t {
	FILTER_none = 0, FILTER_duplicates, FILTER_inconsistently_clipped, FILTER_homopolymer, FILTER_read_through, FILTER_same_gene,
	FILTER_small_insert_size, FILTER_long_gap, FILTER_hairpin, FILTER_multimappers, FILTER_mismatches, FILTER_mismappers,
	FILTER_relative_support, FILTER_intronic, FILTER_non_coding_neighbors, FILTER_intragenic_exonic, FILTER_internal_tandem_duplication,
	FILTER_min_support, FILTER_known_fusions, FILTER_spliced, FILTER_blacklist, FILTER_end_to_end, FILTER_in_vitro, FILTER_merge_adjacent,
	FILTER_select_best, FILTER_marginal_read_through, FILTER_short_anchor, FILTER_no_coverage, FILTER_many_spliced, FILTER_no_genomic_support,
	FILTER_uninteresting_contigs, FILTER_viral_contigs, FILTER_top_expressed_viral_contigs, FILTER_low_coverage_viral_contigs,
	FILTER_genomic_support, FILTER_isoforms, FILTER_low_entropy, FILTER_homologs, FILTER_COUNT
};
extern const char* const FILTER_NAMES[FILTER_COUNT];

const int COVERAGE_RESOLUTION = 20;         // reference: source/read_stats.hpp:15
const int MAX_SPLICE_SITE_DISTANCE = 2;     // reference: source/annotation.hpp:14

// CIGAR encoding is BAM's: length << 4 | op
enum { CIGAR_M = 0, CIGAR_I = 1, CIGAR_D = 2, CIGAR_N = 3, CIGAR_S = 4, CIGAR_H = 5, CIGAR_P = 6, CIGAR_EQ = 7, CIGAR_X = 8 };
inline uint32_t cigar_op(uint32_t c) { return c & 15; }
inline uint32_t cigar_len(uint32_t c) { return c >> 4; }
inline uint32_t cigar_make(uint32_t length, uint32_t op) { return length << 4 | op; }
inline bool cigar_consumes_query(uint32_t op) { return (0x3C1A7 >> (op << 1)) & 1; }
inline bool cigar_consumes_reference(uint32_t op) { return (0x3C1A7 >> (op << 1)) & 2; }

std::string remove_chr(std::string contig);                                                  // reference: source/common.hpp:74-80
bool is_interesting_contig(std::string contig, const std::string& interesting_contigs);     // reference: source/common.hpp:82-110

// ---- reference data ---------------------------------------------------------------------------

struct Contigs {
	std::map<std::string, contig_t> by_name;   // ordered like the reference's contigs_t (source/common.hpp:72)
	std::vector<std::string> original_names;
	contig_t add(const std::string& original_name); // returns the id (existing or new)
	size_t size() const { return by_name.size(); }
};

struct Assembly {
	std::vector<std::string> sequence;          // per contig id; empty = not loaded (uninteresting)
	std::vector<std::string> file_names;        // the contigs of the file in its order, as it spells them, the uninteresting ones included (--realign-kept writes them as @SQ lines)
	std::vector<uint64_t> file_lengths;         // their bases
	bool has(contig_t contig) const { return contig < sequence.size() && !sequence[contig].empty(); }
};
// reference: source/assembly.cpp:28-58
void load_assembly(Assembly& assembly, const std::string& fasta_path, Contigs& contigs, const std::string& interesting_contigs);

struct GeneRecord {
	contig_t contig; position_t start, end; bool strand; // strand: true = forward
	std::string gene_id, name;
	int exonic_length;
	bool is_dummy, is_protein_coding;
};
struct ExonRecord {
	contig_t contig; position_t start, end; bool strand;
	int gene, transcript;
	int previous_exon, next_exon;               // exon ids, -1 = none
	position_t coding_region_start, coding_region_end;
};
struct TranscriptRecord {
	unsigned int id; std::string name;
	int first_exon, last_exon;
	unsigned int coding_length;
};
struct Annotation {
	std::vector<GeneRecord> genes;              // index == the reference's gene->id (list order, dummy genes appended last)
	std::vector<ExonRecord> exons;              // index == allocation order == canonical order inside exon sets (hazard H1)
	std::vector<TranscriptRecord> transcripts;
	std::unordered_map<std::string, int> gene_by_name;
	size_t real_genes = 0;                      // genes[0..real_genes) come from the GTF
};
// reference: source/annotation.cpp:161-377
// blacklist (keywords allowed in the second column) or known-fusions file -> rules; reference: source/filter_blacklisted_ranges.cpp:17-118, :244-264
void load_range_rules(const std::string& path, const Contigs& contigs, const Annotation& annotation, bool allow_keyword_in_second_column, std::vector<agpu_range_rule>& rules);
// tags (-t; reference: source/annotate_tags.cpp:11-44): lines of two items (no keywords) and a tag, looked up through 100 kb genome bins
struct TagRule { agpu_range_item first, second; std::string tag; };
struct Tags { std::vector<TagRule> rules; std::map<uint64_t, std::vector<uint32_t> > by_bin; bool empty() const { return by_bin.empty(); } };
void load_tags(const std::string& path, const Contigs& contigs, const Annotation& annotation, Tags& tags);
// protein domains (-p; reference: source/annotate_protein_domains.cpp:33-121): GFF3 records mapped to genes by id or name, indexed like the exons
struct ProteinDomain { contig_t contig; position_t start, end; bool strand; int gene; std::string name; };
void read_annotation_gtf(Annotation& annotation, const std::string& gtf_path, const std::string& gtf_features, Contigs& contigs, const Assembly& assembly);

// Flattened interval index (reference: source/annotation.t.hpp:25-45): per contig a sorted array of
// boundary keys (every feature.end and feature.start-1); bucket k lists the features that contain
// position keys[k], in ascending feature id.
struct FlatIndex {
	std::vector<uint32_t> contig_offset;        // [n_contigs+1] into keys
	std::vector<position_t> keys;
	std::vector<uint32_t> member_offset;        // [n_keys+1] into members
	std::vector<uint32_t> members;
	size_t n_contigs() const { return contig_offset.empty() ? 0 : contig_offset.size() - 1; }
	// first key >= position on the contig; returns the global key index or contig end
	uint32_t lower_bound(contig_t contig, position_t position) const;
	// (size_t, not contig_t: the index has as many slots as there are FEATURES -- the reference sizes it so, source/annotation.t.hpp:26 -- and a walk over all of them, as
	//  compute_exonic_length makes it, must not wrap at 65 536: with the 550 666 exons of a GENCODE-size annotation every real contig was visited nine times and every exonic length
	//  came out nine-fold -- found by the test on reference data of the size of hg38, round 6)
	uint32_t contig_begin(size_t contig) const { return contig_offset[contig]; }
	uint32_t contig_end(size_t contig) const { return contig_offset[contig + 1]; }
};
template <class Feature> void make_flat_index(const std::vector<Feature>& features, size_t n_contigs, FlatIndex& index);
// reference: source/arriba.cpp:166-184
void compute_exonic_length(Annotation& annotation, const FlatIndex& exon_index);

// structural variants from WGS (-d): Arriba's four-column format or VCF (BND, INV, DEL, DUP); reference: source/filter_genomic_support.cpp:15-165
void load_genomic_breakpoints(const std::string& path, const Contigs& contigs, std::vector<agpu_genomic_breakpoint>& variants);
void load_protein_domains(const std::string& path, const Contigs& contigs, const Annotation& annotation, std::vector<ProteinDomain>& domains, FlatIndex& index);

// host-side queries on the flat index (used by ingest and by host-only stages)
void get_annotation_by_coordinate(contig_t contig, position_t start, position_t end, std::vector<uint32_t>& result, const FlatIndex& index); // reference: source/annotation.t.hpp:55-101
bool is_breakpoint_spliced(int gene, bool direction_upstream, position_t breakpoint, const Annotation& annotation, const FlatIndex& exon_index); // reference: source/annotation.cpp:379-429
int get_spliced_distance(contig_t contig, position_t position1, position_t position2, int gene, const Annotation& annotation, const FlatIndex& exon_index); // reference: source/annotation.cpp:570-618

// ---- coverage -----------------------------------------------------------------------------------

struct Coverage { // reference: source/read_stats.hpp:17-27
	std::vector<std::vector<uint16_t> > coverage;
	std::vector<std::vector<uint8_t> > fragment_starts, fragment_ends;
	void resize(const Contigs& contigs, const Assembly& assembly);
	bool fragment_starts_here(contig_t contig, position_t start, position_t end) const;
	bool fragment_ends_here(contig_t contig, position_t start, position_t end) const;
	int get_coverage(contig_t contig, position_t position, bool direction_upstream) const;
};

// ---- packed batch -------------------------------------------------------------------------------

const unsigned MATE1 = 0, MATE2 = 1, SPLIT_READ = 1, SUPPLEMENTARY = 2;

// alignment bits (one byte per alignment slot)
enum : uint8_t { ABIT_STRAND = 1, ABIT_FIRST_IN_PAIR = 2, ABIT_SUPPLEMENTARY = 4, ABIT_EXONIC = 8, ABIT_PREDICTED_STRAND = 16, ABIT_PREDICTED_STRAND_AMBIGUOUS = 32 };
// fragment bits
enum : uint8_t { FBIT_SINGLE_END = 1, FBIT_MULTIMAPPER = 2, FBIT_DUPLICATE = 4 };

// Structure-of-arrays table of chimeric fragments in name order (index == name rank, hazard H3).
// Slot-major columns: column[slot][fragment].  Sequences are BAM 4-bit codes, two bases per byte,
// each sequence starting on a 4-byte boundary; only slots 0 and 1 carry a sequence.
struct Batch {
	size_t n = 0;
	std::vector<uint8_t> n_aln;                 // 2 = discordant mates, 3 = split read
	std::vector<uint8_t> fbits;
	std::vector<uint8_t> filter;
	std::vector<uint32_t> group;                // fragments sharing a read name (multimapper group) share a group id
	std::vector<contig_t> contig[3];
	std::vector<position_t> start[3], end[3];
	std::vector<uint8_t> abits[3];
	std::vector<uint32_t> cigar_offset[3];      // into cigar_pool
	std::vector<uint16_t> cigar_count[3];
	std::vector<uint32_t> cigar_pool;
	std::vector<uint32_t> seq_offset[2];        // in units of 4 bytes into seq_pool
	std::vector<uint32_t> seq_length[2];        // in bases
	std::vector<uint8_t> seq_pool;
	std::vector<uint32_t> name_offset;          // [n+1] into names ("QNAME,HI" as the reference keys its map)
	std::string names;
	std::string name(size_t i) const { return names.substr(name_offset[i], name_offset[i + 1] - name_offset[i]); }
	std::vector<uint32_t> cigar(unsigned slot, size_t i) const { return std::vector<uint32_t>(cigar_pool.begin() + cigar_offset[slot][i], cigar_pool.begin() + cigar_offset[slot][i] + cigar_count[slot][i]); }
	std::string sequence(unsigned slot, size_t i) const;
	void sequence_into(unsigned slot, size_t i, std::string& out) const; // the same into a string the caller keeps (no allocation once it has grown)
};

struct IngestOptions {
	std::string interesting_contigs = "1 2 3 4 5 6 7 8 9 10 11 12 13 14 15 16 17 18 19 20 21 22 X Y AC_* NC_*";
	std::string viral_contigs = "AC_* NC_*";
	bool external_duplicate_marking = false;
	unsigned int max_itd_length = 100;
};

struct IngestResult {
	Batch batch;
	Coverage coverage;
	uint64_t mapped_reads = 0;
	std::vector<uint64_t> mapped_viral_reads_by_contig;
	unsigned int malformed_count = 0, missing_hi_tag = 0;
	uint64_t records = 0;
	uint64_t separate_fragments = 0; unsigned int separate_malformed_count = 0; // -c: what pass C (the separate chimeric file) reported: its "(total=N)" and its WARNING
};
enum { INGEST_ROLE_WHOLE = 0, INGEST_ROLE_SEPARATE_CHIMERIC = 1, INGEST_ROLE_SEPARATE_RNA = 2 }; // what a file is to the loop of read_chimeric_alignments (its two booleans)

// Streaming source of uncompressed BAM bytes; returns the number of bytes delivered (0 = end of data).
struct ByteSource { virtual size_t read(uint8_t* buffer, size_t capacity) = 0; virtual ~ByteSource() {} };
ByteSource* open_bam_file(const std::string& path);               // BGZF/gzip or raw BAM, file or /dev/stdin
ByteSource* open_memory_source(const uint8_t* data, size_t size); // raw (already inflated) BAM stream

// SAM text: the header lines, the @SQ names as sam_core.hpp looks them up, and the lines stepped on the host (ingest.cpp)
struct SamHeader {
	std::vector<std::string> names; std::vector<uint32_t> lengths; bool sorted_by_coordinate = false; uint64_t bytes = 0, lines = 0;
	bool scan(const uint8_t* text, size_t size, bool at_end);
	void bam_header(const uint8_t* text, std::vector<uint8_t>& out) const;
};
struct SamTargetTable {
	std::string names; std::vector<uint32_t> offsets, table;
	void build(const char* all_names, const uint32_t* name_offset, uint32_t n);
	void build(const std::vector<std::string>& list);
	agpu::SamTargets view() const;
};
bool head_is_sam_text(const uint8_t* head, size_t size);
void sam_transcode_lines(const uint8_t* text, size_t size, const agpu::SamTargets& targets, uint64_t first_line_number, std::vector<uint8_t>& out, uint64_t& n_records, uint64_t& n_lines, uint64_t& bad_line, uint32_t& bad_reason);
std::string sam_line_error(uint64_t line, uint32_t reason);
ByteSource* text_or_bam_source(ByteSource* inner); // takes `inner`; BAM bytes pass through, SAM text comes out as the BAM stream of the same alignments

// The file side of the device ingest (agpu_ingest_*): container recognised from the one open stream, BAM header parsed, bytes handed on in pieces.
class BamFeed;
BamFeed* open_bam_feed(const std::string& path);
void close_bam_feed(BamFeed* feed);
uint64_t bam_feed_header(BamFeed* feed, std::vector<std::string>& target_names); // returns the size of the header = offset of the first record in the uncompressed stream
uint64_t bam_feed_take_part(BamFeed* feed, uint32_t part, uint32_t parts);            // the feed delivers only part `part` of `parts` of the records from now on; returns the offset of its first record in the stream
uint64_t bam_feed_size_hint(BamFeed* feed);                                       // expected size of the uncompressed stream, 0 = unknown
const SamTargetTable* bam_feed_sam_targets(BamFeed* feed);                        // the @SQ names when the file is SAM text (its pieces are of kind 3), NULL for BAM
bool bam_feed_next(BamFeed* feed, uint8_t* buffer, size_t capacity, agpu_bgzf_block* blocks, uint32_t block_capacity, ahost_bam_piece& piece);

// --sorted-bam on the host (sorted_bam.cpp): the header of the output from the head of the input (a BAM header, or the '@' lines of SAM text), stored BGZF blocks, the records in
// coordinate order with the arrays of the index (arriba_amd/csrc/device/sorted_bam_core.hpp stepped on the host), FILE.bai from those arrays, and the two files written
struct SortedBam {
	std::vector<uint8_t> blocks; // the record blocks
	agpu_sorted_bam_info info;
	bool indexed = false;
	std::vector<uint64_t> chunk_key, chunk_begin, chunk_end, interval_offset, intervals, ref_begin, ref_end, ref_mapped, ref_unmapped;
	uint64_t n_no_coor = 0;
	agpu_sorted_bam_index_arrays view(uint32_t n_ref);
};
void sorted_bam_header(const uint8_t* input, size_t size, std::vector<uint8_t>& out, std::vector<uint32_t>& ref_length);
void sorted_bam_frame(const uint8_t* bytes, uint64_t size, std::vector<uint8_t>& out);
bool references_fit_bai(const uint32_t* ref_length, uint32_t n_ref);
void sorted_bam_of(const uint8_t* records, uint64_t size, uint64_t first_block_file_offset, const uint32_t* ref_length /* NULL: no index */, uint32_t n_ref, SortedBam& result, int level = 0, const uint8_t* duplicate = NULL); // level: 0 stored blocks, 1 deflate_out_core.hpp stepped on the host; duplicate: --mark-duplicates, one byte per record
struct SortedBamIndexed { int32_t ref, pos, end; bool unmapped; uint64_t begin_offset, end_offset; }; // a record of a file for its index: coordinates, and the virtual offsets of its first byte and behind its last
void sorted_bam_index_of(uint64_t n, const std::function<SortedBamIndexed(uint64_t)>& record, const uint32_t* ref_length, uint32_t n_ref, SortedBam& result);
void sorted_bam_bai(const agpu_sorted_bam_index_arrays& index, std::vector<uint8_t>& out);
void write_file(const std::string& path, const std::vector<const std::vector<uint8_t>*>& parts);
void sorted_bam_write(const uint8_t* input_header, size_t header_size, const uint8_t* records, uint64_t size, const std::string& path, agpu_sorted_bam_info* info, int level = 0, bool mark_duplicates = false, agpu_markdup_counts* counts = NULL);
// --mark-duplicates on the host (markdup.cpp): arriba_amd/csrc/device/markdup_core.hpp stepped over records in host memory; flag[r]: MDUP_FLAG_MASK if record r leaves with 0x400
void markdup_flags(const uint8_t* records, uint64_t size, std::vector<uint8_t>& flag, agpu_markdup_counts& counts);
// --supporting-alignments on the host (supporting.cpp): the writer that cuts the framed record blocks of all rows -- one row's behind the other's, from the device or from the
// stepping -- into PREFIX_ID.bam and makes PREFIX_ID.bam.bai from the arrays of their records; everything goes through *.tmp, and unless `commit` ran nothing of the prefix is
// left behind.  supporting_alignments: arriba_amd/csrc/device/supporting_core.hpp stepped on the host over records in host memory.
class SupportingWriter {
public:
	SupportingWriter(const std::string& prefix, const uint8_t* framed_header, uint64_t framed_bytes, uint32_t n_rows, const uint64_t* row_file_bytes);
	~SupportingWriter();
	void push(const uint8_t* bytes, uint64_t size);
	void index(const agpu_supporting_index_arrays& arrays, const uint32_t* ref_length, uint32_t n_ref);
	void commit();
	void abandon();
private:
	std::string path_of(uint32_t row) const;
	void open_row(); void close_row(); void skip_finished_rows();
	std::string prefix_; std::vector<uint8_t> header_; std::vector<uint64_t> row_bytes_; size_t row_; uint64_t written_; FILE* file_; bool indexed_;
	std::vector<std::string> temporaries_, finals_;
};
void supporting_alignments(const uint8_t* input_header, size_t header_size, const uint8_t* records, uint64_t size, const char* names, const uint64_t* name_offset, uint64_t n_names, bool strip_hit_index,
                           const agpu_supporting_rows& rows, int64_t window, const std::string& prefix, agpu_supporting_info* info);
// --virus-expression on the host (virus.cpp): the viral contigs of a header (a BAM header, or the '@' lines of SAM text) by the patterns of -v, arriba_amd/csrc/device/virus_core.hpp
// stepped over records in host memory, and what turns the counters -- the host's or the device's -- into the text of the reference's scripts/quantify_virus_expression.sh
struct VirusContigs { uint32_t n_ref = 0; std::vector<int32_t> ref; std::vector<uint32_t> length; std::vector<std::string> name; std::string names; std::vector<uint32_t> name_offset; ahost_virus_contigs view(); };
struct VirusCounters { uint64_t total = 0, candidates = 0, kmer_keys = 0; std::vector<uint64_t> reads, covered, kmer_count, shared; std::vector<uint32_t> active; agpu_virus_counters view() const; };
void virus_contigs_of(const uint8_t* input, size_t size, const std::string& viral_contigs, VirusContigs& contigs);
void virus_expression(const uint8_t* records, uint64_t size, const int32_t* viral_ref, const uint32_t* viral_length, uint32_t n_viruses, uint32_t n_ref, VirusCounters& counters);
std::string virus_expression_table(const agpu_virus_counters& counters, const ahost_virus_contigs& contigs);
void virus_expression_write(const std::string& text, const std::string& path); // through path + ".tmp"; on a failure nothing is left behind
void header_contigs(const uint8_t* input, size_t size, std::vector<std::string>& names, std::vector<uint32_t>& lengths); // the references of a BAM header, or of the '@' lines of SAM text, in their order
// --coverage on the host (depth.cpp): the contigs of a header, arriba_amd/csrc/device/depth_core.hpp stepped over records in host memory -- the comparator of agpu_depth.hip, and
// what --host-ingest and the CPU tier run --: the bedGraph text and the statistics of the device
struct DepthContigs { std::vector<uint32_t> length; std::string names; std::vector<uint32_t> name_offset; ahost_depth_contigs view() const; };
void depth_contigs_of(const uint8_t* input, size_t size, DepthContigs& contigs);
void depth_track(const uint8_t* records, uint64_t size, const ahost_depth_contigs& contigs, std::string& text, agpu_depth_stats& stats);
std::string depth_line_text(const std::string& name, uint32_t start, uint32_t end, uint32_t depth);
// --gene-counts on the host (gene_counts.cpp): arriba_amd/csrc/device/genecount_core.hpp stepped over records in host memory against the exon index, exon_gene and gene_bits of a
// session (view: pointers into the session) -- the comparator of agpu_genecount.hip, and what --host-ingest and the CPU tier run; and the text of the file
struct GeneCountAnnotation { agpu::AnnotationView view; };
void gene_counts_of(const GeneCountAnnotation& annotation, const std::vector<uint32_t>& tid_to_contig, const std::vector<uint32_t>& ref_length, const uint8_t* records, uint64_t size, std::vector<uint64_t>& counts,
                    agpu_gene_count_stats& stats); // counts: [3][n_genes + 4]
std::string gene_counts_text(const std::vector<std::string>& gene_ids, const uint64_t* counts);
// --splice-junctions on the host (splice_junctions.cpp): arriba_amd/csrc/device/junction_core.hpp stepped over records in host memory against the exon chains, gene_contig and
// gene_bits and the assembly of a session (view, genome: pointers into the session) -- the comparator of agpu_junctions.hip, and what --host-ingest and the CPU tier run; and the
// text of the file from a row table, the host's or the device's
struct JunctionReferences { agpu::AnnotationView view; agpu::GenomeView genome; };
void splice_junctions_of(const JunctionReferences& references, const std::vector<uint32_t>& tid_to_contig, const std::vector<uint32_t>& ref_length, const uint8_t* records, uint64_t size, std::vector<agpu_junction_row>& rows,
                         agpu_junction_stats& stats);
std::string splice_junctions_text(const ahost_depth_contigs& contigs, const agpu_junction_row* rows, uint64_t n_rows);
// --allele-counts on the host (allele_counts.cpp): the lines of a sites file (contig as spelled, 0-based position, the reference of a header it is placed on),
// arriba_amd/csrc/device/allele_core.hpp stepped over records in host memory with REF from the assembly of a session (genome: pointers into the session) -- the comparator of
// agpu_alleles.hip, and what --host-ingest and the CPU tier run; and the text of the file from a row table, the host's or the device's
struct AlleleSiteList {
	std::vector<agpu_allele_site> sites; std::string names; std::vector<uint64_t> name_offset; uint64_t placed = 0;
	void place(const uint8_t* header, size_t header_size); // every line on the references of a BAM header or of the '@' lines of SAM text (none: every line unplaced)
};
void allele_sites_parse(const std::string& path, AlleleSiteList& list); // refusals name the line
void allele_counts_of(const agpu::GenomeView& genome, const std::vector<uint32_t>& tid_to_contig, const std::vector<uint32_t>& ref_length, const agpu_allele_site* sites, uint64_t n_sites, const uint8_t* records, uint64_t size,
                      uint32_t min_mapq, uint32_t min_baseq, std::vector<agpu_allele_row>& rows, agpu_allele_stats& stats);
std::string allele_counts_text(const AlleleSiteList& list, const agpu_allele_row* rows, uint64_t n_rows);
// --variant-sites on the host (variant_sites.cpp): arriba_amd/csrc/device/variant_core.hpp and allele_core.hpp stepped over records in host memory with REF from the assembly of a
// session (genome: pointers into the session) -- the comparator of agpu_variants.hip, and what --host-ingest and the CPU tier run; and the text of the file from a row table, the
// host's or the device's
void variant_sites_of(const agpu::GenomeView& genome, const std::vector<uint32_t>& tid_to_contig, const std::vector<uint32_t>& ref_length, const uint8_t* records, uint64_t size, uint32_t min_mapq, uint32_t min_baseq,
                      uint32_t min_alt, uint32_t min_percent, std::vector<agpu_variant_row>& rows, agpu_variant_stats& stats);
std::string variant_sites_text(const ahost_depth_contigs& contigs, const agpu_variant_row* rows, uint64_t n_rows);
// --indel-sites on the host (indel_sites.cpp): arriba_amd/csrc/device/indel_core.hpp and allele_core.hpp stepped over records in host memory, normalised against the assembly of a
// session (genome: pointers into the session) -- the comparator of agpu_indels.hip, and what --host-ingest and the CPU tier run; and the text of the file from a row table, the
// host's or the device's (the deleted bases are read from the assembly: tid_to_contig says where the references of the header lie in it)
void indel_sites_of(const agpu::GenomeView& genome, const std::vector<uint32_t>& tid_to_contig, const std::vector<uint32_t>& ref_length, const uint8_t* records, uint64_t size, uint32_t min_mapq, uint32_t min_alt,
                    uint32_t min_percent, std::vector<agpu_indel_row>& rows, agpu_indel_stats& stats);
std::string indel_sites_text(const agpu::GenomeView& genome, const std::vector<uint32_t>& tid_to_contig, const ahost_depth_contigs& contigs, const agpu_indel_row* rows, uint64_t n_rows);
// --realign-reads on the host (realign_split.cpp): which references of a header are contigs of the assembly and the header of the file of the kept templates; and
// arriba_amd/csrc/device/realign_core.hpp stepped over records in host memory -- the comparator of agpu_realign.hip, and what --host-ingest and the CPU tier run.  kept: the lines
// without the header (empty unless want_kept)
struct RealignPlan { std::vector<uint8_t> in_assembly; std::string header; };
void realign_plan_of(const Assembly& assembly, const uint8_t* header, size_t size, RealignPlan& plan);
void realign_split_of(const uint8_t* in_assembly, const ahost_depth_contigs& contigs, const uint8_t* records, uint64_t size, bool want_kept, std::string& realign, std::string& kept, agpu_realign_stats& stats);
// --rna-metrics on the host (region_track.cpp, rna_metrics.cpp): the lines of an rRNA interval file (BED); the region track of an annotation and those intervals -- runs of bases
// with equal bits and body gene per contig (include/arriba_gpu.h: agpu_region_track) --; arriba_amd/csrc/device/rnametrics_core.hpp stepped over records in host memory against a
// track -- the comparator of agpu_rnametrics.hip, and what --host-ingest and the CPU tier run; and the text of the file from a counter block, the host's or the device's
struct RrnaInterval { std::string contig; int64_t start, end; }; // 0-based, half open, the contig as the file spells it
void rrna_intervals_parse(const std::string& path, std::vector<RrnaInterval>& intervals); // refusals name the line
struct RegionTrack {
	uint64_t id = 0;
	std::vector<uint32_t> contig_offset; std::vector<int32_t> run_start; std::vector<uint8_t> run_bits; std::vector<uint32_t> run_gene, run_rank, gene_body;
	uint64_t intervals = 0, intervals_unknown_contig = 0;
	agpu_region_track view() const;
};
void region_track_build(const Annotation& annotation, const Contigs& contigs, size_t n_contigs, const std::vector<RrnaInterval>& intervals, RegionTrack& track);
void rna_metrics_of(const agpu_region_track& track, const std::vector<uint32_t>& tid_to_contig, const std::vector<uint32_t>& ref_length, const uint8_t* records, uint64_t size, std::vector<uint64_t>& counters,
                    agpu_rna_metrics_stats& stats); // counters: [AGPU_RNA_METRICS_WORDS]
std::string rna_metrics_text(const uint64_t* counters);
const std::vector<uint8_t>& bam_feed_header_bytes(BamFeed* feed); // the head of the uncompressed input as the feed read it: the BAM header, or the '@' lines of SAM text

// reference: source/read_chimeric_alignments.cpp:560-773 with separate_chimeric_bam_file=false, is_rna_bam_file=true
// gene_index must be the index over the GTF genes (before dummy genes are added).
void read_chimeric_alignments(ByteSource& source, const Assembly& assembly, Contigs& contigs, const Annotation& annotation, const FlatIndex& gene_index, const IngestOptions& options, IngestResult& result);
// -c: the same with separate_chimeric_bam_file=true, twice over one table of fragments (source/arriba.cpp:123-130): is_rna_bam_file=false over `chimeric_source`, true over `rna_source`
void read_chimeric_alignments_separate(ByteSource& chimeric_source, ByteSource& rna_source, const Assembly& assembly, Contigs& contigs, const Annotation& annotation, const FlatIndex& gene_index, const IngestOptions& options, IngestResult& result);

}

#endif
