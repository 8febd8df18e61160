/*
 * include/arriba_host.h -- C ABI of the host driver library (libarriba_host.so).
 *
 * The host side reads the reference data and the BAM once and produces the structure-of-arrays views
 * of include/arriba_gpu.h; it also holds the few inherently sequential scalar stages of the path
 * (strandedness vote, fragment-length estimate, per-contig viral verdicts) that the reference
 * computes between its per-read stages.  No per-read filtering or clustering happens here.
 * Each entry point cites the reference code it restates.
 */
#ifndef ARRIBA_HOST_C_H
#define ARRIBA_HOST_C_H 1

#include "arriba_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ahost_session ahost_session;

const char* ahost_last_error(void);

/* load_assembly + read_annotation_gtf + make_annotation_index (source/arriba.cpp:91-113).
 * NULL strings select the reference defaults (source/options.cpp:74-75, source/annotation.hpp:23). */
ahost_session* ahost_open(const char* fasta_path, const char* gtf_path, const char* interesting_contigs, const char* viral_contigs, const char* gtf_features);
void ahost_close(ahost_session* session);

/* read_chimeric_alignments for -x (source/read_chimeric_alignments.cpp:560-773); data = raw (inflated) BAM stream, or SAM text (told by content, as sam_open does) */
int ahost_ingest_bam_file(ahost_session* session, const char* bam_path, int external_duplicate_marking, unsigned int max_itd_length);
int ahost_ingest_bam_memory(ahost_session* session, const uint8_t* data, size_t size, int external_duplicate_marking, unsigned int max_itd_length);
/* -c: the chimeric alignments of STAR --chimOutType SeparateSAMold come in a file of their own: read_chimeric_alignments twice over one table of fragments, as source/arriba.cpp:123-130
 * calls it -- `chimeric_path` with (separate_chimeric_bam_file, !is_rna_bam_file), then `rna_path` with both true.  Both take what ahost_ingest_bam_file takes.  The two WARNING lines
 * of the reference go to stderr; chimeric_fragments / chimeric_malformed (may be NULL): the "(total=N)" and the WARNING count of the first call.  The batch view then holds the union
 * as the second call leaves it.  Fails if the two headers do not list the same reference names in the same order, or if a record of `chimeric_path` has no reference. */
int ahost_ingest_separate(ahost_session* session, const char* chimeric_path, const char* rna_path, int external_duplicate_marking, unsigned int max_itd_length, uint64_t* chimeric_fragments, uint64_t* chimeric_malformed);
/* The result of an ingest (batch, counters, coverage) as a file, and back into a session opened on the same assembly and annotation: repeated
 * benchmark and profiling runs over one batch skip the parse.  Tooling; not a step of the reference. */
int ahost_save_ingest(ahost_session* session, const char* path);
int ahost_load_ingest(ahost_session* session, const char* path);

/* ---- read_chimeric_alignments on the device (agpu_ingest_*, include/arriba_gpu.h): the host side --------------------------------------------------
 * The host opens the file (BGZF, gzip or raw BAM; a path, a pipe, /dev/stdin or "-": sam_open, source/read_chimeric_alignments.cpp:563), parses the BAM
 * header -- the contigs of the run must be known before the records are classified (:566-582) -- and hands the bytes on in pieces.
 *   ahost_bam_open     opens and parses the header; fills `config` for agpu_ingest_begin (its pointers stay valid until ahost_bam_close).  The genome
 *                      view of the session then holds the contigs of the header, too: upload it (again) before agpu_ingest_begin.
 *   ahost_bam_next     the next piece into `buffer` (>= 1 MiB; pinned memory from agpu_host_alloc): stored_bgzf = 1: raw BGZF bytes whose blocks are
 *                      all stored, with the table of the blocks -> agpu_ingest_push_bgzf; 0: bytes of the uncompressed stream (deflated blocks inflated
 *                      by all cores, CRC-checked) -> agpu_ingest_push.  Returns 1, 0 at the end of the file, -1 on error.
 *                      SAM text (the format is told by the content of the uncompressed head, never by the name of the file; plain, gzip or BGZF, inflated here):
 *                      the header lines are read here -- @SQ SN/LN are the targets, @HD SO:coordinate the sort order -- config->first_record_offset is 0 and the pieces are
 *                      of kind 3: whole lines only, first_line counting the header lines in -> agpu_ingest_push_sam, after ONE agpu_ingest_sam_targets with what
 *                      ahost_bam_sam_targets returns.  ahost_bam_open_part refuses SAM text: text has no record sizes to find a record start by in the middle of the file.
 *   ahost_adopt_device_ingest   what the device found: the reference's checks and warnings behind its loop (:759-771: "no normal reads found", malformed
 *                      records, no chimeric reads, missing HI tags), the counters, and coverage_t (flat arrays in the order of config.coverage_window_offset)
 *   ahost_set_batch_rows   the rows of the batch the host itself works on (the output writer: names, CIGARs and sequences of the supporting reads), fetched
 *                      with agpu_gather_rows_*; fragment indices in an ahost_fusion_table then refer to these rows */
typedef struct { int stored_bgzf; /* the KIND of the piece (the name is from when there were two). 0: the buffer holds bytes of the stream; 1: raw BGZF bytes whose blocks are stored, with their table; 2: raw BGZF bytes whose blocks are deflated, with their table (both: agpu_ingest_push_bgzf); 3: whole lines of SAM text (agpu_ingest_push_sam; stream_bytes is 0: the size of their records is known on the device only) */ size_t bytes; size_t stream_bytes; uint32_t n_blocks; uint64_t first_line; /* kind 3: the 1-based number, in the file, of the first line of the piece */ } ahost_bam_piece;
/* The processors this process may use at once (affinity, CPU quota of the cgroup), and a limit for every decision about a number of threads that is made on the calling thread
 * from now on (0: none): a session that feeds the next sample beside the stages of the current one and writes the last file beside both gives each of the three its share --
 * more busy threads than the quota has CPUs are all stopped together for the rest of the scheduler's period. */
unsigned int ahost_cpu_budget(void);
void ahost_limit_threads_of_this_thread(unsigned int n);
int ahost_bam_open(ahost_session* session, const char* bam_path, int external_duplicate_marking, unsigned int max_itd_length, agpu_ingest_config* config);
/* -c on the device: as ahost_bam_open, with config->role set (include/arriba_gpu.h: AGPU_ROLE_*).  The file opened with AGPU_ROLE_SEPARATE_CHIMERIC leaves its reference names
 * with the session; the one opened with AGPU_ROLE_SEPARATE_RNA behind it must list the same names in the same order. */
int ahost_bam_open_role(ahost_session* session, const char* bam_path, int external_duplicate_marking, unsigned int max_itd_length, int role, agpu_ingest_config* config);
/* One sample over several GPUs: as ahost_bam_open, but the pieces that follow hold only part `part` of `parts` of the records -- the file (BGZF or
 * uncompressed BAM on disk; the alignments of a read name next to each other, as STAR writes them) is cut between read names near the byte offsets
 * size * k / parts, at places every rank finds by itself from the bytes of the file.  config->part_of_sample is set: agpu_shard_export / agpu_shard_merge
 * (include/arriba_gpu.h) put the parts together, and ahost_adopt_device_ingest then takes the result of the merge. */
int ahost_bam_open_part(ahost_session* session, const char* bam_path, int external_duplicate_marking, unsigned int max_itd_length, unsigned int part, unsigned int parts, agpu_ingest_config* config);
int ahost_bam_next(ahost_session* session, void* buffer, size_t capacity, agpu_bgzf_block* blocks, uint32_t block_capacity, ahost_bam_piece* piece);
void ahost_bam_close(ahost_session* session);
/* 1: the file ahost_bam_open opened is SAM text -- names / name_offset [n_targets + 1] / n_targets are the @SQ names in tid order as agpu_ingest_sam_targets takes them (valid until
 * ahost_bam_close); 0: it is BAM; -1: no file is open */
int ahost_bam_sam_targets(ahost_session* session, const char** names, const uint32_t** name_offset, uint32_t* n_targets);
/* Alignment lines of SAM text -> the BAM records `samtools view -b` writes for them (SAMv1 section 4.2), by arriba_amd/csrc/device/sam_core.hpp stepped on the host: the comparator of
 * agpu_sam_transcode, and what the host ingest (ahost_ingest_bam_file / _memory, which take SAM text like BAM) runs.  text: whole lines, the last may lack its "\n"; '@' lines in front
 * of the first alignment are skipped and counted.  names / name_offset [n_targets + 1]: the @SQ names in tid order.  Returns 0, or -1 with *bad_line = the 1-based number of the first
 * malformed line (its record is left out; the others are still written) or when `out` is too small (*out_bytes then says how much is needed). */
int ahost_sam_transcode(const void* text, size_t size, const char* names, const uint32_t* name_offset, uint32_t n_targets, void* out, size_t capacity, uint64_t* out_bytes, uint64_t* n_records, uint64_t* bad_line);
/* ---- --sorted-bam: the host side of agpu_sorted_bam_* (include/arriba_gpu.h) -- the records of -x in coordinate order as a BAM file of stored BGZF blocks, and its BAI index ----
 *   ahost_sorted_bam_header     the header of the output, already in BGZF blocks of its own (the record blocks begin at *framed_bytes of the file): the header of the file the last
 *                               ahost_bam_open opened, with "@HD ... SO:coordinate" -- an SO: already there is replaced, a header without @HD gets "@HD\tVN:1.6\tSO:coordinate" in
 *                               front, every other line and the references stay.  SAM text: the BAM header is built from the '@' lines (l_text, the text, n_ref, SN / LN of every
 *                               @SQ); an @SQ without LN is an error that names the line.  ref_length [n_ref]: for agpu_sorted_bam_index.  Valid until the next call on the session.
 *   ahost_sorted_bam_header_of  the same from the head of an uncompressed input in memory (a BAM header, or the '@' lines of SAM text); valid until the next call on the thread
 *   ahost_sorted_bam            arriba_amd/csrc/device/sorted_bam_core.hpp stepped on the host over BAM records in host memory: key, std::stable_sort, offsets, framing, index -- the same
 *                               record blocks and the same index arrays as the device gives (its comparator; what --host-ingest and the CPU tier run).  index == NULL: no index.
 *                               *blocks and the arrays of *index stay valid until the next call on the thread.
 *   ahost_sorted_bam_write_index   FILE.bai (SAMv1 5.2) from the arrays
 *   ahost_sorted_bam_eof        the 28 bytes that end a BGZF file
 *   ahost_sorted_bam_write      all of it: path and path + ".bai" written through path + ".tmp" / ".bai.tmp" and renamed; a reference longer than 2^29 bases: the BAM file without
 *                               an index, and a warning on stderr */
int ahost_sorted_bam_header(ahost_session* session, const uint8_t** framed, uint64_t* framed_bytes, const uint32_t** ref_length, uint32_t* n_ref);
int ahost_sorted_bam_header_of(const void* input_header, size_t size, const uint8_t** framed, uint64_t* framed_bytes, const uint32_t** ref_length, uint32_t* n_ref);
int ahost_sorted_bam(const void* records, size_t size, uint64_t first_block_file_offset, const uint32_t* ref_length, uint32_t n_ref, const uint8_t** blocks, agpu_sorted_bam_info* info, agpu_sorted_bam_index_arrays* index);
int ahost_sorted_bam_write_index(const agpu_sorted_bam_index_arrays* index, const char* path);
void ahost_sorted_bam_eof(uint8_t* block /* [28] */);
 /*  ahost_sorted_bam_file       the same for a file (BAM in BGZF, gzip or raw; SAM text): read whole into host memory -- what --host-ingest does for --sorted-bam */
int ahost_sorted_bam_file(const char* input_path, const char* path, agpu_sorted_bam_info* info /* may be NULL */);
int ahost_sorted_bam_write(const void* input_header, size_t header_size, const void* records, size_t size, const char* path, agpu_sorted_bam_info* info /* may be NULL */);
/* --sorted-bam-compression: the same three with a level.  0: the stored blocks of the functions above, byte for byte.  1: every record block is one deflate block, the smallest of
 * stored / fixed Huffman / dynamic Huffman over LZ77 tokens (arriba_amd/csrc/device/deflate_out_core.hpp stepped on the host: the bytes agpu_sorted_bam_* give at level 1); the
 * virtual offsets of the index come from the sizes the blocks really have; info->file_bytes is the size the record blocks really have.  The header blocks and the end-of-file block
 * are the same at every level.  Another level: an error with a message. */
int ahost_sorted_bam_level(const void* records, size_t size, uint64_t first_block_file_offset, const uint32_t* ref_length, uint32_t n_ref, int level, const uint8_t** blocks, agpu_sorted_bam_info* info, agpu_sorted_bam_index_arrays* index);
int ahost_sorted_bam_file_level(const char* input_path, const char* path, int level, agpu_sorted_bam_info* info /* may be NULL */);
int ahost_sorted_bam_write_level(const void* input_header, size_t header_size, const void* records, size_t size, const char* path, int level, agpu_sorted_bam_info* info /* may be NULL */);
/* --mark-duplicates: arriba_amd/csrc/device/markdup_core.hpp stepped sequentially on the host (the rule: DESIGN.md 4.14) -- the comparator of agpu_markdup.hip, what --host-ingest runs.
 *   ahost_markdup                        flag[r], r < n_records (the records the stream holds, else an error): 0x04 -- the mask of 0x400 in byte 19 of a record -- if record r
 *                                        belongs to a duplicate template, else 0; counts (may be NULL): as agpu_markdup_stats reports them
 *   ahost_sorted_bam_file_marked         ahost_sorted_bam_file_level; with mark_duplicates != 0 every record is copied with bit 0x400 set or cleared by those bytes -- the file that
 *                                        agpu_sorted_bam_* writes behind agpu_sorted_bam_set_mark_duplicates.  ahost_sorted_bam_file_level keeps its behaviour.
 *   ahost_sorted_bam_file_marked_counts  the same, and the counts */
int ahost_markdup(const void* records, size_t size, uint8_t* flag, uint64_t n_records, agpu_markdup_counts* counts /* may be NULL */);
int ahost_sorted_bam_file_marked(const char* input_path, const char* path, int level, int mark_duplicates, agpu_sorted_bam_info* info /* may be NULL */);
int ahost_sorted_bam_file_marked_counts(const char* input_path, const char* path, int level, int mark_duplicates, agpu_sorted_bam_info* info /* may be NULL */, agpu_markdup_counts* counts /* may be NULL */);
/* ---- --supporting-alignments: the host side of agpu_support_pool_build / agpu_supporting_* (include/arriba_gpu.h) -- one sorted, indexed BAM file per row of fusions.tsv with
 * the alignments of the row's read_identifiers near its breakpoints (the reference's scripts/extract_fusion-supporting_alignments.sh), PREFIX_ID.bam and PREFIX_ID.bam.bai, ID = 1-based
 * rank of the row ----
 *   ahost_written_fusion_rows        the data rows of the fusions file (-o, not -O) the session wrote last, in their order: the candidate of the table each was made from, and per
 *                                    row two (refID of the BAM header, 0-based breakpoint) pairs as columns 5 and 6 print them (-1: a contig the BAM header does not have).  The
 *                                    supporting fragments of row r are entries list_offset[3 c] .. list_offset[3 c + 3] of read_lists of that table, c = candidate[r].
 *                                    Valid until the next call on the session.
 *   ahost_supporting_writer_*        cuts the framed record blocks of all rows (agpu_supporting_next) into the files, each with the header of --sorted-bam (ahost_sorted_bam_header)
 *                                    and the end-of-file block; _index makes the BAI files from the arrays of agpu_supporting_index (a reference longer than 2^29 bases: none, and the
 *                                    warning of --sorted-bam); _close(commit = 1) renames the *.tmp files; _close(0), or any failure: nothing of the prefix is left behind
 *   ahost_supporting_alignments      arriba_amd/csrc/device/supporting_core.hpp stepped on the host over BAM records in host memory, with an explicit list of names: the same files
 *                                    as the device gives (its comparator; the CPU tier)
 *   ahost_supporting_alignments_file the same for a file and the rows ahost_written_fusion_rows gives, with the names of the batch of a host ingest: what --host-ingest runs */
typedef struct ahost_supporting_writer ahost_supporting_writer;
int ahost_written_fusion_rows(ahost_session* session, uint32_t* n_rows, const uint32_t** candidate, const int32_t** ref /* [2 * n_rows] */, const int32_t** breakpoint /* [2 * n_rows] */);
ahost_supporting_writer* ahost_supporting_writer_open(const char* prefix, const void* framed_header, uint64_t framed_bytes, uint32_t n_rows, const uint64_t* row_file_bytes);
int ahost_supporting_writer_push(ahost_supporting_writer* writer, const void* bytes, uint64_t size);
int ahost_supporting_writer_index(ahost_supporting_writer* writer, const agpu_supporting_index_arrays* index, const uint32_t* ref_length, uint32_t n_ref);
int ahost_supporting_writer_close(ahost_supporting_writer* writer, int commit);
int ahost_supporting_alignments(const void* input_header, size_t header_size, const void* records, size_t size, const char* names, const uint64_t* name_offset, uint64_t n_names,
                                const agpu_supporting_rows* rows, int64_t window, const char* prefix, agpu_supporting_info* info /* may be NULL */);
/* ---- --virus-expression: the host side of agpu_virus_expression (include/arriba_gpu.h) -- the table of the reference's scripts/quantify_virus_expression.sh with its default
 * parameters (the rule: DESIGN.md 4.11) ----
 *   ahost_virus_contigs_of_session  the viral contigs of the header of the file the last ahost_bam_open opened, by the patterns of -v of the session: slot v is viral_ref[v]
 *   ahost_virus_contigs_of       the same from the head of an uncompressed input in memory (a BAM header, or the '@' lines of SAM text); viral_contigs NULL: "AC_* NC_*".
 *                                Both: valid until the next call on the thread
 *   ahost_virus_expression       arriba_amd/csrc/device/virus_core.hpp stepped on the host over BAM records in host memory: the counters the device gives (its comparator; the
 *                                CPU tier); valid until the next call on the thread
 *   ahost_virus_expression_table counters to the text: RPKM in double precision, related strains collapsed onto the most expressed one, the thresholds of 100 bases and 5 %,
 *                                numbers as awk prints them, rows in the order of `LC_ALL=C sort -k6,6gr`; valid until the next call on the thread
 *   ahost_virus_expression_write the text into `path`, through path.tmp; on a failure nothing is left behind
 *   ahost_virus_expression_file  all of it for a file (BAM in BGZF, gzip or raw; SAM text) with the patterns of the session: what --host-ingest runs */
typedef struct {
	uint32_t n_ref, n_viruses;
	const int32_t* viral_ref;     /* [n_viruses] ascending refIDs */
	const uint32_t* viral_length; /* [n_viruses] LN */
	const char* names;            /* the names of the viral contigs, one behind the other */
	const uint32_t* name_offset;  /* [n_viruses + 1] */
} ahost_virus_contigs;
int ahost_virus_contigs_of_session(ahost_session* session, ahost_virus_contigs* contigs);
int ahost_virus_contigs_of(const void* input_header, size_t size, const char* viral_contigs, ahost_virus_contigs* contigs);
int ahost_virus_expression(const void* records, size_t size, const ahost_virus_contigs* contigs, agpu_virus_counters* counters);
int ahost_virus_expression_table(const agpu_virus_counters* counters, const ahost_virus_contigs* contigs, const char** text, uint64_t* bytes);
int ahost_virus_expression_write(const agpu_virus_counters* counters, const ahost_virus_contigs* contigs, const char* path);
int ahost_virus_expression_file(ahost_session* session, const char* input_path, const char* path);
/* ---- --coverage: the host side of agpu_depth_begin / _next / _end (include/arriba_gpu.h) -- the per-base alignment depth of the records as bedGraph text (the rule: DESIGN.md
 * 4.13) ----
 *   ahost_depth_contigs_of_session  the contigs of the header of the file the last ahost_bam_open opened: what agpu_depth_begin takes
 *   ahost_depth_contigs_of   the same from the head of an uncompressed input in memory (a BAM header, or the '@' lines of SAM text).  Both: valid until the next call on the thread
 *   ahost_depth_track        arriba_amd/csrc/device/depth_core.hpp stepped on the host over BAM records in host memory: the text and the statistics the device gives (its
 *                            comparator; the CPU tier); the text is valid until the next call on the thread
 *   ahost_depth_line         the line formatter alone: NAME\tSTART\tEND\tDEPTH\n into out[0 .. capacity); *bytes: its length (nothing is written if it does not fit: -1)
 *   ahost_depth_write        bytes into `path`, through path.tmp; on a failure nothing is left behind
 *   ahost_depth_file         all of it for a file (BAM in BGZF, gzip or raw; SAM text): what --host-ingest runs; stats may be NULL */
typedef struct {
	uint32_t n_ref;
	const uint32_t* length;      /* [n_ref] LN */
	const char* names;           /* the names of the contigs, one behind the other */
	const uint32_t* name_offset; /* [n_ref + 1] */
} ahost_depth_contigs;
int ahost_depth_contigs_of_session(ahost_session* session, ahost_depth_contigs* contigs);
int ahost_depth_contigs_of(const void* input_header, size_t size, ahost_depth_contigs* contigs);
int ahost_depth_track(const void* records, size_t size, const ahost_depth_contigs* contigs, const char** text, uint64_t* bytes, agpu_depth_stats* stats);
int ahost_depth_line(const char* name, uint32_t start, uint32_t end, uint32_t depth, char* out, uint32_t capacity, uint32_t* bytes);
int ahost_depth_write(const void* text, uint64_t bytes, const char* path);
int ahost_depth_file(const char* input_path, const char* path, agpu_depth_stats* stats);
/* ---- --gene-counts: the host side of agpu_gene_counts (include/arriba_gpu.h) -- reads per gene in three columns, the file STAR writes as ReadsPerGene.out.tab (the rule: DESIGN.md
 * 4.15).  A table is counts[c * (n_genes + 4) + row] as agpu_gene_counts fills it; n_counts = 3 * (n_genes + 4) is checked against the session ----
 *   ahost_gene_counts_genes   n_genes of the session's gene table (its GTF genes) and their gene_ids as loaded, each followed by "\n", in table order (ids, bytes: may be NULL; valid
 *                             until the next call on the thread)
 *   ahost_gene_counts_of      arriba_amd/csrc/device/genecount_core.hpp stepped on the host over BAM records in host memory (the device's comparator; the CPU tier).  input_header:
 *                             the head of the input the records come from (a BAM header, or the '@' lines of SAM text): its references are looked up among the contigs of the
 *                             session by name, their LN clips the blocks
 *   ahost_gene_counts_text    a table and the session's gene ids -> the text of the file: N_unmapped, N_multimapping, N_noFeature, N_ambiguous, then ID\tc0\tc1\tc2\n per gene; valid
 *                             until the next call on the thread
 *   ahost_gene_counts_write   that text into `path`, through path.tmp; on a failure nothing is left behind
 *   ahost_gene_counts_file    all of it for a file (BAM in BGZF, gzip or raw; SAM text): what --host-ingest runs; stats may be NULL */
int ahost_gene_counts_genes(ahost_session* session, uint32_t* n_genes, const char** ids, uint64_t* bytes);
int ahost_gene_counts_of(ahost_session* session, const void* input_header, size_t header_size, const void* records, size_t size, uint64_t* counts, uint64_t n_counts, agpu_gene_count_stats* stats /* may be NULL */);
int ahost_gene_counts_text(ahost_session* session, const uint64_t* counts, uint64_t n_counts, const char** text, uint64_t* bytes);
int ahost_gene_counts_write(ahost_session* session, const uint64_t* counts, uint64_t n_counts, const char* path);
int ahost_gene_counts_file(ahost_session* session, const char* input_path, const char* path, agpu_gene_count_stats* stats);
/* ---- --splice-junctions: the host side of agpu_splice_junctions (include/arriba_gpu.h) -- the table of splice junctions, the file STAR writes as SJ.out.tab (the rule: DESIGN.md
 * 4.16).  A row table is what agpu_splice_junctions gives: agpu_junction_row, ordered by (ref, start, end) ----
 *   ahost_splice_junctions_of      arriba_amd/csrc/device/junction_core.hpp stepped on the host over BAM records in host memory (the device's comparator; the CPU tier).
 *                                  input_header: the head of the input the records come from (a BAM header, or the '@' lines of SAM text): its references are looked up among the
 *                                  contigs of the session by name (motif from its assembly, annotated from its exon chains), their LN bounds the introns.  The rows are valid until
 *                                  the next call on the thread
 *   ahost_splice_junctions_text    a row table and the names of the references (ahost_depth_contigs_of / _of_session) -> the text of the file:
 *                                  NAME\ts+1\te+1\tstrand\tmotif\tannotated\tunique\tmultimapping\toverhang\n per row; valid until the next call on the thread
 *   ahost_splice_junctions_write   that text into `path`, through path.tmp; on a failure nothing is left behind
 *   ahost_splice_junctions_file    all of it for a file (BAM in BGZF, gzip or raw; SAM text): what --host-ingest runs; stats may be NULL */
int ahost_splice_junctions_of(ahost_session* session, const void* input_header, size_t header_size, const void* records, size_t size, const agpu_junction_row** rows, uint64_t* n_rows, agpu_junction_stats* stats /* may be NULL */);
int ahost_splice_junctions_text(const ahost_depth_contigs* contigs, const agpu_junction_row* rows, uint64_t n_rows, const char** text, uint64_t* bytes);
int ahost_splice_junctions_write(const ahost_depth_contigs* contigs, const agpu_junction_row* rows, uint64_t n_rows, const char* path);
int ahost_splice_junctions_file(ahost_session* session, const char* input_path, const char* path, agpu_junction_stats* stats);
/* ---- --allele-counts: the host side of agpu_allele_counts (include/arriba_gpu.h) -- the bases the records show at a list of known positions (the rule: DESIGN.md 4.17) ----
 *   ahost_allele_sites_load        reads a sites file (text; a line per site, cut at tabs: contig, 1-based position in plain decimal, further fields ignored -- the body of a VCF
 *                                  is one; empty lines and lines that begin with '#' are skipped) and places every line on the references of input_header (a BAM header, or the
 *                                  '@' lines of SAM text): the name byte for byte, else once more with a leading "chr" removed or added; no such reference, or a position beyond
 *                                  its LN: unplaced (ref 0xFFFFFFFF).  input_header NULL: every line unplaced (the file is only checked).  A file that cannot be read, a line with
 *                                  fewer than two fields, an empty position, one with a non-digit, 0 or above 2^31-1: refused, the message names the line.  The list belongs to
 *                                  the caller until ahost_allele_sites_free
 *   ahost_allele_sites_place_session   places the lines of a loaded list again, on the references of the file the last ahost_bam_open opened
 *   ahost_allele_counts_of         arriba_amd/csrc/device/allele_core.hpp stepped on the host over BAM records in host memory (the device's comparator; the CPU tier).  sites: as
 *                                  placed on input_header; REF comes from the assembly of the session.  The rows (one per site, in their order) are valid until the next call on
 *                                  the thread
 *   ahost_allele_counts_text       a row table and the list it belongs to -> the text of the file: "#CONTIG\tPOS\tREF\tA\tC\tG\tT\tN\tDEL\tSKIP\tLOWQ\n", then a line per site with the
 *                                  contig as the sites file spells it; valid until the next call on the thread
 *   ahost_allele_counts_write      that text into `path`, through path.tmp; on a failure nothing is left behind
 *   ahost_allele_counts_file       all of it for a file (BAM in BGZF, gzip or raw; SAM text): what --host-ingest runs; stats may be NULL */
typedef struct {
	uint64_t n_sites, placed;
	const agpu_allele_site* sites;  /* [n_sites], in the order of the lines */
	const char* names;              /* the contigs as the file spells them, one behind the other */
	const uint64_t* name_offset;    /* [n_sites + 1] */
	void* owner;
} ahost_allele_sites;
int ahost_allele_sites_load(const char* path, const void* input_header, size_t header_size, ahost_allele_sites* sites);
int ahost_allele_sites_place_session(ahost_session* session, ahost_allele_sites* sites);
void ahost_allele_sites_free(ahost_allele_sites* sites);
int ahost_allele_counts_of(ahost_session* session, const void* input_header, size_t header_size, const void* records, size_t size, const ahost_allele_sites* sites, uint32_t min_mapq, uint32_t min_baseq,
                           const agpu_allele_row** rows, agpu_allele_stats* stats /* may be NULL */);
int ahost_allele_counts_text(const ahost_allele_sites* sites, const agpu_allele_row* rows, uint64_t n_rows, const char** text, uint64_t* bytes);
int ahost_allele_counts_write(const ahost_allele_sites* sites, const agpu_allele_row* rows, uint64_t n_rows, const char* path);
int ahost_allele_counts_file(ahost_session* session, const char* input_path, const char* sites_path, const char* path, uint32_t min_mapq, uint32_t min_baseq, agpu_allele_stats* stats);
/* ---- --variant-sites: the host side of agpu_variant_sites (include/arriba_gpu.h) -- the positions at which the records show a base that differs from the assembly, with their
 * base counts (the rule: DESIGN.md 4.21).  A row table is what agpu_variant_sites gives: agpu_variant_row, ordered by (ref, pos) ----
 *   ahost_variant_sites_of         arriba_amd/csrc/device/variant_core.hpp and allele_core.hpp stepped on the host over BAM records in host memory (the device's comparator; the
 *                                  CPU tier).  input_header: the head of the input the records come from (a BAM header, or the '@' lines of SAM text): its references are looked
 *                                  up among the contigs of the session by name (REF from its assembly), their LN bounds the positions.  min_mapq, min_baseq: at most 255;
 *                                  min_alt: 1 .. 2^31-1; min_percent: 0 .. 100.  The rows are valid until the next call on the thread
 *   ahost_variant_sites_text       a row table and the names of the references (ahost_depth_contigs_of / _of_session) -> the text of the file:
 *                                  "#CONTIG\tPOS\tREF\tALT\tA\tC\tG\tT\tN\tDEL\tSKIP\tLOWQ\n", then a line per row, the reported alts joined by ',' in the order A, C, G, T; valid
 *                                  until the next call on the thread
 *   ahost_variant_sites_write      that text into `path`, through path.tmp; on a failure nothing is left behind
 *   ahost_variant_sites_file       all of it for a file (BAM in BGZF, gzip or raw; SAM text): what --host-ingest runs; stats may be NULL */
int ahost_variant_sites_of(ahost_session* session, const void* input_header, size_t header_size, const void* records, size_t size, uint32_t min_mapq, uint32_t min_baseq, uint32_t min_alt, uint32_t min_percent,
                           const agpu_variant_row** rows, uint64_t* n_rows, agpu_variant_stats* stats /* may be NULL */);
int ahost_variant_sites_text(const ahost_depth_contigs* contigs, const agpu_variant_row* rows, uint64_t n_rows, const char** text, uint64_t* bytes);
int ahost_variant_sites_write(const ahost_depth_contigs* contigs, const agpu_variant_row* rows, uint64_t n_rows, const char* path);
int ahost_variant_sites_file(ahost_session* session, const char* input_path, const char* path, uint32_t min_mapq, uint32_t min_baseq, uint32_t min_alt, uint32_t min_percent, agpu_variant_stats* stats);
/* ---- --indel-sites: the host side of agpu_indel_sites (include/arriba_gpu.h) -- the insertions and deletions of the CIGARs, left-normalised against the assembly, with their
 * support and the depth at their anchor (the rule: DESIGN.md 4.22).  A row table is what agpu_indel_sites gives: agpu_indel_row, ordered by (ref, pos, type, length, bases) ----
 *   ahost_indel_sites_of           arriba_amd/csrc/device/indel_core.hpp and allele_core.hpp stepped on the host over BAM records in host memory (the device's comparator; the CPU
 *                                  tier).  input_header: the head of the input the records come from (a BAM header, or the '@' lines of SAM text): its references are looked up
 *                                  among the contigs of the session by name (the events are normalised against its assembly), their LN bounds the positions.  min_mapq: at most
 *                                  255; min_alt: 1 .. 2^31-1; min_percent: 0 .. 100.  ARRIBA_INDEL_MAX_SHIFT is read as the device reads it.  The rows are valid until the next
 *                                  call on the thread
 *   ahost_indel_sites_text         a row table and the names of the references (ahost_depth_contigs_of / _of_session) -> the text of the file:
 *                                  "#CONTIG\tPOS\tREF\tTYPE\tLENGTH\tBASES\tSUPPORT\tDEPTH\n", then a line per row; BASES: the inserted bases, or the deleted bases of the assembly of
 *                                  the session in upper case up to 64 of them, else "."; valid until the next call on the thread
 *   ahost_indel_sites_write        that text into `path`, through path.tmp; on a failure nothing is left behind
 *   ahost_indel_sites_file         all of it for a file (BAM in BGZF, gzip or raw; SAM text): what --host-ingest runs; stats may be NULL */
int ahost_indel_sites_of(ahost_session* session, const void* input_header, size_t header_size, const void* records, size_t size, uint32_t min_mapq, uint32_t min_alt, uint32_t min_percent,
                         const agpu_indel_row** rows, uint64_t* n_rows, agpu_indel_stats* stats /* may be NULL */);
int ahost_indel_sites_text(ahost_session* session, const ahost_depth_contigs* contigs, const agpu_indel_row* rows, uint64_t n_rows, const char** text, uint64_t* bytes);
int ahost_indel_sites_write(ahost_session* session, const ahost_depth_contigs* contigs, const agpu_indel_row* rows, uint64_t n_rows, const char* path);
int ahost_indel_sites_file(ahost_session* session, const char* input_path, const char* path, uint32_t min_mapq, uint32_t min_alt, uint32_t min_percent, agpu_indel_stats* stats);
/* ---- --realign-reads: the host side of agpu_realign_* (include/arriba_gpu.h) -- the records split into the templates to realign and the templates to keep, as SAM text (the
 * rule: DESIGN.md 4.18) ----
 *   ahost_realign_plan_of          what the split needs from the assembly of the session for the references of input_header (a BAM header, or the '@' lines of SAM text): a byte
 *                                  per reference, 1 if it is a contig of the assembly -- the names compared as the loaders of the session compare them, a leading "chr" removed on
 *                                  both sides --, and the header of the file of the kept templates: "@HD\tVN:1.4\tSO:unsorted\n", then "@SQ\tSN:...\tLN:...\n" per contig of the
 *                                  assembly in the order of its file, spelled as the input spells it where the input has it.  Valid until the next call on the thread
 *   ahost_realign_plan_of_session  the same for the file the last ahost_bam_open opened
 *   ahost_realign_split_of         arriba_amd/csrc/device/realign_core.hpp stepped on the host over BAM records in host memory (the device's comparator; the CPU tier): the bytes
 *                                  of the two files, the second with its header (want_kept 0: kept may be NULL).  Valid until the next call on the thread.
 *                                  ARRIBA_REALIGN_HASH_BITS: bits of the name hash (the tests force collisions)
 *   ahost_realign_split_file       all of it for a file (BAM in BGZF, gzip or raw; SAM text), written through NAME.tmp: what --host-ingest runs; kept_path and stats may be NULL */
typedef struct {
	uint32_t n_ref;
	const uint8_t* in_assembly;     /* [n_ref] */
	const char* header;             /* of the file of the kept templates */
	uint64_t header_bytes;
} ahost_realign_plan;
int ahost_realign_plan_of(ahost_session* session, const void* input_header, size_t header_size, ahost_realign_plan* plan);
int ahost_realign_plan_of_session(ahost_session* session, ahost_realign_plan* plan);
int ahost_realign_split_of(ahost_session* session, const void* input_header, size_t header_size, const void* records, size_t size, int want_kept, const char** realign, uint64_t* realign_bytes, const char** kept, uint64_t* kept_bytes,
                           agpu_realign_stats* stats /* may be NULL */);
int ahost_realign_split_file(ahost_session* session, const char* input_path, const char* realign_path, const char* kept_path, agpu_realign_stats* stats);
/* ---- --rna-metrics: the host side of agpu_rna_metrics (include/arriba_gpu.h) -- the alignment QC table of an input (the rule: DESIGN.md 4.19).  A counter block is
 * AGPU_RNA_METRICS_WORDS words as agpu_rna_metrics fills them; n_counters is checked ----
 *   ahost_rrna_intervals_load  reads an rRNA interval file (--rrna-intervals; BED: contig, start, end separated by tabs, 0-based and half open; further fields are ignored; lines that
 *                              start with '#', "track" or "browser" and empty lines are skipped).  A line that does not parse or whose start lies behind its end is refused with
 *                              its number.  n_intervals may be NULL
 *   ahost_region_track         the region track of the session for an interval file (NULL: no rRNA intervals): built when it is asked for first and kept until ahost_close; the
 *                              pointers of `track` stay valid as long.  Contig names are looked up without a leading "chr" among the contigs of the assembly and the annotation; a
 *                              line on another contig is counted in info->intervals_unknown_contig and ignored.  info may be NULL
 *   ahost_rna_metrics_of       arriba_amd/csrc/device/rnametrics_core.hpp stepped on the host over BAM records in host memory (the device's comparator; the CPU tier).  input_header:
 *                              the head of the input the records come from (a BAM header, or the '@' lines of SAM text): its references are looked up among the contigs of the
 *                              session by name, their LN clips the blocks
 *   ahost_rna_metrics_text     a counter block -> the text of the file; valid until the next call on the thread
 *   ahost_rna_metrics_write    that text into `path`, through path.tmp; on a failure nothing is left behind
 *   ahost_rna_metrics_file     all of it for a file (BAM in BGZF, gzip or raw; SAM text): what --host-ingest runs; rrna_intervals_path and stats may be NULL */
typedef struct {
	uint32_t n_contigs;                 /* of the track: the contigs the session knew when it was opened */
	uint64_t runs;
	uint64_t intervals;                 /* lines of the interval file */
	uint64_t intervals_unknown_contig;  /* ... on a contig the session lacks: ignored */
	uint64_t bytes;                     /* of the arrays of the track */
} ahost_region_track_info;
int ahost_rrna_intervals_load(const char* path, uint64_t* n_intervals);
int ahost_region_track(ahost_session* session, const char* rrna_intervals_path, agpu_region_track* track, ahost_region_track_info* info);
int ahost_rna_metrics_of(ahost_session* session, const char* rrna_intervals_path, const void* input_header, size_t header_size, const void* records, size_t size, uint64_t* counters, uint64_t n_counters,
                         agpu_rna_metrics_stats* stats /* may be NULL */);
int ahost_rna_metrics_text(const uint64_t* counters, uint64_t n_counters, const char** text, uint64_t* bytes);
int ahost_rna_metrics_write(const uint64_t* counters, uint64_t n_counters, const char* path);
int ahost_rna_metrics_file(ahost_session* session, const char* input_path, const char* rrna_intervals_path, const char* path, agpu_rna_metrics_stats* stats);
int ahost_adopt_device_ingest(ahost_session* session, const agpu_ingest_result* result, const uint64_t* viral_read_counts, const uint16_t* coverage, const uint8_t* fragment_starts, const uint8_t* fragment_ends);
int ahost_set_batch_rows(ahost_session* session, const agpu_batch_rows* rows, const uint32_t* fragments /* [rows->n] ascending: the fragment every row holds; NULL: row k holds the fragment
                         of entry k of the read lists of the table the next ahost_write_fusions writes (the reads of a candidate next to each other; the table then carries read_filter_of_rows) */);

/* A blacklist (allow_keywords = 1: the second column may hold a keyword, source/filter_blacklisted_ranges.cpp:91-102) or a known-fusions file
 * (allow_keywords = 0) parsed into rules for agpu_filter_blacklisted_ranges / agpu_recover_known_fusions (parse_blacklist_item, parse_range:
 * source/filter_blacklisted_ranges.cpp:17-118; plain or gzip).  Malformed lines are skipped with the reference's warning.  The rules stay
 * valid until the next call with the same allow_keywords or ahost_close. */
int ahost_load_range_rules(ahost_session* session, const char* path, int allow_keywords, const agpu_range_rule** rules, uint32_t* n_rules);

/* The output files (write_fusions_to_file, source/output_fusions.cpp:1043-1261, called at source/arriba.cpp:604-610).  The candidate table is what the
 * device hands back at the end of the workflow: agpu_get_candidates + agpu_get_candidate_read_lists, agpu_get_evalues, agpu_assign_confidence,
 * agpu_candidate_iteration_order (the discarded candidates are written in the iteration order of the reference's fusions_t), agpu_get_filters
 * (filter of every fragment) and agpu_get_gene_table (GTF genes + the dummy genes of the sample).  write_discarded = 0: the candidates that passed
 * all filters, sorted by support; 1: the discarded ones.  print_extra_info: read identifiers (and, once built, transcript / peptide columns). */
typedef struct {
	uint32_t n_candidates;
	const uint32_t* gene1; const uint32_t* gene2; const uint32_t* contigs; const int32_t* breakpoint1; const int32_t* breakpoint2; const uint32_t* flags; const uint8_t* filter;
	const uint32_t* split_reads1; const uint32_t* split_reads2; const uint32_t* discordant_mates;
	const uint64_t* list_offset;   /* [3 * n_candidates + 1]; 64-bit: with -U 32767 the lists of the candidates of a sample pass 2^32 entries */
	const uint32_t* read_lists;
	const float* evalue; const uint8_t* confidence; const uint32_t* iteration_rank;
	const uint8_t* read_filter;    /* [fragments of the session's batch] */
	const int32_t* closest_genomic_breakpoint1; const int32_t* closest_genomic_breakpoint2; /* agpu_get_genomic_support; NULL = no structural variants given */
	uint32_t n_genes; const uint16_t* gene_contig; const int32_t* gene_start; const int32_t* gene_end;
	const uint8_t* read_filter_of_rows; /* instead of read_filter (then NULL): the filters of the fragments handed over with ahost_set_batch_rows, in the order of the rows (agpu_get_filters_of) */
} ahost_fusion_table;
int ahost_write_fusions(ahost_session* session, const ahost_fusion_table* table, const char* path, int write_discarded, int print_extra_info, unsigned int max_itd_length, int max_mate_gap,
                        int fill_sequence_gaps /* -I: complete the fusion transcript from the assembly along the chosen transcripts */);
/* --supporting-alignments under --host-ingest (described with ahost_supporting_alignments above) */
int ahost_supporting_alignments_file(ahost_session* session, const ahost_fusion_table* table, const char* input_path, int64_t window, const char* prefix, agpu_supporting_info* info /* may be NULL */);
/* The last output file of a sample written while the session reads the next one (arriba_workflow_defer_output): ahost_detach_sample moves what the writer reads of the SAMPLE --
 * coverage_t, the rows of ahost_set_batch_rows, the contig names as its header left them -- out of the session (which then holds no sample until its next ingest);
 * ahost_write_fusions_of writes from there on any thread, beside ahost_bam_open / ahost_bam_next / ahost_adopt_device_ingest of the next sample on the same session, with the
 * reference data of the session (annotation, assembly, tags, protein domains), which no sample changes; ahost_release_sample gives the vectors of the rows back to the session.
 * ahost_close waits for the samples that are still detached.  (reference: the same call as ahost_write_fusions, source/output_fusions.cpp:791-1007) */
typedef struct ahost_detached_sample ahost_detached_sample;
ahost_detached_sample* ahost_detach_sample(ahost_session* session);
int ahost_write_fusions_of(ahost_detached_sample* sample, const ahost_fusion_table* table, const char* path, int write_discarded, int print_extra_info, unsigned int max_itd_length, int max_mate_gap,
                           int fill_sequence_gaps);
void ahost_release_sample(ahost_detached_sample* sample);
/* One sample over several ranks that hold the same candidates: the rows part, part + parts, part + 2 parts, ... of the file ahost_write_fusions would write, as text
 * (the header line in front of the rows of part 0); *text stays valid until the next call.  Rows are independent of each other: the rank that gathers the texts of all
 * parts writes row k of the file from the text of part k % parts. */
int ahost_format_fusions(ahost_session* session, const ahost_fusion_table* table, int write_discarded, int print_extra_info, unsigned int max_itd_length, int max_mate_gap, int fill_sequence_gaps,
                         unsigned int part, unsigned int parts, const char** text, uint64_t* bytes);
/* the fragments whose rows ahost_write_fusions(table, write_discarded, print_extra_info = 1) reads: the supporting reads of the candidates it writes, ascending, unique.
 * Call with fragments == NULL to get the number in *count.  (Without print_extra_info the writer needs no rows.) */
int ahost_fusion_table_reads(const ahost_fusion_table* table, int write_discarded, uint32_t* fragments, uint64_t capacity, uint64_t* count);
/* estimate_fragment_length's float sum of the read lengths (source/read_stats.cpp:30-37, hazard H4: sequential, in name order) over lengths fetched from the
 * device (agpu_get_read_lengths); continues `running_sum` */
float ahost_read_length_sum_of(float running_sum, const uint32_t* mate1_lengths, const uint32_t* mate2_lengths, uint64_t count);
/* Optional inputs of the output files: a tags file (-t; load_tags, source/annotate_tags.cpp:11-44) and protein domains in GFF3 (-p; load_protein_domains,
 * source/annotate_protein_domains.cpp:33-121).  Loaded into the session; ahost_write_fusions fills the columns `tags` and `retained_protein_domains` from them. */
int ahost_load_tags(ahost_session* session, const char* path);
/* Structural variants from WGS (-d) for agpu_mark_genomic_support: Arriba's four-column format or VCF (source/filter_genomic_support.cpp:15-165).  The
 * variants stay valid until the next call or ahost_close. */
int ahost_load_genomic_breakpoints(ahost_session* session, const char* path, const agpu_genomic_breakpoint** variants, uint32_t* n_variants);
int ahost_load_protein_domains(ahost_session* session, const char* path);

const agpu_annotation_view* ahost_annotation_view(ahost_session* session);
const agpu_genome_view* ahost_genome_view(ahost_session* session);
const agpu_coverage_view* ahost_coverage_view(ahost_session* session);  /* coverage_t of the ingest for agpu_upload_coverage; NULL before an ingest */
const agpu_batch_view* ahost_batch_view(ahost_session* session);
/* Shards of the batch for one context per GPU: contiguous ranges of fragments in name order.  ahost_shard_boundary moves a cut forward
 * until it does not separate fragments of one read name (mark_multimappers compares neighbours, source/read_chimeric_alignments.cpp:792-802);
 * ahost_batch_slice_view returns the view of fragments [first, first + count) (valid until the next call). */
uint64_t ahost_shard_boundary(ahost_session* session, uint64_t target);
const agpu_batch_view* ahost_batch_slice_view(ahost_session* session, uint64_t first, uint64_t count);

uint64_t ahost_fragment_count(ahost_session* session);
uint64_t ahost_mapped_reads(ahost_session* session);
uint64_t ahost_viral_read_total(ahost_session* session); /* the pristine reads the ingest counted on viral contigs (mapped_viral_reads_by_contig, source/read_chimeric_alignments.cpp:736-739), summed */
/* FNV-1a over coverage_t as the ingest built it (coverage windows, fragment start/end flags of every contig; reference: coverage_t,
 * source/read_stats.hpp:17-27) -- a fingerprint for tests and for comparing runs, e.g. with different numbers of ingest threads. */
uint64_t ahost_coverage_checksum(ahost_session* session);
uint32_t ahost_contig_count(ahost_session* session);
const char* ahost_contig_name(ahost_session* session, uint32_t contig);
/* "QNAME,HI" of fragment i (the reference's map key); valid until the session is closed */
const char* ahost_fragment_name(ahost_session* session, uint64_t i, uint32_t* length);

/* detect_strandedness (source/read_stats.cpp:94-143): 0 no, 1 yes, 2 reverse */
int ahost_detect_strandedness(ahost_session* session);

/* per-contig verdicts of filter_top_expressed_viral_contigs (source/filter_top_expressed_viral_contigs.cpp:51-127) and
 * filter_low_coverage_viral_contigs (source/filter_low_coverage_viral_contigs.cpp:11-27); pairs = (viral contig, gene id)
 * from agpu_get_viral_integration_sites, gene_bits = AGPU_GBIT_* for every gene id incl. dummy genes */
int ahost_viral_verdicts(ahost_session* session, const uint32_t* pairs, uint64_t n_pairs, const uint8_t* gene_bits, uint32_t n_genes,
                         unsigned int top_count, float min_covered_fraction, uint8_t* top_expressed_verdict, uint8_t* low_coverage_verdict);

/* estimate_fragment_length (source/read_stats.cpp:11-92) + source/arriba.cpp:352-364.  mate_gaps / fragments_visited come from
 * agpu_fragment_length_samples.  Returns 1 if estimated, 0 if the defaults were used. */
int ahost_estimate_fragment_length(ahost_session* session, const int32_t* mate_gaps, uint32_t n_samples, uint64_t fragments_visited, unsigned int default_fragment_length,
                                   float* mate_gap_mean, float* mate_gap_stddev, float* read_length_mean, int32_t* max_mate_gap);

/* The same for a sample whose fragments are spread over several sessions (shards in name order): the reference's float sum of the read
 * lengths is sequential over the whole sample (hazard H4), so each shard continues the running sum of the shards before it
 * (ahost_read_length_sum) and the estimate is made from the mate gaps, the final sum and the number of fragments visited. */
float ahost_read_length_sum(ahost_session* session, float running_sum, uint64_t first, uint64_t count);
int ahost_estimate_fragment_length_from_sums(const int32_t* mate_gaps, uint32_t n_samples, float read_length_sum, uint64_t fragments_visited, unsigned int default_fragment_length,
                                             float* mate_gap_mean, float* mate_gap_stddev, float* read_length_mean, int32_t* max_mate_gap);

/* Position of every candidate in the iteration order of the reference's fusions_t (std::unordered_map with the tuple hash of
 * source/common.hpp:286-314), given the candidates in insertion order as agpu_get_candidates returns them.  Stages whose result
 * depends on that order (partner dedup in estimate_expected_fusions, source/filter_relative_support.cpp:22-29) take it as input. */
int ahost_candidate_iteration_order(uint64_t n, const uint32_t* gene1, const uint32_t* gene2, const uint32_t* contigs, const int32_t* breakpoint1, const int32_t* breakpoint2, const uint32_t* flags, uint32_t* iteration_rank);

#ifdef __cplusplus
}
#endif

#endif
