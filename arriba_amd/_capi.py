"""ctypes bindings of the two C ABIs (include/arriba_gpu.h, include/arriba_host.h).

The device library is mandatory: there is no CPU fallback for the hot path.  Loading fails loudly if
``arriba_amd/lib/libarriba_gpu.so`` is missing (build it with ``__graft_entry__.build()``).
"""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_size_t, c_uint8, c_uint16, c_uint32, c_uint64, c_void_p

LIB_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib")
FILTER_COUNT = 38
KERNEL_NAME_LENGTH = 48
FILTER_NAMES = [
    "", "duplicates", "inconsistently_clipped", "homopolymer", "read_through", "same_gene", "small_insert_size", "long_gap", "hairpin",
    "multimappers", "mismatches", "mismappers", "relative_support", "intronic", "non_coding_neighbors", "intragenic_exonic",
    "internal_tandem_duplication", "min_support", "known_fusions", "spliced", "blacklist", "end_to_end", "in_vitro", "merge_adjacent",
    "select_best", "marginal_read_through", "short_anchor", "no_coverage", "many_spliced", "no_genomic_support", "uninteresting_contigs",
    "viral_contigs", "top_expressed_viral_contigs", "low_coverage_viral_contigs", "genomic_support", "isoforms", "low_entropy", "homologs",
]


class FlatIndex(ctypes.Structure):
    _fields_ = [("n_contigs", c_uint32), ("contig_offset", POINTER(c_uint32)), ("n_keys", c_uint32), ("keys", POINTER(c_int32)),
                ("member_offset", POINTER(c_uint32)), ("n_members", c_uint32), ("members", POINTER(c_uint32))]


class AnnotationView(ctypes.Structure):
    _fields_ = [("n_genes", c_uint32), ("gene_contig", POINTER(c_uint16)), ("gene_start", POINTER(c_int32)), ("gene_end", POINTER(c_int32)),
                ("gene_bits", POINTER(c_uint8)), ("gene_exonic_length", POINTER(c_int32)),
                ("n_exons", c_uint32), ("exon_start", POINTER(c_int32)), ("exon_end", POINTER(c_int32)), ("exon_gene", POINTER(c_uint32)),
                ("exon_previous", POINTER(c_int32)), ("exon_next", POINTER(c_int32)), ("exon_cds_start", POINTER(c_int32)), ("exon_cds_end", POINTER(c_int32)),
                ("exon_index", FlatIndex), ("gene_index", FlatIndex)]


class GenomeView(ctypes.Structure):
    _fields_ = [("n_contigs", c_uint32), ("contig_offset", POINTER(c_uint64)), ("contig_bits", POINTER(c_uint8)), ("bases", c_void_p)]


class CoverageView(ctypes.Structure):
    _fields_ = [("n_contigs", c_uint32), ("window_offset", POINTER(c_uint64)), ("coverage", POINTER(c_uint16)), ("fragment_starts", POINTER(c_uint8)), ("fragment_ends", POINTER(c_uint8))]


class RangeItem(ctypes.Structure):
    _fields_ = [("type", c_uint8), ("strand_defined", c_uint8), ("strand", c_uint8), ("reserved", c_uint8), ("contig", c_uint32), ("start", c_int32), ("end", c_int32), ("gene", c_uint32)]


class RangeRule(ctypes.Structure):
    _fields_ = [("first", RangeItem), ("second", RangeItem)]


class GenomicBreakpoint(ctypes.Structure):
    _fields_ = [("contig1", c_uint32), ("contig2", c_uint32), ("position1", c_int32), ("position2", c_int32), ("upstream1", c_uint8), ("upstream2", c_uint8), ("reserved", c_uint8 * 2)]


class FusionTable(ctypes.Structure):
    _fields_ = [("n_candidates", c_uint32), ("gene1", c_void_p), ("gene2", c_void_p), ("contigs", c_void_p), ("breakpoint1", c_void_p), ("breakpoint2", c_void_p), ("flags", c_void_p), ("filter", c_void_p),
                ("split_reads1", c_void_p), ("split_reads2", c_void_p), ("discordant_mates", c_void_p), ("list_offset", c_void_p), ("read_lists", c_void_p), ("evalue", c_void_p), ("confidence", c_void_p),
                ("iteration_rank", c_void_p), ("read_filter", c_void_p), ("closest_genomic_breakpoint1", c_void_p), ("closest_genomic_breakpoint2", c_void_p), ("n_genes", c_uint32), ("gene_contig", c_void_p), ("gene_start", c_void_p), ("gene_end", c_void_p), ("read_filter_of_rows", c_void_p)]


class SelectedCandidates(ctypes.Structure):
    _fields_ = [(name, c_void_p) for name in ("candidate", "gene1", "gene2", "contigs", "breakpoint1", "breakpoint2", "flags", "filter", "split_reads1", "split_reads2", "discordant_mates", "evalue", "confidence",
                                              "iteration_rank", "closest_genomic_breakpoint1", "closest_genomic_breakpoint2")]


class BatchView(ctypes.Structure):
    _fields_ = [("n", c_uint64), ("n_aln", POINTER(c_uint8)), ("fbits", POINTER(c_uint8)), ("group", POINTER(c_uint32)),
                ("contig", POINTER(c_uint16) * 3), ("start", POINTER(c_int32) * 3), ("end", POINTER(c_int32) * 3), ("abits", POINTER(c_uint8) * 3),
                ("cigar_offset", POINTER(c_uint32) * 3), ("cigar_count", POINTER(c_uint16) * 3),
                ("cigar_pool_size", c_uint64), ("cigar_pool", POINTER(c_uint32)),
                ("seq_offset", POINTER(c_uint32) * 2), ("seq_length", POINTER(c_uint32) * 2),
                ("seq_pool_size", c_uint64), ("seq_pool", POINTER(c_uint8))]


class IngestConfig(ctypes.Structure):
    _fields_ = [("n_targets", c_uint32), ("tid_to_contig", POINTER(c_uint32)), ("first_record_offset", c_uint64), ("stream_size_hint", c_uint64), ("n_contigs", c_uint32),
                ("coverage_window_offset", POINTER(c_uint64)), ("external_duplicate_marking", c_uint8), ("max_itd_length", c_uint32), ("part_of_sample", c_uint8), ("host_buffers", c_uint8), ("role", c_uint8)]


ROLE_WHOLE, ROLE_SEPARATE_CHIMERIC, ROLE_SEPARATE_RNA = 0, 1, 2  # agpu_ingest_config.role (include/arriba_gpu.h: AGPU_ROLE_*)


class BgzfBlock(ctypes.Structure):
    _fields_ = [("raw_offset", c_uint64), ("payload_offset", c_uint32), ("payload_size", c_uint32), ("stream_offset", c_uint64), ("crc32", c_uint32), ("isize", c_uint32), ("skip", c_uint32), ("keep", c_uint32)]


class IngestResult(ctypes.Structure):
    _fields_ = [("records", c_uint64), ("fragments", c_uint64), ("mapped_reads", c_uint64), ("malformed_count", c_uint64), ("missing_hi_tag", c_uint64), ("no_chimeric_reads", c_uint8),
                ("names_were_sorted", c_uint8), ("windows", ctypes.c_uint16), ("reserved", c_uint8 * 4), ("stream_bytes", c_uint64)]


class SortedBamInfo(ctypes.Structure):
    """agpu_sorted_bam_info"""
    _fields_ = [("records", c_uint64), ("uncompressed_bytes", c_uint64), ("file_bytes", c_uint64), ("windows", c_uint64), ("window_bytes", c_uint64)]


class SortedBamIndex(ctypes.Structure):
    """agpu_sorted_bam_index_arrays: the sizes, then the arrays of the BAI index"""
    _fields_ = [("n_ref", c_uint32), ("n_chunks", c_uint64), ("n_intervals", c_uint64), ("n_no_coor", c_uint64)] + [
        (name, c_void_p) for name in ("chunk_key", "chunk_begin", "chunk_end", "interval_offset", "intervals", "ref_begin", "ref_end", "ref_mapped", "ref_unmapped")]


class SupportPoolInfo(ctypes.Structure):
    """agpu_support_pool_info"""
    _fields_ = [("names", c_uint64), ("stream_records", c_uint64), ("pooled_records", c_uint64), ("pool_bytes", c_uint64)]


class SupportingRows(ctypes.Structure):
    """agpu_supporting_rows: per row two (refID, 0-based breakpoint) pairs and the entries of the names that support it (CSR)"""
    _fields_ = [("n_rows", c_uint32), ("ref", c_void_p), ("breakpoint", c_void_p), ("name_begin", c_void_p), ("names", c_void_p)]


class SupportingInfo(ctypes.Structure):
    """agpu_supporting_info"""
    _fields_ = [(name, c_uint64) for name in ("rows", "records", "uncompressed_bytes", "file_bytes", "blocks", "windows", "window_bytes")]


class SupportingIndex(ctypes.Structure):
    """agpu_supporting_index_arrays: the sizes, then per record of the files its coordinates, bin and virtual offsets"""
    _fields_ = [("n_rows", c_uint32), ("n_records", c_uint64)] + [(name, c_void_p) for name in ("row_first", "ref", "pos", "end_flag", "bin", "begin", "end")]


class VirusCounters(ctypes.Structure):
    """agpu_virus_counters: what agpu_virus_expression / ahost_virus_expression count; the arrays belong to the callee"""
    _fields_ = [("total", c_uint64), ("n_viruses", c_uint32), ("n_active", c_uint32)] + [(name, c_void_p) for name in ("reads", "covered", "kmer_count", "active", "shared")] + [
        (name, c_uint64) for name in ("candidates", "kmer_keys", "kmer_rounds", "peak_bytes")] + [("seconds", ctypes.c_double * 4)]


class VirusContigs(ctypes.Structure):
    """ahost_virus_contigs: the viral contigs of a header -- slot v is reference viral_ref[v]"""
    _fields_ = [("n_ref", c_uint32), ("n_viruses", c_uint32), ("viral_ref", c_void_p), ("viral_length", c_void_p), ("names", c_void_p), ("name_offset", c_void_p)]


class DepthInfo(ctypes.Structure):
    """agpu_depth_info"""
    _fields_ = [("positions", c_uint64), ("window_bytes", c_uint64)]


class DepthStats(ctypes.Structure):
    """agpu_depth_stats: what agpu_depth_end / ahost_depth_track count"""
    _fields_ = [(name, c_uint64) for name in ("records", "segments", "runs", "covered_positions", "aligned_bases", "max_depth", "text_bytes", "position_windows", "text_windows", "peak_bytes")] + [("seconds", ctypes.c_double * 4)]


class MarkdupCounts(ctypes.Structure):
    """agpu_markdup_counts: what agpu_markdup_stats / ahost_markdup count"""
    _fields_ = [(name, c_uint64) for name in ("templates", "pairs", "fragments", "duplicate_pairs", "duplicate_fragments", "records_flagged", "records_changed", "peak_bytes")] + [("seconds", ctypes.c_double * 3)]


class GeneCountStats(ctypes.Structure):
    """agpu_gene_count_stats: what agpu_gene_counts / ahost_gene_counts_of count"""
    _fields_ = [(name, c_uint64) for name in ("records", "templates", "without_primary", "ends", "blocks", "peak_bytes")] + [("seconds", ctypes.c_double * 2)]


class JunctionRow(ctypes.Structure):
    """agpu_junction_row: a row of the table of --splice-junctions"""
    _fields_ = [("ref", c_uint32), ("start", c_int32), ("end", c_int32), ("strand", c_uint8), ("motif", c_uint8), ("annotated", c_uint8), ("reserved", c_uint8), ("unique", c_uint32), ("multimapping", c_uint32), ("overhang", c_uint32)]


class JunctionStats(ctypes.Structure):
    """agpu_junction_stats: what agpu_splice_junctions / ahost_splice_junctions_of count"""
    _fields_ = [(name, c_uint64) for name in ("records", "contributing", "crossings", "pairs", "junctions", "annotated", "peak_bytes")] + [("seconds", ctypes.c_double * 5)]


class AlleleSite(ctypes.Structure):
    """agpu_allele_site: a line of the sites file of --allele-counts, placed on a reference of the header (ref 0xFFFFFFFF: unplaced)"""
    _fields_ = [("ref", c_uint32), ("pos", c_int32)]


class AlleleRow(ctypes.Structure):
    """agpu_allele_row: the counts of a site"""
    _fields_ = [(name, c_uint32) for name in ("a", "c", "g", "t", "n", "del_", "skip", "lowq")] + [("ref_base", c_uint8), ("reserved", c_uint8 * 3)]


class AlleleStats(ctypes.Structure):
    """agpu_allele_stats: what agpu_allele_counts / ahost_allele_counts_of count"""
    _fields_ = [(name, c_uint64) for name in ("records", "contributing", "hits", "sites", "placed", "covered", "peak_bytes")] + [("seconds", ctypes.c_double * 3)]


class AlleleSites(ctypes.Structure):
    """ahost_allele_sites: the lines of a sites file as ahost_allele_sites_load placed them"""
    _fields_ = [("n_sites", c_uint64), ("placed", c_uint64), ("sites", POINTER(AlleleSite)), ("names", c_void_p), ("name_offset", POINTER(c_uint64)), ("owner", c_void_p)]


class VariantRow(ctypes.Structure):
    """agpu_variant_row: a reported site of --variant-sites with its counts"""
    _fields_ = [("ref", c_uint32), ("pos", c_int32)] + [(name, c_uint32) for name in ("a", "c", "g", "t", "n", "del_", "skip", "lowq")] + [("ref_base", c_uint8), ("alt_mask", c_uint8), ("reserved", c_uint8 * 2)]


class VariantStats(ctypes.Structure):
    """agpu_variant_stats: what agpu_variant_sites / ahost_variant_sites_of count"""
    _fields_ = [(name, c_uint64) for name in ("records", "contributing", "events", "runs", "candidates", "reported", "inconsistent", "peak_bytes")] + [("seconds", ctypes.c_double * 5)]


class IndelRow(ctypes.Structure):
    """agpu_indel_row: a reported event of --indel-sites"""
    _fields_ = [("ref", c_uint32), ("pos", c_int32), ("bases", c_uint64), ("length", c_uint32), ("support", c_uint32), ("depth", c_uint32), ("type", c_uint8), ("ref_base", c_uint8), ("reserved", c_uint8 * 2)]


class IndelStats(ctypes.Structure):
    """agpu_indel_stats: what agpu_indel_sites / ahost_indel_sites_of count"""
    _fields_ = [(name, c_uint64) for name in ("records", "contributing", "operations", "events", "unkeyed_insertions", "shift_capped", "runs", "candidates", "sites", "reported", "peak_bytes")] + [("seconds", ctypes.c_double * 5)]


class RealignStats(ctypes.Structure):
    """agpu_realign_stats: what agpu_realign_end / ahost_realign_split_of count"""
    _fields_ = [(name, c_uint64) for name in ("records", "templates", "realign_templates", "kept_templates", "dropped_secondary", "extra", "orphans", "placeholder_cigar", "realign_bytes", "kept_bytes")] + [
        ("layout", c_uint32), ("reserved", c_uint32), ("peak_bytes", c_uint64), ("seconds", ctypes.c_double * 4)]


class RegionTrack(ctypes.Structure):
    """agpu_region_track: the annotation and the rRNA intervals as runs of bases, per contig (ahost_region_track)"""
    _fields_ = [("id", c_uint64), ("n_contigs", c_uint32), ("contig_offset", c_void_p), ("n_runs", c_uint32), ("run_start", c_void_p), ("run_bits", c_void_p), ("run_gene", c_void_p), ("run_rank", c_void_p),
                ("n_genes", c_uint32), ("gene_body", c_void_p)]


class RegionTrackInfo(ctypes.Structure):
    """ahost_region_track_info"""
    _fields_ = [("n_contigs", c_uint32), ("runs", c_uint64), ("intervals", c_uint64), ("intervals_unknown_contig", c_uint64), ("bytes", c_uint64)]


class RnaMetricsStats(ctypes.Structure):
    """agpu_rna_metrics_stats: what agpu_rna_metrics / ahost_rna_metrics_of count"""
    _fields_ = [(name, c_uint64) for name in ("records", "base_records", "blocks", "segments", "track_runs", "peak_bytes")] + [("seconds", ctypes.c_double * 1)]


RNA_METRICS_SCALARS, RNA_METRICS_WORDS = 34, 1394  # AGPU_RNA_METRICS_SCALARS, AGPU_RNA_METRICS_WORDS


class RealignInfo(ctypes.Structure):
    """agpu_realign_info: what agpu_realign_begin tells"""
    _fields_ = [("window_bytes", c_uint64), ("realign_bytes", c_uint64), ("kept_bytes", c_uint64), ("layout", c_uint32), ("reserved", c_uint32)]


class RealignPlan(ctypes.Structure):
    """ahost_realign_plan: the references of a header against the assembly, and the header of the file of the kept templates"""
    _fields_ = [("n_ref", c_uint32), ("in_assembly", c_void_p), ("header", c_void_p), ("header_bytes", c_uint64)]


class DepthContigs(ctypes.Structure):
    """ahost_depth_contigs: the contigs of a header"""
    _fields_ = [("n_ref", c_uint32), ("length", c_void_p), ("names", c_void_p), ("name_offset", c_void_p)]


class BamPiece(ctypes.Structure):
    """ahost_bam_piece: stored_bgzf is the KIND of the piece -- 0 stream bytes, 1 stored BGZF, 2 deflated BGZF, 3 lines of SAM text (first_line: the number of its first line)"""
    _fields_ = [("stored_bgzf", c_int), ("bytes", c_size_t), ("stream_bytes", c_size_t), ("n_blocks", c_uint32), ("first_line", c_uint64)]


PIECE_STREAM, PIECE_STORED_BGZF, PIECE_DEFLATED_BGZF, PIECE_SAM_TEXT = 0, 1, 2, 3


class BatchRows(ctypes.Structure):
    _fields_ = [("n", c_uint64), ("n_aln", c_void_p), ("fbits", c_void_p), ("group", c_void_p),
                ("contig", c_void_p * 3), ("start", c_void_p * 3), ("end", c_void_p * 3), ("abits", c_void_p * 3), ("cigar_offset", c_void_p * 3), ("cigar_count", c_void_p * 3),
                ("cigar_pool_size", c_uint64), ("cigar_pool", c_void_p), ("seq_offset", c_void_p * 2), ("seq_length", c_void_p * 2), ("seq_pool_size", c_uint64), ("seq_pool", c_void_p),
                ("name_offset", c_void_p), ("names_size", c_uint64), ("names", c_void_p)]


class Params(ctypes.Structure):
    _fields_ = [("homopolymer_length", c_uint32), ("min_read_through_distance", c_uint32), ("max_itd_length", c_uint32), ("subsampling_threshold", c_uint32),
                ("mismatch_pvalue_cutoff", c_float), ("max_kmer_content", c_float), ("evalue_cutoff", c_float), ("max_mismapper_fraction", c_float),
                ("fragment_length", c_uint32), ("external_duplicate_marking", c_uint8), ("strandedness", c_uint8), ("filter_enabled", c_uint8 * FILTER_COUNT),
                ("exonic_fraction", c_float), ("min_support", c_uint32)]


def _load(path):
    if not os.path.exists(path):
        raise ImportError(
            "%s is missing: the MI355X hot path has no CPU fallback. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950)." % path)
    return ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)


def bind_device_api(lib, prefix="agpu_"):
    """Declare the argument types of the device C ABI on `lib` and return a namespace of its functions."""
    class Api(object):
        pass
    api = Api()
    ctx = c_void_p
    signatures = {
        "last_error": (c_char_p, []),
        "api_version": (c_int, []),
        "device_count": (c_int, []),
        "default_params": (None, [POINTER(Params)]),
        "create": (ctx, [c_int, POINTER(Params)]),
        "destroy": (None, [ctx]),
        "set_params": (c_int, [ctx, POINTER(Params)]),
        "upload_annotation": (c_int, [ctx, POINTER(AnnotationView)]),
        "upload_genome": (c_int, [ctx, POINTER(GenomeView)]),
        "upload_batch": (c_int, [ctx, POINTER(BatchView)]),
        "reset": (c_int, [ctx]),
        "mark_multimappers": (c_int, [ctx, POINTER(c_uint64)]),
        "annotate": (c_int, [ctx, POINTER(c_uint32)]),
        "read_filters_stage1": (c_int, [ctx, c_void_p, c_void_p]),
        "get_viral_integration_sites": (c_int, [ctx, c_void_p, c_uint64, POINTER(c_uint64)]),
        "fragment_length_samples": (c_int, [ctx, c_void_p, POINTER(c_uint32), POINTER(c_uint64)]),
        "read_filters_stage2": (c_int, [ctx, c_void_p]),
        "find_fusions": (c_int, [ctx, c_int32, POINTER(c_uint64)]),
        "get_candidates": (c_int, [ctx] + [c_void_p] * 13),
        "get_candidate_read_lists": (c_int, [ctx, c_void_p, c_uint64, POINTER(c_uint64)]),
        "get_candidate_read_lists_of": (c_int, [ctx, c_void_p, c_uint64, c_void_p, c_void_p, c_uint64, POINTER(c_uint64)]),
        "get_discordant_swapped": (c_int, [ctx, c_void_p]),
        "shard_merge_rccl": (c_int, [ctx, c_void_p, c_uint32, POINTER(IngestResult)]),
        "filter_mismappers_rccl": (c_int, [ctx, c_void_p, c_int32, c_uint32, c_uint32, POINTER(c_uint64), POINTER(c_uint64)]),
        "rccl_unique_id": (c_int, [c_void_p]),
        "rccl_join": (c_int, [ctx, c_void_p, c_uint32, c_uint32, POINTER(c_void_p)]),
        "rccl_leave": (c_int, [c_void_p]),
        "rccl_all_gather_host": (c_int, [ctx, c_void_p, c_uint32, c_void_p, c_void_p, c_uint64]),
        "rccl_all_reduce_host": (c_int, [ctx, c_void_p, c_void_p, c_uint64, c_int]),
        "get_filters": (c_int, [ctx, c_void_p]),
        "get_filters_of": (c_int, [ctx, c_void_p, c_uint64, c_void_p]),
        "select_candidates": (c_int, [ctx, c_int, POINTER(c_uint64)]),
        "get_selected_candidates": (c_int, [ctx, POINTER(SelectedCandidates)]),
        "get_alignment_bits": (c_int, [ctx, c_int, c_void_p]),
        "get_fragment_bits": (c_int, [ctx, c_void_p]),
        "get_gene_sets": (c_int, [ctx, c_int, c_void_p, c_void_p, c_uint64, POINTER(c_uint64)]),
        "get_gene_table": (c_int, [ctx, c_uint32, c_uint32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
        "get_fusion_stats": (c_int, [ctx, c_void_p]),
        "set_shard": (c_int, [ctx, c_uint64, c_uint64]),
        "annotate_begin": (c_int, [ctx, POINTER(c_uint64)]),
        "copy_unmapped_positions": (c_int, [ctx, c_void_p]),
        "annotate_finish": (c_int, [ctx, c_void_p, c_uint64, POINTER(c_uint32)]),
        "duplicates_begin": (c_int, [ctx, POINTER(c_uint64)]),
        "copy_duplicate_entries": (c_int, [ctx, c_void_p]),
        "read_filters_stage1_global": (c_int, [ctx, c_void_p, c_uint64, c_void_p, c_void_p]),
        "fragment_length_samples_limited": (c_int, [ctx, c_uint32, c_void_p, POINTER(c_uint32), POINTER(c_uint64)]),
        "build_emissions": (c_int, [ctx, c_uint32, c_void_p]),
        "copy_emissions": (c_int, [ctx, c_void_p]),
        "find_fusions_from_emissions": (c_int, [ctx, c_void_p, c_uint64, c_int32, POINTER(c_uint64)]),
        "get_candidate_first_occurrence": (c_int, [ctx, c_void_p]),
        "import_candidates": (c_int, [ctx, c_uint64] + [c_void_p] * 12),
        "set_read_filters": (c_int, [ctx, c_void_p]),
        "make_kmer_index": (c_int, [ctx, c_int32, POINTER(c_uint64)]),
        "filter_mismappers": (c_int, [ctx, c_int32, POINTER(c_uint64), POINTER(c_uint64)]),
        "candidate_iteration_order": (c_int, [ctx, c_void_p]),
        "merge_adjacent_fusions": (c_int, [ctx, c_int32, POINTER(c_uint64)]),
        "filter_multimappers": (c_int, [ctx, POINTER(c_uint64), POINTER(c_uint64)]),
        "upload_coverage": (c_int, [ctx, POINTER(CoverageView)]),
        "recover_internal_tandem_duplication": (c_int, [ctx, c_uint32, c_float, POINTER(c_uint64)]),
        "filter_both_intronic": (c_int, [ctx, POINTER(c_uint64)]),
        "filter_short_anchor": (c_int, [ctx, c_uint32, POINTER(c_uint64)]),
        "filter_end_to_end": (c_int, [ctx, POINTER(c_uint64)]),
        "filter_no_coverage": (c_int, [ctx, POINTER(c_uint64)]),
        "filter_marginal_read_through": (c_int, [ctx, POINTER(c_uint64)]),
        "select_most_supported_breakpoints": (c_int, [ctx, POINTER(c_uint64)]),
        "recover_many_spliced": (c_int, [ctx, c_uint32, POINTER(c_uint64)]),
        "filter_in_vitro": (c_int, [ctx, c_float, POINTER(c_uint64)]),
        "filter_homologs": (c_int, [ctx, c_float, POINTER(c_uint64)]),
        "recover_isoforms": (c_int, [ctx, POINTER(c_uint64)]),
        "mark_genomic_support": (c_int, [ctx, POINTER(GenomicBreakpoint), c_uint32, c_int32, POINTER(c_uint64)]),
        "get_genomic_support": (c_int, [ctx, c_void_p, c_void_p]),
        "filter_no_genomic_support": (c_int, [ctx, POINTER(c_uint64)]),
        "recover_genomic_support": (c_int, [ctx, POINTER(c_uint64)]),
        "filter_blacklisted_ranges": (c_int, [ctx, POINTER(RangeRule), c_uint32, c_float, c_int32, POINTER(c_uint64)]),
        "recover_known_fusions": (c_int, [ctx, POINTER(RangeRule), c_uint32, c_int32, POINTER(c_uint64)]),
        "assign_confidence": (c_int, [ctx, c_void_p]),
        "recover_both_spliced": (c_int, [ctx, c_uint32, c_float, c_int32, c_uint32, POINTER(c_uint64)]),
        "set_owned_candidates": (c_int, [ctx, c_void_p, c_uint64]),
        "copy_multimapper_flags": (c_int, [ctx, c_void_p]),
        "multimappers_begin": (c_int, [ctx, c_void_p, POINTER(c_uint64)]),
        "multimappers_partial_best": (c_int, [ctx, c_void_p]),
        "multimappers_resolve": (c_int, [ctx, c_void_p, c_void_p, POINTER(c_uint64)]),
        "multimappers_recount": (c_int, [ctx, c_void_p, c_void_p]),
        "multimappers_finish": (c_int, [ctx, c_void_p, POINTER(c_uint64)]),
        "set_candidate_state": (c_int, [ctx, c_void_p, c_void_p, c_void_p, c_void_p]),
        "estimate_expected_fusions": (c_int, [ctx, c_uint64, c_void_p]),
        "get_evalues": (c_int, [ctx, c_void_p]),
        "filter_candidate_predicates": (c_int, [ctx, c_void_p]),
        "filter_relative_support": (c_int, [ctx, POINTER(c_uint64)]),
        "host_alloc": (c_void_p, [c_size_t]),
        "host_free": (None, [c_void_p]),
        "ingest_begin": (c_int, [ctx, POINTER(IngestConfig)]),
        "ingest_push": (c_int, [ctx, c_void_p, c_size_t]),
        "ingest_push_bgzf": (c_int, [ctx, c_void_p, c_size_t, POINTER(BgzfBlock), c_uint32, c_size_t]),
        "ingest_sam_targets": (c_int, [ctx, c_void_p, c_void_p, c_uint32]),
        "ingest_push_sam": (c_int, [ctx, c_void_p, c_size_t, c_uint64]),
        "sam_transcode": (c_int, [ctx, c_void_p, c_size_t, c_void_p, c_void_p, c_uint32, c_void_p, c_size_t, POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64)]),
        "bgzf_unpack": (c_int, [ctx, c_void_p, c_size_t, POINTER(BgzfBlock), c_uint32, c_int, c_void_p, c_size_t, c_void_p, POINTER(c_uint32), POINTER(c_uint32)]),
        "ingest_finish": (c_int, [ctx, POINTER(IngestResult)]),
        "separate_adopt": (c_int, [ctx]),
        "separate_merge": (c_int, [ctx, POINTER(IngestResult)]),
        "sorted_bam_begin": (c_int, [ctx, POINTER(SortedBamInfo)]),
        "sorted_bam_next": (c_int, [ctx, c_void_p, c_uint64, POINTER(c_uint64)]),
        "sorted_bam_index": (c_int, [ctx, c_uint64, c_void_p, c_uint32, POINTER(SortedBamIndex)]),
        "sorted_bam_end": (c_int, [ctx]),
        "sorted_bam_set_compression": (c_int, [ctx, c_int]),
        "sorted_bam_compressed_bytes": (c_int, [ctx, POINTER(c_uint64)]),
        "sorted_bam_compression_allocated_bytes": (c_int, [ctx, POINTER(c_uint64)]),
        "support_pool_build": (c_int, [ctx, c_void_p, c_void_p, c_uint64, POINTER(SupportPoolInfo)]),
        "supporting_begin": (c_int, [ctx, POINTER(SupportingRows), ctypes.c_int64, POINTER(SupportingInfo)]),
        "supporting_row_bytes": (c_int, [ctx, c_void_p]),
        "supporting_next": (c_int, [ctx, c_void_p, c_uint64, POINTER(c_uint64)]),
        "supporting_index": (c_int, [ctx, c_uint64, POINTER(SupportingIndex)]),
        "supporting_end": (c_int, [ctx]),
        "support_pool_release": (c_int, [ctx]),
        "support_allocated_bytes": (c_int, [ctx, POINTER(c_uint64)]),
        "virus_expression": (c_int, [ctx, c_void_p, c_void_p, c_uint32, c_uint32, POINTER(VirusCounters)]),
        "virus_allocated_bytes": (c_int, [ctx, POINTER(c_uint64)]),
        "depth_begin": (c_int, [ctx, c_void_p, c_void_p, c_void_p, c_uint32, POINTER(DepthInfo)]),
        "depth_next": (c_int, [ctx, c_void_p, c_uint64, POINTER(c_uint64)]),
        "depth_end": (c_int, [ctx, POINTER(DepthStats)]),
        "depth_allocated_bytes": (c_int, [ctx, POINTER(c_uint64)]),
        "sorted_bam_set_mark_duplicates": (c_int, [ctx, c_int]),
        "markdup_stats": (c_int, [ctx, POINTER(MarkdupCounts)]),
        "markdup_allocated_bytes": (c_int, [ctx, POINTER(c_uint64)]),
        "gene_counts": (c_int, [ctx, c_void_p, c_uint32, c_void_p, POINTER(GeneCountStats)]),
        "gene_counts_allocated_bytes": (c_int, [ctx, POINTER(c_uint64)]),
        "splice_junctions": (c_int, [ctx, c_void_p, c_uint32, POINTER(POINTER(JunctionRow)), POINTER(c_uint64), POINTER(JunctionStats)]),
        "splice_junctions_allocated_bytes": (c_int, [ctx, POINTER(c_uint64)]),
        "allele_counts": (c_int, [ctx, POINTER(AlleleSite), c_uint64, c_void_p, c_uint32, c_uint32, c_uint32, POINTER(POINTER(AlleleRow)), POINTER(AlleleStats)]),
        "allele_counts_allocated_bytes": (c_int, [ctx, POINTER(c_uint64)]),
        "variant_sites": (c_int, [ctx, c_void_p, c_uint32, c_uint32, c_uint32, c_uint32, c_uint32, POINTER(POINTER(VariantRow)), POINTER(c_uint64), POINTER(VariantStats)]),
        "variant_sites_allocated_bytes": (c_int, [ctx, POINTER(c_uint64)]),
        "indel_sites": (c_int, [ctx, c_void_p, c_uint32, c_uint32, c_uint32, c_uint32, POINTER(POINTER(IndelRow)), POINTER(c_uint64), POINTER(IndelStats)]),
        "indel_sites_allocated_bytes": (c_int, [ctx, POINTER(c_uint64)]),
        "realign_begin": (c_int, [ctx, c_void_p, c_void_p, c_void_p, c_uint32, c_int, POINTER(RealignInfo)]),
        "realign_next": (c_int, [ctx, c_int, c_void_p, c_uint64, POINTER(c_uint64)]),
        "realign_end": (c_int, [ctx, POINTER(RealignStats)]),
        "realign_allocated_bytes": (c_int, [ctx, POINTER(c_uint64)]),
        "rna_metrics": (c_int, [ctx, POINTER(RegionTrack), c_void_p, c_uint32, c_void_p, POINTER(RnaMetricsStats)]),
        "rna_metrics_allocated_bytes": (c_int, [ctx, POINTER(c_uint64)]),
        "shard_export_size": (c_int, [ctx, POINTER(c_uint64)]),
        "shard_export": (c_int, [ctx, c_void_p, c_uint64]),
        "shard_merge": (c_int, [ctx, c_void_p, c_uint64, c_uint32, POINTER(IngestResult)]),
        "mismapper_jobs": (c_int, [ctx, POINTER(c_uint64)]),
        "mismapper_verdicts": (c_int, [ctx, c_int32, c_uint32, c_uint32, c_void_p]),
        "filter_mismappers_apply": (c_int, [ctx, c_void_p, POINTER(c_uint64), POINTER(c_uint64)]),
        "get_viral_read_counts": (c_int, [ctx, c_void_p]),
        "get_coverage": (c_int, [ctx, c_void_p, c_void_p, c_void_p]),
        "detect_strandedness": (c_int, [ctx, POINTER(c_int)]),
        "get_read_lengths": (c_int, [ctx, c_uint64, c_uint64, c_void_p, c_void_p]),
        "gather_rows_begin": (c_int, [ctx, c_void_p, c_uint64, POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64)]),
        "gather_rows_copy": (c_int, [ctx, POINTER(BatchRows)]),
        "set_profiling": (c_int, [ctx, c_int]),
        "debug_fail_allocation_in_finish": (None, [c_int]),
        "keep_batch_buffers": (c_int, [ctx, c_int]),
        "get_kernel_profile": (c_int, [ctx, c_void_p, c_void_p, c_void_p, c_uint32, POINTER(c_uint32)]),
        "last_kernel_ms": (c_int, [ctx, POINTER(c_float)]),
        "last_kernel_bytes": (c_int, [ctx, POINTER(c_uint64)]),
    }
    for name, (restype, argtypes) in signatures.items():
        function = getattr(lib, prefix + name, None)
        if function is None:
            continue
        function.restype = restype
        function.argtypes = argtypes
        setattr(api, name, function)
    api.exported = sorted(name for name in signatures if hasattr(api, name))
    api.declared = sorted(signatures)
    return api


def bind_host_api(lib):
    session = c_void_p
    signatures = {
        "ahost_last_error": (c_char_p, []),
        "ahost_open": (session, [c_char_p, c_char_p, c_char_p, c_char_p, c_char_p]),
        "ahost_close": (None, [session]),
        "ahost_ingest_bam_file": (c_int, [session, c_char_p, c_int, ctypes.c_uint]),
        "ahost_ingest_bam_memory": (c_int, [session, c_void_p, c_size_t, c_int, ctypes.c_uint]),
        "ahost_ingest_separate": (c_int, [session, c_char_p, c_char_p, c_int, ctypes.c_uint, POINTER(c_uint64), POINTER(c_uint64)]),
        "ahost_bam_open_role": (c_int, [session, c_char_p, c_int, ctypes.c_uint, c_int, POINTER(IngestConfig)]),
        "ahost_save_ingest": (c_int, [session, c_char_p]),
        "ahost_load_ingest": (c_int, [session, c_char_p]),
        "ahost_annotation_view": (POINTER(AnnotationView), [session]),
        "ahost_genome_view": (POINTER(GenomeView), [session]),
        "ahost_batch_view": (POINTER(BatchView), [session]),
        "ahost_fragment_count": (c_uint64, [session]),
        "ahost_mapped_reads": (c_uint64, [session]),
        "ahost_viral_read_total": (c_uint64, [session]),
        "ahost_coverage_checksum": (c_uint64, [session]),
        "ahost_coverage_view": (POINTER(CoverageView), [session]),
        "ahost_write_fusions": (c_int, [session, POINTER(FusionTable), c_char_p, c_int, c_int, c_uint32, c_int, c_int]),
        "ahost_detach_sample": (c_void_p, [session]),
        "ahost_write_fusions_of": (c_int, [c_void_p, POINTER(FusionTable), c_char_p, c_int, c_int, c_uint32, c_int, c_int]),
        "ahost_release_sample": (None, [c_void_p]),
        "ahost_format_fusions": (c_int, [session, POINTER(FusionTable), c_int, c_int, c_uint32, c_int, c_int, c_uint32, c_uint32, POINTER(c_void_p), POINTER(c_uint64)]),
        "ahost_load_tags": (c_int, [session, c_char_p]),
        "ahost_load_genomic_breakpoints": (c_int, [session, c_char_p, POINTER(POINTER(GenomicBreakpoint)), POINTER(c_uint32)]),
        "ahost_load_protein_domains": (c_int, [session, c_char_p]),
        "ahost_load_range_rules": (c_int, [session, c_char_p, c_int, POINTER(POINTER(RangeRule)), POINTER(c_uint32)]),
        "ahost_contig_count": (c_uint32, [session]),
        "ahost_contig_name": (c_char_p, [session, c_uint32]),
        "ahost_fragment_name": (c_void_p, [session, c_uint64, POINTER(c_uint32)]),
        "ahost_detect_strandedness": (c_int, [session]),
        "ahost_viral_verdicts": (c_int, [session, c_void_p, c_uint64, c_void_p, c_uint32, ctypes.c_uint, c_float, c_void_p, c_void_p]),
        "ahost_read_length_sum": (c_float, [session, c_float, c_uint64, c_uint64]),
        "ahost_shard_boundary": (c_uint64, [session, c_uint64]),
        "ahost_batch_slice_view": (POINTER(BatchView), [session, c_uint64, c_uint64]),
        "ahost_estimate_fragment_length_from_sums": (c_int, [c_void_p, c_uint32, c_float, c_uint64, ctypes.c_uint, POINTER(c_float), POINTER(c_float), POINTER(c_float), POINTER(c_int32)]),
        "ahost_candidate_iteration_order": (c_int, [c_uint64] + [c_void_p] * 7),
        "ahost_bam_open": (c_int, [session, c_char_p, c_int, ctypes.c_uint, POINTER(IngestConfig)]),
        "ahost_bam_open_part": (c_int, [session, c_char_p, c_int, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, POINTER(IngestConfig)]),
        "ahost_bam_next": (c_int, [session, c_void_p, c_size_t, POINTER(BgzfBlock), c_uint32, POINTER(BamPiece)]),
        "ahost_bam_close": (None, [session]),
        "ahost_bam_sam_targets": (c_int, [session, POINTER(c_void_p), POINTER(c_void_p), POINTER(c_uint32)]),
        "ahost_sam_transcode": (c_int, [c_void_p, c_size_t, c_void_p, c_void_p, c_uint32, c_void_p, c_size_t, POINTER(c_uint64), POINTER(c_uint64), POINTER(c_uint64)]),
        "ahost_adopt_device_ingest": (c_int, [session, POINTER(IngestResult), c_void_p, c_void_p, c_void_p, c_void_p]),
        "ahost_sorted_bam_header": (c_int, [session, POINTER(c_void_p), POINTER(c_uint64), POINTER(c_void_p), POINTER(c_uint32)]),
        "ahost_sorted_bam_header_of": (c_int, [c_void_p, c_size_t, POINTER(c_void_p), POINTER(c_uint64), POINTER(c_void_p), POINTER(c_uint32)]),
        "ahost_sorted_bam": (c_int, [c_void_p, c_size_t, c_uint64, c_void_p, c_uint32, POINTER(c_void_p), POINTER(SortedBamInfo), POINTER(SortedBamIndex)]),
        "ahost_sorted_bam_write_index": (c_int, [POINTER(SortedBamIndex), c_char_p]),
        "ahost_sorted_bam_eof": (None, [c_void_p]),
        "ahost_sorted_bam_file": (c_int, [c_char_p, c_char_p, POINTER(SortedBamInfo)]),
        "ahost_sorted_bam_write": (c_int, [c_void_p, c_size_t, c_void_p, c_size_t, c_char_p, POINTER(SortedBamInfo)]),
        "ahost_sorted_bam_level": (c_int, [c_void_p, c_size_t, c_uint64, c_void_p, c_uint32, c_int, POINTER(c_void_p), POINTER(SortedBamInfo), POINTER(SortedBamIndex)]),
        "ahost_sorted_bam_file_level": (c_int, [c_char_p, c_char_p, c_int, POINTER(SortedBamInfo)]),
        "ahost_sorted_bam_write_level": (c_int, [c_void_p, c_size_t, c_void_p, c_size_t, c_char_p, c_int, POINTER(SortedBamInfo)]),
        "ahost_written_fusion_rows": (c_int, [session, POINTER(c_uint32), POINTER(c_void_p), POINTER(c_void_p), POINTER(c_void_p)]),
        "ahost_supporting_writer_open": (c_void_p, [c_char_p, c_void_p, c_uint64, c_uint32, c_void_p]),
        "ahost_supporting_writer_push": (c_int, [c_void_p, c_void_p, c_uint64]),
        "ahost_supporting_writer_index": (c_int, [c_void_p, POINTER(SupportingIndex), c_void_p, c_uint32]),
        "ahost_supporting_writer_close": (c_int, [c_void_p, c_int]),
        "ahost_supporting_alignments": (c_int, [c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_void_p, c_uint64, POINTER(SupportingRows), ctypes.c_int64, c_char_p, POINTER(SupportingInfo)]),
        "ahost_supporting_alignments_file": (c_int, [session, c_void_p, c_char_p, ctypes.c_int64, c_char_p, POINTER(SupportingInfo)]),
        "ahost_virus_contigs_of_session": (c_int, [session, POINTER(VirusContigs)]),
        "ahost_virus_contigs_of": (c_int, [c_void_p, c_size_t, c_char_p, POINTER(VirusContigs)]),
        "ahost_virus_expression": (c_int, [c_void_p, c_size_t, POINTER(VirusContigs), POINTER(VirusCounters)]),
        "ahost_virus_expression_table": (c_int, [POINTER(VirusCounters), POINTER(VirusContigs), POINTER(c_void_p), POINTER(c_uint64)]),
        "ahost_virus_expression_write": (c_int, [POINTER(VirusCounters), POINTER(VirusContigs), c_char_p]),
        "ahost_virus_expression_file": (c_int, [session, c_char_p, c_char_p]),
        "ahost_depth_contigs_of_session": (c_int, [session, POINTER(DepthContigs)]),
        "ahost_depth_contigs_of": (c_int, [c_void_p, c_size_t, POINTER(DepthContigs)]),
        "ahost_depth_track": (c_int, [c_void_p, c_size_t, POINTER(DepthContigs), POINTER(c_void_p), POINTER(c_uint64), POINTER(DepthStats)]),
        "ahost_depth_line": (c_int, [c_char_p, c_uint32, c_uint32, c_uint32, c_void_p, c_uint32, POINTER(c_uint32)]),
        "ahost_depth_write": (c_int, [c_void_p, c_uint64, c_char_p]),
        "ahost_depth_file": (c_int, [c_char_p, c_char_p, POINTER(DepthStats)]),
        "ahost_markdup": (c_int, [c_void_p, c_size_t, c_void_p, c_uint64, POINTER(MarkdupCounts)]),
        "ahost_sorted_bam_file_marked": (c_int, [c_char_p, c_char_p, c_int, c_int, POINTER(SortedBamInfo)]),
        "ahost_sorted_bam_file_marked_counts": (c_int, [c_char_p, c_char_p, c_int, c_int, POINTER(SortedBamInfo), POINTER(MarkdupCounts)]),
        "ahost_gene_counts_genes": (c_int, [session, POINTER(c_uint32), POINTER(c_void_p), POINTER(c_uint64)]),
        "ahost_gene_counts_of": (c_int, [session, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_uint64, POINTER(GeneCountStats)]),
        "ahost_gene_counts_text": (c_int, [session, c_void_p, c_uint64, POINTER(c_void_p), POINTER(c_uint64)]),
        "ahost_gene_counts_write": (c_int, [session, c_void_p, c_uint64, c_char_p]),
        "ahost_gene_counts_file": (c_int, [session, c_char_p, c_char_p, POINTER(GeneCountStats)]),
        "ahost_splice_junctions_of": (c_int, [session, c_void_p, c_size_t, c_void_p, c_size_t, POINTER(POINTER(JunctionRow)), POINTER(c_uint64), POINTER(JunctionStats)]),
        "ahost_splice_junctions_text": (c_int, [POINTER(DepthContigs), POINTER(JunctionRow), c_uint64, POINTER(c_void_p), POINTER(c_uint64)]),
        "ahost_splice_junctions_write": (c_int, [POINTER(DepthContigs), POINTER(JunctionRow), c_uint64, c_char_p]),
        "ahost_splice_junctions_file": (c_int, [session, c_char_p, c_char_p, POINTER(JunctionStats)]),
        "ahost_allele_sites_load": (c_int, [c_char_p, c_void_p, c_size_t, POINTER(AlleleSites)]),
        "ahost_allele_sites_place_session": (c_int, [session, POINTER(AlleleSites)]),
        "ahost_allele_sites_free": (None, [POINTER(AlleleSites)]),
        "ahost_allele_counts_of": (c_int, [session, c_void_p, c_size_t, c_void_p, c_size_t, POINTER(AlleleSites), c_uint32, c_uint32, POINTER(POINTER(AlleleRow)), POINTER(AlleleStats)]),
        "ahost_allele_counts_text": (c_int, [POINTER(AlleleSites), POINTER(AlleleRow), c_uint64, POINTER(c_void_p), POINTER(c_uint64)]),
        "ahost_allele_counts_write": (c_int, [POINTER(AlleleSites), POINTER(AlleleRow), c_uint64, c_char_p]),
        "ahost_allele_counts_file": (c_int, [session, c_char_p, c_char_p, c_char_p, c_uint32, c_uint32, POINTER(AlleleStats)]),
        "ahost_variant_sites_of": (c_int, [session, c_void_p, c_size_t, c_void_p, c_size_t, c_uint32, c_uint32, c_uint32, c_uint32, POINTER(POINTER(VariantRow)), POINTER(c_uint64), POINTER(VariantStats)]),
        "ahost_variant_sites_text": (c_int, [POINTER(DepthContigs), POINTER(VariantRow), c_uint64, POINTER(c_void_p), POINTER(c_uint64)]),
        "ahost_variant_sites_write": (c_int, [POINTER(DepthContigs), POINTER(VariantRow), c_uint64, c_char_p]),
        "ahost_variant_sites_file": (c_int, [session, c_char_p, c_char_p, c_uint32, c_uint32, c_uint32, c_uint32, POINTER(VariantStats)]),
        "ahost_indel_sites_of": (c_int, [session, c_void_p, c_size_t, c_void_p, c_size_t, c_uint32, c_uint32, c_uint32, POINTER(POINTER(IndelRow)), POINTER(c_uint64), POINTER(IndelStats)]),
        "ahost_indel_sites_text": (c_int, [session, POINTER(DepthContigs), POINTER(IndelRow), c_uint64, POINTER(c_void_p), POINTER(c_uint64)]),
        "ahost_indel_sites_write": (c_int, [session, POINTER(DepthContigs), POINTER(IndelRow), c_uint64, c_char_p]),
        "ahost_indel_sites_file": (c_int, [session, c_char_p, c_char_p, c_uint32, c_uint32, c_uint32, POINTER(IndelStats)]),
        "ahost_realign_plan_of": (c_int, [session, c_void_p, c_size_t, POINTER(RealignPlan)]),
        "ahost_realign_plan_of_session": (c_int, [session, POINTER(RealignPlan)]),
        "ahost_realign_split_of": (c_int, [session, c_void_p, c_size_t, c_void_p, c_size_t, c_int, POINTER(c_void_p), POINTER(c_uint64), POINTER(c_void_p), POINTER(c_uint64), POINTER(RealignStats)]),
        "ahost_realign_split_file": (c_int, [session, c_char_p, c_char_p, c_char_p, POINTER(RealignStats)]),
        "ahost_rrna_intervals_load": (c_int, [c_char_p, POINTER(c_uint64)]),
        "ahost_region_track": (c_int, [session, c_char_p, POINTER(RegionTrack), POINTER(RegionTrackInfo)]),
        "ahost_rna_metrics_of": (c_int, [session, c_char_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, c_uint64, POINTER(RnaMetricsStats)]),
        "ahost_rna_metrics_text": (c_int, [c_void_p, c_uint64, POINTER(c_void_p), POINTER(c_uint64)]),
        "ahost_rna_metrics_write": (c_int, [c_void_p, c_uint64, c_char_p]),
        "ahost_rna_metrics_file": (c_int, [session, c_char_p, c_char_p, c_char_p, POINTER(RnaMetricsStats)]),
        "ahost_set_batch_rows": (c_int, [session, POINTER(BatchRows), c_void_p]),
        "ahost_fusion_table_reads": (c_int, [POINTER(FusionTable), c_int, c_void_p, c_uint64, POINTER(c_uint64)]),
        "ahost_read_length_sum_of": (c_float, [c_float, c_void_p, c_void_p, c_uint64]),
        "ahost_estimate_fragment_length": (c_int, [session, c_void_p, c_uint32, c_uint64, ctypes.c_uint, POINTER(c_float), POINTER(c_float), POINTER(c_float), POINTER(c_int32)]),
    }
    for name, (restype, argtypes) in signatures.items():
        function = getattr(lib, name)
        function.restype = restype
        function.argtypes = argtypes
    return lib


_device_lib = None
_host_lib = None


class WorkflowOptions(ctypes.Structure):
    """arriba_workflow_options (include/arriba_workflow.h): options_t of the reference (source/options.hpp)"""
    _fields_ = [(name, c_char_p) for name in ("assembly_file", "gene_annotation_file", "chimeric_bam_file", "output_file", "discarded_output_file", "blacklist_file", "known_fusions_file", "tags_file",
                                              "protein_domains_file", "genomic_breakpoints_file", "interesting_contigs", "viral_contigs", "gtf_features")] + [
        ("device", Params), ("min_itd_support", c_uint32), ("min_itd_allele_fraction", c_float), ("high_expression_quantile", c_float), ("min_spliced_events", c_uint32), ("min_anchor_length", c_uint32),
        ("max_homolog_identity", c_float), ("top_viral_contigs", c_uint32), ("viral_contig_min_covered_fraction", c_float), ("max_genomic_breakpoint_distance", c_int32),
        ("print_extra_info_for_discarded_fusions", c_uint8), ("fill_sequence_gaps", c_uint8), ("device_index", c_int), ("log_to_stdout", c_uint8), ("host_ingest", c_uint8), ("sorted_bam_file", c_char_p), ("supporting_alignments_prefix", c_char_p), ("supporting_alignments_window", ctypes.c_int64), ("sorted_bam_compression", c_int), ("virus_expression_file", c_char_p), ("coverage_file", c_char_p), ("mark_duplicates", c_int), ("gene_counts_file", c_char_p), ("splice_junctions_file", c_char_p), ("allele_sites_file", c_char_p), ("allele_counts_file", c_char_p), ("allele_min_mapq", c_uint32), ("allele_min_baseq", c_uint32), ("realign_reads_file", c_char_p), ("realign_kept_file", c_char_p), ("rna_metrics_file", c_char_p), ("rrna_intervals_file", c_char_p), ("separate_chimeric_file", c_char_p), ("variant_sites_file", c_char_p), ("variant_min_alt", c_uint32), ("variant_min_percent", c_uint32), ("variant_min_mapq", c_uint32), ("variant_min_baseq", c_uint32), ("indel_sites_file", c_char_p), ("indel_min_alt", c_uint32), ("indel_min_percent", c_uint32), ("indel_min_mapq", c_uint32)]


class WorkflowStage(ctypes.Structure):
    _fields_ = [("stage", ctypes.c_char * 48), ("count", c_uint64)]


class WorkflowReport(ctypes.Structure):
    _fields_ = [("n_stages", c_uint32), ("stages", WorkflowStage * 64)]


class WorkflowTiming(ctypes.Structure):
    _fields_ = [(name, ctypes.c_double) for name in ("total", "feed", "ingest", "adopt", "stages", "filter_mismappers", "output", "output_results", "output_rows", "output_format", "feed_read", "feed_push", "feed_total", "exchange_parts", "exchange_verdicts", "exchange_rows", "shard_fragments", "exchanged_bytes", "sorted_bam", "supporting_alignments", "virus_expression", "coverage", "gene_counts", "splice_junctions", "allele_counts", "realign", "rna_metrics", "variant_sites", "indel_sites")]


WORKFLOW_MAX, WORKFLOW_MIN, WORKFLOW_SUM = 0, 1, 2
RCCL_ID_BYTES = 128
ALL_GATHER = ctypes.CFUNCTYPE(c_int, c_void_p, c_void_p, c_void_p, c_uint64)
ALL_REDUCE_INT64 = ctypes.CFUNCTYPE(c_int, c_void_p, c_void_p, c_uint64, c_int)
ALL_REDUCE_MAX_BYTES = ctypes.CFUNCTYPE(c_int, c_void_p, c_void_p, c_uint64)


class WorkflowCommunicator(ctypes.Structure):
    """arriba_workflow_communicator (include/arriba_workflow.h): the ranks of one sample and the three collectives over host memory the driver asks its caller for"""
    _fields_ = [("rank", c_uint32), ("size", c_uint32), ("state", c_void_p), ("all_gather", ALL_GATHER), ("all_reduce_int64", ALL_REDUCE_INT64), ("all_reduce_max_bytes", ALL_REDUCE_MAX_BYTES),
                ("rccl_communicator", c_void_p)]


_workflow_lib = None


def workflow_library():
    """libarriba_workflow.so: the reference's main() over the two C ABIs (include/arriba_workflow.h); tests replace it with the build against the host stepping harness"""
    global _workflow_lib
    if _workflow_lib is None:
        device_library(); host_library()
        lib = _load(os.environ.get("ARRIBA_WORKFLOW_LIBRARY", os.path.join(LIB_DIR, "libarriba_workflow.so")))
        lib.arriba_workflow_default_options.argtypes = [POINTER(WorkflowOptions)]; lib.arriba_workflow_default_options.restype = None
        lib.arriba_workflow_last_error.restype = c_char_p
        lib.arriba_workflow_run.argtypes = [POINTER(WorkflowOptions), POINTER(WorkflowReport)]; lib.arriba_workflow_run.restype = c_int
        lib.arriba_workflow_open.argtypes = [POINTER(WorkflowOptions)]; lib.arriba_workflow_open.restype = c_void_p
        lib.arriba_workflow_sample.argtypes = [c_void_p, c_char_p, c_char_p, c_char_p, POINTER(WorkflowReport), POINTER(WorkflowTiming)]; lib.arriba_workflow_sample.restype = c_int
        lib.arriba_workflow_sample_separate.argtypes = [c_void_p, c_char_p, c_char_p, c_char_p, c_char_p, POINTER(WorkflowReport), POINTER(WorkflowTiming)]; lib.arriba_workflow_sample_separate.restype = c_int
        lib.arriba_workflow_submit.argtypes = [c_void_p, c_char_p]; lib.arriba_workflow_submit.restype = c_int
        lib.arriba_workflow_sorted_bam.argtypes = [c_void_p, c_char_p]; lib.arriba_workflow_sorted_bam.restype = c_int
        lib.arriba_workflow_supporting_alignments.argtypes = [c_void_p, c_char_p]; lib.arriba_workflow_supporting_alignments.restype = c_int
        lib.arriba_workflow_virus_expression.argtypes = [c_void_p, c_char_p]; lib.arriba_workflow_virus_expression.restype = c_int
        lib.arriba_workflow_coverage.argtypes = [c_void_p, c_char_p]; lib.arriba_workflow_coverage.restype = c_int
        lib.arriba_workflow_gene_counts.argtypes = [c_void_p, c_char_p]; lib.arriba_workflow_gene_counts.restype = c_int
        lib.arriba_workflow_splice_junctions.argtypes = [c_void_p, c_char_p]; lib.arriba_workflow_splice_junctions.restype = c_int
        lib.arriba_workflow_allele_counts.argtypes = [c_void_p, c_char_p, c_char_p, c_uint32, c_uint32]; lib.arriba_workflow_allele_counts.restype = c_int
        lib.arriba_workflow_realign.argtypes = [c_void_p, c_char_p, c_char_p]; lib.arriba_workflow_realign.restype = c_int
        lib.arriba_workflow_rna_metrics.argtypes = [c_void_p, c_char_p, c_char_p]; lib.arriba_workflow_rna_metrics.restype = c_int
        lib.arriba_workflow_variant_sites.argtypes = [c_void_p, c_char_p, c_uint32, c_uint32, c_uint32, c_uint32]; lib.arriba_workflow_variant_sites.restype = c_int
        lib.arriba_workflow_indel_sites.argtypes = [c_void_p, c_char_p, c_uint32, c_uint32, c_uint32]; lib.arriba_workflow_indel_sites.restype = c_int
        lib.arriba_workflow_sorted_bam_compression.argtypes = [c_void_p, c_int]; lib.arriba_workflow_sorted_bam_compression.restype = c_int
        lib.arriba_workflow_sorted_bam_mark_duplicates.argtypes = [c_void_p, c_int]; lib.arriba_workflow_sorted_bam_mark_duplicates.restype = c_int
        lib.arriba_workflow_cancel.argtypes = [c_void_p]; lib.arriba_workflow_cancel.restype = c_int
        lib.arriba_workflow_defer_output.argtypes = [c_void_p, c_int]; lib.arriba_workflow_defer_output.restype = c_int
        lib.arriba_workflow_finish_ahead.argtypes = [c_void_p, c_int]; lib.arriba_workflow_finish_ahead.restype = c_int
        lib.arriba_workflow_flush.argtypes = [c_void_p, POINTER(ctypes.c_double)]; lib.arriba_workflow_flush.restype = c_int
        lib.arriba_workflow_set_communicator.argtypes = [c_void_p, POINTER(WorkflowCommunicator)]; lib.arriba_workflow_set_communicator.restype = c_int
        lib.arriba_workflow_rccl_unique_id.argtypes = [c_void_p]; lib.arriba_workflow_rccl_unique_id.restype = c_int
        lib.arriba_workflow_join_rccl.argtypes = [c_void_p, c_void_p, c_uint32, c_uint32]; lib.arriba_workflow_join_rccl.restype = c_int
        lib.arriba_workflow_device.argtypes = [c_void_p]; lib.arriba_workflow_device.restype = c_void_p
        lib.arriba_workflow_lane_device.argtypes = [c_void_p, c_int]; lib.arriba_workflow_lane_device.restype = c_void_p
        lib.arriba_workflow_host.argtypes = [c_void_p]; lib.arriba_workflow_host.restype = c_void_p
        lib.arriba_workflow_close.argtypes = [c_void_p]; lib.arriba_workflow_close.restype = None
        _workflow_lib = lib
    return _workflow_lib


def device_library():
    global _device_lib
    if _device_lib is None:
        _device_lib = _load(os.path.join(LIB_DIR, "libarriba_gpu.so"))
    return _device_lib


def host_library():
    global _host_lib
    if _host_lib is None:
        _host_lib = bind_host_api(_load(os.environ.get("ARRIBA_HOST_LIBRARY", os.path.join(LIB_DIR, "libarriba_host.so"))))  # the override: a sanitizer build (tools/)
    return _host_lib
