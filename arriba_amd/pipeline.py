"""Host-side mirror of the reference's stage order for the hot path (reference: source/arriba.cpp:119-413).

``HostSession`` reads FASTA/GTF/BAM through libarriba_host.so and owns the structure-of-arrays views.
``DevicePipeline`` pushes them through the C ABI of libarriba_gpu.so (include/arriba_gpu.h) and calls the
device stages where the reference calls the corresponding stage function.  Method names follow the reference.
"""
import ctypes
from ctypes import POINTER, byref, c_float, c_int32, c_uint32, c_uint64

import numpy as np

from . import _capi


def _array(pointer, count, kind):
    return np.ctypeslib.as_array(ctypes.cast(pointer, POINTER(kind)), (count,)).copy() if count else np.zeros(0, np.dtype(kind))


def virus_counters_of(counters):
    """agpu_virus_counters (the device's or the host's) as a dict of numbers and arrays of its own"""
    n, m = counters.n_viruses, counters.n_active
    out = {name: _array(getattr(counters, name), n, c_uint64) for name in ("reads", "covered", "kmer_count")}
    out.update({"total": int(counters.total), "active": _array(counters.active, m, c_uint32), "shared": _array(counters.shared, m * m, c_uint64).reshape(m, m)})
    out.update({name: int(getattr(counters, name)) for name in ("candidates", "kmer_keys", "kmer_rounds", "peak_bytes")})
    out["seconds"] = dict(zip(("scan", "candidates", "kmer_sets", "covered"), counters.seconds))
    return out


def virus_contigs_of(contigs):
    """ahost_virus_contigs as a dict"""
    n = contigs.n_viruses
    offsets = _array(contigs.name_offset, n + 1, c_uint32)
    text = ctypes.string_at(contigs.names, int(offsets[-1])) if n else b""
    return {"n_ref": int(contigs.n_ref), "viral_ref": _array(contigs.viral_ref, n, c_int32), "viral_length": _array(contigs.viral_length, n, c_uint32),
            "names": [text[offsets[k]:offsets[k + 1]].decode() for k in range(n)]}


def depth_stats_of(stats):
    """agpu_depth_stats (the device's or the host's) as a dict"""
    out = {name: int(getattr(stats, name)) for name in ("records", "segments", "runs", "covered_positions", "aligned_bases", "max_depth", "text_bytes", "position_windows", "text_windows", "peak_bytes")}
    out["seconds"] = dict(zip(("marks", "scan", "runs", "text"), stats.seconds))
    return out


def markdup_counts_of(counts):
    """agpu_markdup_counts (the device's or the host's) as a dict"""
    out = {name: int(getattr(counts, name)) for name in ("templates", "pairs", "fragments", "duplicate_pairs", "duplicate_fragments", "records_flagged", "records_changed", "peak_bytes")}
    out["seconds"] = dict(zip(("name_ids", "ends", "selection"), counts.seconds))
    return out


def gene_count_stats_of(stats):
    """agpu_gene_count_stats (the device's or the host's) as a dict"""
    out = {name: int(getattr(stats, name)) for name in ("records", "templates", "without_primary", "ends", "blocks", "peak_bytes")}
    out["seconds"] = dict(zip(("names", "assign"), stats.seconds))
    return out


def junction_stats_of(stats):
    """agpu_junction_stats (the device's or the host's) as a dict"""
    out = {name: int(getattr(stats, name)) for name in ("records", "contributing", "crossings", "pairs", "junctions", "annotated", "peak_bytes")}
    out["seconds"] = dict(zip(("count", "names", "emit", "order", "classify"), stats.seconds))
    return out


def allele_stats_of(stats):
    """agpu_allele_stats (the device's or the host's) as a dict"""
    out = {name: int(getattr(stats, name)) for name in ("records", "contributing", "hits", "sites", "placed", "covered", "peak_bytes")}
    out["seconds"] = dict(zip(("sites", "count", "rows"), stats.seconds))
    return out


def variant_stats_of(stats):
    """agpu_variant_stats (the device's or the host's) as a dict"""
    out = {name: int(getattr(stats, name)) for name in ("records", "contributing", "events", "runs", "candidates", "reported", "inconsistent", "peak_bytes")}
    out["seconds"] = dict(zip(("count", "fill", "group", "counters", "rows"), stats.seconds))
    return out


def indel_stats_of(stats):
    """agpu_indel_stats (the device's or the host's) as a dict"""
    out = {name: int(getattr(stats, name)) for name in ("records", "contributing", "operations", "events", "unkeyed_insertions", "shift_capped", "runs", "candidates", "sites", "reported", "peak_bytes")}
    out["seconds"] = dict(zip(("count", "fill", "group", "counters", "rows"), stats.seconds))
    return out


def rna_metrics_stats_of(stats):
    """agpu_rna_metrics_stats (the device's or the host's) as a dict"""
    out = {name: int(getattr(stats, name)) for name in ("records", "base_records", "blocks", "segments", "track_runs", "peak_bytes")}
    out["seconds"] = {"kernel": stats.seconds[0]}
    return out


def realign_stats_of(stats):
    """agpu_realign_stats (the device's or the host's) as a dict"""
    out = {name: int(getattr(stats, name)) for name in ("records", "templates", "realign_templates", "kept_templates", "dropped_secondary", "extra", "orphans", "placeholder_cigar", "realign_bytes", "kept_bytes", "peak_bytes")}
    out["layout"] = "PE" if stats.layout else "SE"
    out["seconds"] = dict(zip(("name", "verdict", "scan", "text"), stats.seconds))
    return out


class ArribaError(RuntimeError):
    pass


class HostSession(object):
    """load_assembly + read_annotation_gtf + read_chimeric_alignments (reference: source/arriba.cpp:91-130)."""

    def __init__(self, fasta, gtf, interesting_contigs=None, viral_contigs=None, gtf_features=None):
        self._lib = _capi.host_library()
        enc = lambda s: None if s is None else s.encode()
        self._session = self._lib.ahost_open(enc(fasta), enc(gtf), enc(interesting_contigs), enc(viral_contigs), enc(gtf_features))
        if not self._session:
            raise ArribaError("ERROR: " + self._lib.ahost_last_error().decode())
        self._keepalive = None

    def close(self):
        if self._session:
            self._lib.ahost_close(self._session)
            self._session = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def read_chimeric_alignments(self, bam, external_duplicate_marking=False, max_itd_length=100, separate_chimeric=None):
        """bam: path to a BAM file, or a bytes-like object / numpy uint8 array holding the raw (inflated) BAM stream.
        separate_chimeric (-c): path of the separate chimeric file of STAR --chimOutType SeparateSAMold, read in front of `bam` (a path, too) as source/arriba.cpp:123-130 does;
        self.separate_counts then holds the (total=N) and the malformed count of that first pass."""
        if separate_chimeric is not None:
            fragments, malformed = ctypes.c_uint64(0), ctypes.c_uint64(0)
            status = self._lib.ahost_ingest_separate(self._session, separate_chimeric.encode(), bam.encode(), int(external_duplicate_marking), max_itd_length, byref(fragments), byref(malformed))
            self.separate_counts = (fragments.value, malformed.value)
        elif isinstance(bam, str):
            status = self._lib.ahost_ingest_bam_file(self._session, bam.encode(), int(external_duplicate_marking), max_itd_length)
        else:
            array = np.frombuffer(bam, dtype=np.uint8) if not isinstance(bam, np.ndarray) else bam
            self._keepalive = array
            status = self._lib.ahost_ingest_bam_memory(self._session, array.ctypes.data, array.size, int(external_duplicate_marking), max_itd_length)
        if status != 0:
            raise ArribaError("ERROR: " + self._lib.ahost_last_error().decode())
        return self.fragment_count

    def load_tags(self, path):
        """-t: tags for the column `tags` of the output files (reference: load_tags, source/annotate_tags.cpp:11-44)"""
        if self._lib.ahost_load_tags(self._session, path.encode()) != 0:
            raise ArribaError("ERROR: " + self._lib.ahost_last_error().decode())

    def load_protein_domains(self, path):
        """-p: protein domains (GFF3) for the column `retained_protein_domains` (reference: load_protein_domains, source/annotate_protein_domains.cpp:33-121)"""
        if self._lib.ahost_load_protein_domains(self._session, path.encode()) != 0:
            raise ArribaError("ERROR: " + self._lib.ahost_last_error().decode())

    def save_ingest(self, path):
        """the ingest result (batch, counters, coverage) as a file; load_ingest() of a session on the same FASTA/GTF restores it without parsing"""
        if self._lib.ahost_save_ingest(self._session, path.encode()) != 0:
            raise ArribaError("ERROR: " + self._lib.ahost_last_error().decode())

    def load_ingest(self, path):
        if self._lib.ahost_load_ingest(self._session, path.encode()) != 0:
            raise ArribaError("ERROR: " + self._lib.ahost_last_error().decode())
        return self.fragment_count

    @property
    def fragment_count(self):
        return int(self._lib.ahost_fragment_count(self._session))

    @property
    def mapped_reads(self):
        return int(self._lib.ahost_mapped_reads(self._session))

    @property
    def viral_read_total(self):
        """the pristine reads the ingest counted on viral contigs, over all of them"""
        return int(self._lib.ahost_viral_read_total(self._session))

    @property
    def annotation_view(self):
        return self._lib.ahost_annotation_view(self._session)

    @property
    def genome_view(self):
        return self._lib.ahost_genome_view(self._session)

    @property
    def batch_view(self):
        view = self._lib.ahost_batch_view(self._session)
        if not view:
            raise ArribaError("no BAM ingested yet")
        return view

    def contig_names(self):
        return [self._lib.ahost_contig_name(self._session, c).decode() for c in range(self._lib.ahost_contig_count(self._session))]

    def fragment_names(self):
        names = []
        length = c_uint32()
        for i in range(self.fragment_count):
            pointer = self._lib.ahost_fragment_name(self._session, i, byref(length))
            names.append(ctypes.string_at(pointer, length.value).decode())
        return names

    def detect_strandedness(self):
        return int(self._lib.ahost_detect_strandedness(self._session))

    def viral_verdicts(self, pairs, gene_bits, top_count=5, min_covered_fraction=0.05):
        n_contigs = self._lib.ahost_contig_count(self._session)
        top = np.zeros(n_contigs, dtype=np.uint8)
        low = np.zeros(n_contigs, dtype=np.uint8)
        pairs = np.ascontiguousarray(pairs, dtype=np.uint32)
        gene_bits = np.ascontiguousarray(gene_bits, dtype=np.uint8)
        self._lib.ahost_viral_verdicts(self._session, pairs.ctypes.data, pairs.size // 2, gene_bits.ctypes.data, gene_bits.size, top_count, min_covered_fraction, top.ctypes.data, low.ctypes.data)
        return top, low

    def estimate_fragment_length(self, mate_gaps, fragments_visited, default_fragment_length=200):
        mate_gaps = np.ascontiguousarray(mate_gaps, dtype=np.int32)
        mean, stddev, read_length = c_float(), c_float(), c_float()
        max_mate_gap = c_int32()
        estimated = self._lib.ahost_estimate_fragment_length(self._session, mate_gaps.ctypes.data, mate_gaps.size, fragments_visited, default_fragment_length,
                                                             byref(mean), byref(stddev), byref(read_length), byref(max_mate_gap))
        return {"estimated": bool(estimated), "mate_gap_mean": mean.value, "mate_gap_stddev": stddev.value, "read_length_mean": read_length.value, "max_mate_gap": max_mate_gap.value}


class WorkflowSession(object):
    """The product path as a resident service: arriba_workflow_open once (assembly, annotation, device context), arriba_workflow_sample per BAM file -- the reference's
    main() in C++ over the two C ABIs (arriba_amd/csrc/workflow/workflow.cpp; reference: source/arriba.cpp:84-615), no Python between the stages.  bench.py times
    `sample`; `device` is a DevicePipeline view of the session's device context for the kernel profile and the post-conditions."""

    def __init__(self, fasta, gtf, params=None, device=0, api=None, **options):
        self._lib = _capi.workflow_library()
        self.options = _capi.WorkflowOptions()
        self._lib.arriba_workflow_default_options(byref(self.options))
        self.options.assembly_file, self.options.gene_annotation_file = fasta.encode(), gtf.encode()
        self.options.device_index = device
        for key, value in (params or {}).items():
            if key == "disable_filters":
                for name in value:
                    self.options.device.filter_enabled[_capi.FILTER_NAMES.index(name)] = 0
            else:
                setattr(self.options.device, key, value)
        for key, value in options.items():
            setattr(self.options, key, value.encode() if isinstance(value, str) else value)
        self._session = self._lib.arriba_workflow_open(byref(self.options))
        if not self._session:
            raise ArribaError(self._lib.arriba_workflow_last_error().decode())
        self.api = api if api is not None else _capi.bind_device_api(_capi.device_library(), "agpu_")
        self.ctx = self._lib.arriba_workflow_device(self._session)
        self.timing, self.report, self.n, self.n_candidates, self.records = {}, [], 0, 0, -1
        self.timings, self._profiling_on, self.ingest_result = {}, False, None  # (what bench.py reads from a DevicePipeline)
        self._profiled = set()

    def sorted_bam_compression(self, level):
        """--sorted-bam-compression of the samples submitted from now on: 0 stored blocks, 1 deflated on the device"""
        if self._lib.arriba_workflow_sorted_bam_compression(self._session, int(level)) != 0:
            raise ArribaError(self._lib.arriba_workflow_last_error().decode())

    def sorted_bam_mark_duplicates(self, on):
        """--mark-duplicates of the samples submitted from now on: their --sorted-bam files leave with flag 0x400 set on duplicate templates and cleared on all others"""
        if self._lib.arriba_workflow_sorted_bam_mark_duplicates(self._session, int(bool(on))) != 0:
            raise ArribaError(self._lib.arriba_workflow_last_error().decode())

    def submit(self, bam, sorted_bam_file=None, supporting_alignments_prefix=None, sorted_bam_compression=None, virus_expression_file=None, coverage_file=None, mark_duplicates=None, gene_counts_file=None, splice_junctions_file=None, allele_sites_file=None, allele_counts_file=None, allele_min_mapq=0, allele_min_baseq=13, realign_reads_file=None, realign_kept_file=None, rna_metrics_file=None, rrna_intervals_file=None, variant_sites_file=None, variant_min_mapq=20, variant_min_baseq=13, variant_min_alt=3, variant_min_percent=5, indel_sites_file=None, indel_min_mapq=20, indel_min_alt=3, indel_min_percent=5):
        """the sample that comes after the one `sample` is called for next: its file is fed (PCIe, the front of read_chimeric_alignments) while the stages of that one run;
        sorted_bam_file: its records in coordinate order with their index (--sorted-bam), written when its ingest is finished; sorted_bam_compression: its level (None: as it is)"""
        if sorted_bam_compression is not None:
            self.sorted_bam_compression(sorted_bam_compression)
        if mark_duplicates is not None:  # (--mark-duplicates: None leaves it as it is)
            self.sorted_bam_mark_duplicates(mark_duplicates)
        self._lib.arriba_workflow_sorted_bam(self._session, sorted_bam_file.encode() if sorted_bam_file else None)
        self._lib.arriba_workflow_supporting_alignments(self._session, supporting_alignments_prefix.encode() if supporting_alignments_prefix else None)  # (--supporting-alignments: PREFIX_ID.bam per row of its fusions file)
        self._lib.arriba_workflow_virus_expression(self._session, virus_expression_file.encode() if virus_expression_file else None)  # (--virus-expression: its table, written when its ingest is finished)
        self._lib.arriba_workflow_coverage(self._session, coverage_file.encode() if coverage_file else None)  # (--coverage: its depth track, written when its ingest is finished)
        self._lib.arriba_workflow_gene_counts(self._session, gene_counts_file.encode() if gene_counts_file else None)  # (--gene-counts: its reads per gene, likewise)
        self._lib.arriba_workflow_splice_junctions(self._session, splice_junctions_file.encode() if splice_junctions_file else None)  # (--splice-junctions: its junction table, likewise)
        self._lib.arriba_workflow_allele_counts(self._session, allele_sites_file.encode() if allele_sites_file else None, allele_counts_file.encode() if allele_counts_file else None, allele_min_mapq, allele_min_baseq)  # (--allele-counts: likewise)
        self._lib.arriba_workflow_realign(self._session, realign_reads_file.encode() if realign_reads_file else None, realign_kept_file.encode() if realign_kept_file else None)  # (--realign-reads: likewise)
        self._lib.arriba_workflow_rna_metrics(self._session, rna_metrics_file.encode() if rna_metrics_file else None, rrna_intervals_file.encode() if rrna_intervals_file else None)  # (--rna-metrics: its QC table, likewise)
        self._lib.arriba_workflow_variant_sites(self._session, variant_sites_file.encode() if variant_sites_file else None, variant_min_mapq, variant_min_baseq, variant_min_alt, variant_min_percent)  # (--variant-sites: likewise)
        self._lib.arriba_workflow_indel_sites(self._session, indel_sites_file.encode() if indel_sites_file else None, indel_min_mapq, indel_min_alt, indel_min_percent)  # (--indel-sites: likewise)
        if self._lib.arriba_workflow_submit(self._session, bam.encode()) != 0:
            raise ArribaError(self._lib.arriba_workflow_last_error().decode())
        if self._profiling_on:
            self.set_profiling(True, only_new_lanes=True)

    def finish_ahead(self, on=True):
        """the ingest of a sample that was submitted ahead is finished by its feeder thread, beside the stages of the sample in front (the lanes keep their batch buffers: ~25 GB more at 10^8 fragments)"""
        if self._lib.arriba_workflow_finish_ahead(self._session, int(on)) != 0:
            raise ArribaError(self._lib.arriba_workflow_last_error().decode())

    def over_ranks(self, group=None):
        """One sample over the ranks of `group` (arriba_workflow_set_communicator, include/arriba_workflow.h): `sample` becomes a collective call -- every rank feeds its part of
        the file, one all-gather of the parts, the stages on every rank, filter_mismappers and the rows of the output files shared out, rank 0 writes.  The three collectives
        over host memory the C++ driver asks for are torch.distributed's (gloo in the CPU tests; with the nccl backend the host bytes go through tensors on this rank's GPU)."""
        import numpy as np
        import torch
        import torch.distributed as dist
        rank, size = dist.get_rank(group), dist.get_world_size(group)
        device = torch.device("cuda", self.options.device_index) if dist.get_backend(group) == "nccl" else torch.device("cpu")

        def host_array(pointer, count, dtype):
            return np.ctypeslib.as_array(ctypes.cast(pointer, ctypes.POINTER(np.ctypeslib.as_ctypes_type(dtype))), shape=(count,))

        def guarded(work):  # an exception must not cross the C frames above a callback: the driver is told with a status and ends the call on every rank
            def call(*arguments):
                try:
                    work(*arguments)
                    return 0
                except Exception as problem:
                    self.exchange_error = problem
                    return 1
            return call

        def all_gather(state, mine, everybody, n_bytes):
            if n_bytes == 0:
                return
            sent = torch.from_numpy(host_array(mine, n_bytes, np.uint8)).to(device)
            parts = [torch.empty(n_bytes, dtype=torch.uint8, device=device) for _ in range(size)]
            dist.all_gather(parts, sent, group=group)
            received = host_array(everybody, size * n_bytes, np.uint8)
            for r in range(size):
                received[r * n_bytes:(r + 1) * n_bytes] = parts[r].cpu().numpy()

        def all_reduce_int64(state, values, count, operation):
            array = host_array(values, count, np.int64)
            tensor = torch.from_numpy(array.copy()).to(device)
            dist.all_reduce(tensor, op={_capi.WORKFLOW_MAX: dist.ReduceOp.MAX, _capi.WORKFLOW_MIN: dist.ReduceOp.MIN, _capi.WORKFLOW_SUM: dist.ReduceOp.SUM}[operation], group=group)
            array[:] = tensor.cpu().numpy()

        def all_reduce_max_bytes(state, values, count):
            array = host_array(values, count, np.uint8)
            tensor = torch.from_numpy(array.copy()).to(device)
            dist.all_reduce(tensor, op=dist.ReduceOp.MAX, group=group)
            array[:] = tensor.cpu().numpy()

        self.exchange_error = None
        self._communicator = _capi.WorkflowCommunicator(rank, size, None, _capi.ALL_GATHER(guarded(all_gather)), _capi.ALL_REDUCE_INT64(guarded(all_reduce_int64)),
                                                        _capi.ALL_REDUCE_MAX_BYTES(guarded(all_reduce_max_bytes)), None)  # (kept: the session calls into it)
        if self._lib.arriba_workflow_set_communicator(self._session, byref(self._communicator)) != 0:
            raise ArribaError(self._lib.arriba_workflow_last_error().decode())
        self.rank, self.world = rank, size

    def join_rccl(self, unique_id, rank, size):
        """One sample over `size` GPUs with RCCL alone (arriba_workflow_join_rccl): `unique_id` = rccl_unique_id() of rank 0, brought to every rank by whatever started them; the
        parts of the batch and the verdicts of filter_mismappers travel in device memory, sizes, status words and row texts are bounced through the device."""
        buffer = (ctypes.c_ubyte * _capi.RCCL_ID_BYTES).from_buffer_copy(bytes(unique_id))
        if self._lib.arriba_workflow_join_rccl(self._session, buffer, rank, size) != 0:
            raise ArribaError(self._lib.arriba_workflow_last_error().decode())
        self.rank, self.world = rank, size

    def rccl_unique_id(self):
        buffer = (ctypes.c_ubyte * _capi.RCCL_ID_BYTES)()
        if self._lib.arriba_workflow_rccl_unique_id(buffer) != 0:
            raise ArribaError(self._lib.arriba_workflow_last_error().decode())
        return bytes(buffer)

    def defer_output(self, on=True):
        """the last output file of a sample is written by a thread of the session while the next sample is worked on (complete behind flush())"""
        self._lib.arriba_workflow_defer_output(self._session, int(on))

    def flush(self):
        """waits for the deferred writers; returns the seconds the last one took"""
        seconds = ctypes.c_double()
        if self._lib.arriba_workflow_flush(self._session, byref(seconds)) != 0:
            raise ArribaError(self._lib.arriba_workflow_last_error().decode())
        return seconds.value

    def cancel(self):
        """throws away what was submitted and not worked on"""
        self._lib.arriba_workflow_cancel(self._session)

    def _lane_contexts(self):
        return [ctx for ctx in (self._lib.arriba_workflow_lane_device(self._session, lane) for lane in (0, 1)) if ctx]

    def sample(self, bam, output_file, discarded_output_file=None, sorted_bam_file=None, supporting_alignments_prefix=None, sorted_bam_compression=None, virus_expression_file=None, coverage_file=None, mark_duplicates=None, gene_counts_file=None, splice_junctions_file=None, allele_sites_file=None, allele_counts_file=None, allele_min_mapq=0, allele_min_baseq=13, realign_reads_file=None, realign_kept_file=None, rna_metrics_file=None, rrna_intervals_file=None, variant_sites_file=None, variant_min_mapq=20, variant_min_baseq=13, variant_min_alt=3, variant_min_percent=5, indel_sites_file=None, indel_min_mapq=20, indel_min_alt=3, indel_min_percent=5):
        """one sample, BAM file -> fusions.tsv (and discarded.tsv); returns the stages with their "(remaining=N)" counts.  sorted_bam_file (--sorted-bam): for a sample that was
        not submitted ahead; one that was says it to `submit`"""
        report, timing = _capi.WorkflowReport(), _capi.WorkflowTiming()
        if sorted_bam_compression is not None:  # (as sorted_bam_file: for a sample that was not submitted ahead)
            self.sorted_bam_compression(sorted_bam_compression)
        if mark_duplicates is not None:  # (likewise)
            self.sorted_bam_mark_duplicates(mark_duplicates)
        if sorted_bam_file:
            self._lib.arriba_workflow_sorted_bam(self._session, sorted_bam_file.encode())
        if supporting_alignments_prefix:  # (as sorted_bam_file: for a sample that was not submitted ahead)
            self._lib.arriba_workflow_supporting_alignments(self._session, supporting_alignments_prefix.encode())
        if virus_expression_file:  # (likewise)
            self._lib.arriba_workflow_virus_expression(self._session, virus_expression_file.encode())
        if coverage_file:  # (likewise)
            self._lib.arriba_workflow_coverage(self._session, coverage_file.encode())
        if gene_counts_file:  # (likewise)
            self._lib.arriba_workflow_gene_counts(self._session, gene_counts_file.encode())
        if splice_junctions_file:  # (likewise)
            self._lib.arriba_workflow_splice_junctions(self._session, splice_junctions_file.encode())
        if allele_sites_file or allele_counts_file:  # (likewise; one without the other is refused by the sample)
            self._lib.arriba_workflow_allele_counts(self._session, allele_sites_file.encode() if allele_sites_file else None, allele_counts_file.encode() if allele_counts_file else None, allele_min_mapq, allele_min_baseq)
        if realign_reads_file or realign_kept_file:  # (likewise; the kept file without the other is refused by the sample)
            self._lib.arriba_workflow_realign(self._session, realign_reads_file.encode() if realign_reads_file else None, realign_kept_file.encode() if realign_kept_file else None)
        if rna_metrics_file or rrna_intervals_file:  # (likewise; the intervals without the table are refused by the sample)
            self._lib.arriba_workflow_rna_metrics(self._session, rna_metrics_file.encode() if rna_metrics_file else None, rrna_intervals_file.encode() if rrna_intervals_file else None)
        if variant_sites_file or (variant_min_mapq, variant_min_baseq, variant_min_alt, variant_min_percent) != (20, 13, 3, 5):  # (likewise; thresholds without the file are refused by the sample)
            self._lib.arriba_workflow_variant_sites(self._session, variant_sites_file.encode() if variant_sites_file else None, variant_min_mapq, variant_min_baseq, variant_min_alt, variant_min_percent)
        if indel_sites_file or (indel_min_mapq, indel_min_alt, indel_min_percent) != (20, 3, 5):  # (likewise; thresholds without the file are refused by the sample)
            self._lib.arriba_workflow_indel_sites(self._session, indel_sites_file.encode() if indel_sites_file else None, indel_min_mapq, indel_min_alt, indel_min_percent)
        if self._lib.arriba_workflow_sample(self._session, bam.encode(), output_file.encode(), discarded_output_file.encode() if discarded_output_file else None, byref(report), byref(timing)) != 0:
            raise ArribaError(self._lib.arriba_workflow_last_error().decode())
        self.ctx = self._lib.arriba_workflow_device(self._session)  # (the lane that worked on this sample)
        self.timing = {name: getattr(timing, name) for name, _ in _capi.WorkflowTiming._fields_}
        self.report = [(report.stages[k].stage.decode(), int(report.stages[k].count)) for k in range(report.n_stages)]
        return self.report

    def sample_separate(self, separate_chimeric, bam, output_file, discarded_output_file=None):
        """-c through the session (arriba_workflow_sample_separate): the chimeric alignments of the sample come in `separate_chimeric`, read in front of `bam`.  Refused with samples
        submitted ahead and with finish_ahead on; the next `sample` is an ordinary one again."""
        report, timing = _capi.WorkflowReport(), _capi.WorkflowTiming()
        if self._lib.arriba_workflow_sample_separate(self._session, separate_chimeric.encode(), bam.encode(), output_file.encode(), discarded_output_file.encode() if discarded_output_file else None, byref(report), byref(timing)) != 0:
            raise ArribaError(self._lib.arriba_workflow_last_error().decode())
        self.ctx = self._lib.arriba_workflow_device(self._session)
        self.timing = {name: getattr(timing, name) for name, _ in _capi.WorkflowTiming._fields_}
        self.report = [(report.stages[k].stage.decode(), int(report.stages[k].count)) for k in range(report.n_stages)]
        return self.report

    def set_profiling(self, enabled, only_new_lanes=False):
        for ctx in self._lane_contexts():
            if only_new_lanes and ctx in self._profiled:
                continue
            self._check(self.api.set_profiling(ctx, int(enabled)))
            self._profiled.add(ctx)
        self._profiling_on = bool(enabled)

    def kernel_profile(self):
        """the launches of both lanes (a sample submitted ahead runs in the other lane)"""
        mine, launches = self.ctx, []
        try:
            for ctx in self._lane_contexts():
                self.ctx = ctx
                launches += DevicePipeline.kernel_profile(self)
        finally:
            self.ctx = mine
        return launches

    def gene_sets(self, slot):
        """of the fragments the device context of the last sample holds: all of them, or -- one sample over several ranks, the reads sharded -- this rank's share"""
        held = int(self.timing["shard_fragments"]) if getattr(self, "timing", None) and self.timing.get("shard_fragments", 0) > 0 else self.n
        everything, self.n = self.n, held
        try:
            return DevicePipeline.gene_sets(self, slot)
        finally:
            self.n = everything

    def _check(self, status):
        if status != 0:
            raise ArribaError("ERROR: " + self.api.last_error().decode() + " (status %d)" % status)

    def close(self):
        if self._session:
            self._lib.arriba_workflow_close(self._session)
            self._session = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DevicePipeline(object):
    """The device stages of the hot path in the reference's order.

    `api` defaults to the product library (libarriba_gpu.so, prefix agpu_); the CPU-only tests pass the host
    stepping harness of tests/emu instead.
    """

    def __init__(self, session, params=None, api=None, device=0, batch_view=None, bam=None, external_duplicate_marking=False, max_itd_length=100, piece_bytes=64 << 20, profiling=False, separate_chimeric=None):
        """bam: path of the BAM file -> read_chimeric_alignments runs on the device (agpu_ingest_*): the host session only opens the file, parses the
        header and feeds the bytes; the batch never exists on the host.  Without it the batch of the session's host ingest is uploaded."""
        self.session = session
        self.api = api if api is not None else _capi.bind_device_api(_capi.device_library(), "agpu_")
        self.params = _capi.Params()
        self.api.default_params(byref(self.params))
        if params:
            for key, value in params.items():
                if key == "disable_filters":
                    for name in value:
                        self.params.filter_enabled[_capi.FILTER_NAMES.index(name)] = 0
                else:
                    setattr(self.params, key, value)
        self.ctx = self.api.create(device, byref(self.params))
        if not self.ctx:
            raise ArribaError("ERROR: " + self.api.last_error().decode())
        self.timings = {}
        self._profiling_on = False
        self.wall_ms = {}
        import time
        self._last_record = time.perf_counter()
        self._check(self.api.upload_annotation(self.ctx, session.annotation_view))
        self.device_ingest = bam is not None
        self.ingest_result = None
        if profiling:
            self.set_profiling(True)  # before the ingest: its kernels are part of the profile
        if self.device_ingest and separate_chimeric is not None:  # -c: the chimeric alignments in a file of their own, read in front of `bam`
            self.read_chimeric_alignments_separate(separate_chimeric, bam, external_duplicate_marking, max_itd_length, piece_bytes)
        elif self.device_ingest:
            self.read_chimeric_alignments(bam, external_duplicate_marking, max_itd_length, piece_bytes)
        else:
            self._check(self.api.upload_genome(self.ctx, session.genome_view))
            self._check(self.api.upload_batch(self.ctx, batch_view if batch_view is not None else session.batch_view))
            self.n = int(batch_view.contents.n) if batch_view is not None else session.fragment_count
        self.n_real_genes = session.annotation_view.contents.n_genes
        self.n_dummy_genes = 0
        self.scalars = {}

    def _free_pieces(self):
        if getattr(self, "_pieces", None) is not None:
            for pointer in self._pieces[1]:
                self.api.host_free(pointer)
            self._pieces = None

    def close(self):
        if self.ctx:
            self._free_pieces()
            self._free_sorted_windows()
            self._free_depth_windows()
            self.api.destroy(self.ctx)
            self.ctx = None

    def read_chimeric_alignments(self, bam, external_duplicate_marking=False, max_itd_length=100, piece_bytes=64 << 20):
        """reference: read_chimeric_alignments, source/read_chimeric_alignments.cpp:560-773, on the device: the host opens the file, parses the BAM header
        and feeds the bytes in pieces (two pinned buffers in turn); records are cut, collated by name, classified, sanity-checked, sorted and packed in HBM"""
        import time
        started = time.perf_counter()
        config, result, fed = self._ingest_records(bam, external_duplicate_marking, max_itd_length, piece_bytes)
        finished = time.perf_counter()
        self._record("read_chimeric_alignments")
        self._adopt_ingest(config, result)
        self.ingest_seconds = {"feed": fed - started, "device": finished - fed, "adopt": time.perf_counter() - finished}
        return self.n

    def read_chimeric_alignments_separate(self, separate_chimeric, bam, external_duplicate_marking=False, max_itd_length=100, piece_bytes=64 << 20):
        """-c on the device (source/arriba.cpp:123-130): the separate chimeric file through the ingest as pass C, its batch set aside (agpu_separate_adopt), the main alignments as pass R,
        both batches as one (agpu_separate_merge).  self.separate_result: what pass C reported -- fragments = its (total=N), malformed_count = its WARNING."""
        _, self.separate_result, _ = self._ingest_records(separate_chimeric, external_duplicate_marking, max_itd_length, piece_bytes, role=_capi.ROLE_SEPARATE_CHIMERIC)
        if self.separate_result.no_chimeric_reads:
            raise ArribaError("ERROR: no split reads or discordant mates found (STAR must either be run with '--chimOutType WithinBAM' or the file 'Chimeric.out.sam' must be passed to Arriba via the argument -c)")
        self._check(self.api.separate_adopt(self.ctx))
        config, result, _ = self._ingest_records(bam, external_duplicate_marking, max_itd_length, piece_bytes, role=_capi.ROLE_SEPARATE_RNA)
        self._check(self.api.separate_merge(self.ctx, byref(result)))
        self._record("read_chimeric_alignments")
        self._adopt_ingest(config, result)
        return self.n

    def _ingest_records(self, bam, external_duplicate_marking, max_itd_length, piece_bytes, part=None, parts=None, role=0):
        """opens the file (or part `part` of `parts` of its records), feeds the pieces, runs agpu_ingest_finish; returns (config, result, time the last piece was fed)"""
        import time
        lib, handle = self.session._lib, self.session._session
        host_error = lambda: ArribaError("ERROR: " + lib.ahost_last_error().decode())
        config = _capi.IngestConfig()
        if role != 0:
            status = lib.ahost_bam_open_role(handle, bam.encode(), int(external_duplicate_marking), max_itd_length, role, byref(config))
        elif part is None:
            status = lib.ahost_bam_open(handle, bam.encode(), int(external_duplicate_marking), max_itd_length, byref(config))
        else:
            status = lib.ahost_bam_open_part(handle, bam.encode(), int(external_duplicate_marking), max_itd_length, part, parts, byref(config))
        if status != 0:
            raise host_error()
        try:
            if getattr(self, "_genome_contigs", None) != config.n_contigs:
                self._check(self.api.upload_genome(self.ctx, self.session.genome_view))  # the contigs of the BAM header are part of the run now
                self._genome_contigs = config.n_contigs
            self._check(self.api.ingest_begin(self.ctx, byref(config)))
            block_capacity = piece_bytes // 4096 + 16
            # the two pinned buffers of the pieces stay with the pipeline (pinning 2 x 256 MB costs as much as feeding a gigabyte): a resident service reads sample after sample
            if getattr(self, "_pieces", None) is None or self._pieces[0] != piece_bytes:
                self._free_pieces()
                buffers = []
                for _ in range(2):
                    pointer = self.api.host_alloc(piece_bytes)
                    if not pointer:
                        for allocated in buffers:
                            self.api.host_free(allocated)
                        raise ArribaError("ERROR: " + self.api.last_error().decode())
                    buffers.append(pointer)
                self._pieces = (piece_bytes, buffers, [(_capi.BgzfBlock * block_capacity)(), (_capi.BgzfBlock * block_capacity)()])
            _, buffers, tables = self._pieces
            piece = _capi.BamPiece()
            pushes = 0
            while True:
                status = lib.ahost_bam_next(handle, buffers[pushes & 1], piece_bytes, tables[pushes & 1], block_capacity, byref(piece))
                if status < 0:
                    raise host_error()
                if status == 0:
                    break
                if piece.stored_bgzf == _capi.PIECE_SAM_TEXT:
                    if pushes == 0:  # the @SQ names the lines are looked up in: once per ingest
                        names, offsets, n_targets = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_uint32()
                        if lib.ahost_bam_sam_targets(handle, byref(names), byref(offsets), byref(n_targets)) != 1:
                            raise host_error()
                        if not hasattr(self.api, "ingest_push_sam"):
                            raise ArribaError("ERROR: SAM text needs the transcoder of the device library (agpu_ingest_push_sam), which this library does not have")
                        self._check(self.api.ingest_sam_targets(self.ctx, names, offsets, n_targets))
                    self._check(self.api.ingest_push_sam(self.ctx, buffers[pushes & 1], piece.bytes, piece.first_line))
                elif piece.stored_bgzf in (_capi.PIECE_STORED_BGZF, _capi.PIECE_DEFLATED_BGZF):
                    self._check(self.api.ingest_push_bgzf(self.ctx, buffers[pushes & 1], piece.bytes, tables[pushes & 1], piece.n_blocks, piece.stream_bytes))
                else:
                    self._check(self.api.ingest_push(self.ctx, buffers[pushes & 1], piece.bytes))
                pushes += 1
            fed = time.perf_counter()
            result = _capi.IngestResult()
            self._check(self.api.ingest_finish(self.ctx, byref(result)))
        finally:
            lib.ahost_bam_close(handle)
        # (config.coverage_window_offset points into the session: read it before anything else touches the session)
        self._coverage_windows = int(config.coverage_window_offset[config.n_contigs]) if config.n_contigs else 0
        return config, result, fed

    def _adopt_ingest(self, config, result):
        """hands what the host's sequential stages and its writer need from the ingest on the device to the host session (reference: the tail of
        read_chimeric_alignments, source/read_chimeric_alignments.cpp:759-771, and coverage_t)"""
        lib, handle = self.session._lib, self.session._session
        n_contigs = config.n_contigs
        viral = np.zeros(max(n_contigs, 1), dtype=np.uint64)
        self._check(self.api.get_viral_read_counts(self.ctx, viral.ctypes.data))
        windows = self._coverage_windows
        coverage, starts, ends = np.zeros(max(windows, 1), dtype=np.uint16), np.zeros(max(windows, 1), dtype=np.uint8), np.zeros(max(windows, 1), dtype=np.uint8)
        self._check(self.api.get_coverage(self.ctx, coverage.ctypes.data, starts.ctypes.data, ends.ctypes.data))
        if lib.ahost_adopt_device_ingest(handle, byref(result), viral.ctypes.data, coverage.ctypes.data, starts.ctypes.data, ends.ctypes.data) != 0:
            raise ArribaError("ERROR: " + lib.ahost_last_error().decode())
        self.ingest_result = result
        self.n = int(result.fragments)
        self.device_ingest = True
        self.n_dummy_genes = 0
        self.scalars = {}
        return self.n

    MAX_BAI_REFERENCE = 1 << 29

    def write_sorted_bam(self, path, compression=0, mark_duplicates=False):
        """mark_duplicates (--mark-duplicates): flag 0x400 of every record set or cleared on the device by the rule of DESIGN.md 4.14 (agpu_sorted_bam_set_mark_duplicates); the counts
        are in self.markdup_counts afterwards.  compression (--sorted-bam-compression): 0 stored blocks; 1 every record block deflated on the device (agpu_sorted_bam_set_compression), "file_bytes" is then what the
        blocks really take.  The records of the file of the last read_chimeric_alignments in coordinate order as `path` (BAM of stored BGZF blocks) and `path`.bai -- what run_arriba.sh:47-51 gets
        from `samtools sort` / `samtools index` -- from the record stream that is still in HBM (agpu_sorted_bam_*).  Valid after read_chimeric_alignments and before the next one.
        Written through `path`.tmp / `path`.bai.tmp; returns {"records", "uncompressed_bytes", "file_bytes", "windows", "indexed"}; the seconds of its parts: self.sorted_bam_seconds."""
        import os
        import sys
        import time
        if not self.device_ingest or not hasattr(self.api, "sorted_bam_begin"):
            raise ArribaError("ERROR: a sorted BAM file needs the record stream of an ingest on the device (DevicePipeline(bam=...))")
        lib, handle = self.session._lib, self.session._session
        started = time.perf_counter()
        info = _capi.SortedBamInfo()
        if compression != 0:
            self._check(self.api.sorted_bam_set_compression(self.ctx, int(compression)))  # (0: the call is not made, as before the level existed)
        if mark_duplicates:
            self._check(self.api.sorted_bam_set_mark_duplicates(self.ctx, 1))  # (off: the call is not made, as before the option existed)
        self._check(self.api.sorted_bam_begin(self.ctx, byref(info)))  # (refused before anything is written: the stream given back, another ingest begun, a part of a sample)
        if mark_duplicates:
            counts = _capi.MarkdupCounts()
            self._check(self.api.markdup_stats(self.ctx, byref(counts)))
            self.markdup_counts = markdup_counts_of(counts)
        sorted_at = time.perf_counter()
        seconds = {"sort": sorted_at - started, "gather_and_copy": 0.0, "write": 0.0, "index": 0.0}
        temporaries = [path + ".tmp", path + ".bai.tmp"]
        try:
            framed, framed_bytes, lengths, n_ref = ctypes.c_void_p(), c_uint64(), ctypes.c_void_p(), ctypes.c_uint32()
            if lib.ahost_sorted_bam_header(handle, byref(framed), byref(framed_bytes), byref(lengths), byref(n_ref)) != 0:
                raise ArribaError("ERROR: " + lib.ahost_last_error().decode())
            ref_length = np.ctypeslib.as_array(ctypes.cast(lengths, ctypes.POINTER(ctypes.c_uint32)), (n_ref.value,)).copy() if n_ref.value else np.zeros(0, np.uint32)
            # two pinned buffers in turn: they stay with the pipeline, as the pieces of the feed do
            if getattr(self, "_sorted_windows", None) is None or self._sorted_windows[0] < info.window_bytes:
                self._free_sorted_windows()
                buffers = [self.api.host_alloc(info.window_bytes) for _ in range(2)]
                self._sorted_windows = (info.window_bytes, buffers)
                if not all(buffers):
                    self._free_sorted_windows()
                    raise ArribaError("ERROR: " + self.api.last_error().decode())
            capacity, buffers = self._sorted_windows
            with open(temporaries[0], "wb") as out:
                out.write(ctypes.string_at(framed, framed_bytes.value))
                got, turn, written = c_uint64(), 0, 0
                while True:
                    before = time.perf_counter()
                    self._check(self.api.sorted_bam_next(self.ctx, buffers[turn & 1], capacity, byref(got)))
                    middle = time.perf_counter()
                    seconds["gather_and_copy"] += middle - before
                    if got.value == 0:
                        break
                    out.write((ctypes.c_char * got.value).from_address(buffers[turn & 1]))
                    seconds["write"] += time.perf_counter() - middle
                    written += got.value
                    turn += 1
                expected = c_uint64(info.file_bytes)
                if compression != 0:  # (announced: the upper bound)
                    self._check(self.api.sorted_bam_compressed_bytes(self.ctx, byref(expected)))
                if written != expected.value or written > info.file_bytes:
                    raise ArribaError("ERROR: the record blocks of the sorted BAM file have %d bytes, %d were announced" % (written, info.file_bytes))
                eof = ctypes.create_string_buffer(28)
                lib.ahost_sorted_bam_eof(eof)
                out.write(eof.raw)
            indexed = bool((ref_length <= self.MAX_BAI_REFERENCE).all())
            if indexed:
                before = time.perf_counter()
                index = _capi.SortedBamIndex()
                self._check(self.api.sorted_bam_index(self.ctx, framed_bytes.value, ref_length.ctypes.data, n_ref.value, byref(index)))
                arrays = {name: np.zeros(max(size, 1), np.uint64) for name, size in (("chunk_key", index.n_chunks), ("chunk_begin", index.n_chunks), ("chunk_end", index.n_chunks), ("interval_offset", n_ref.value + 1),
                                                                                    ("intervals", index.n_intervals), ("ref_begin", n_ref.value), ("ref_end", n_ref.value), ("ref_mapped", n_ref.value), ("ref_unmapped", n_ref.value))}
                for name, array in arrays.items():
                    setattr(index, name, array.ctypes.data)
                self._check(self.api.sorted_bam_index(self.ctx, framed_bytes.value, ref_length.ctypes.data, n_ref.value, byref(index)))
                if lib.ahost_sorted_bam_write_index(byref(index), temporaries[1].encode()) != 0:
                    raise ArribaError("ERROR: " + lib.ahost_last_error().decode())
                seconds["index"] = time.perf_counter() - before
            else:
                sys.stderr.write("WARNING: a reference is longer than 2^29 bases, which a BAI index cannot address: '%s' is written without '%s.bai'\n" % (path, path))
            os.replace(temporaries[0], path)
            if indexed:
                os.replace(temporaries[1], path + ".bai")
        finally:
            for temporary in temporaries:
                if os.path.exists(temporary):
                    os.remove(temporary)
            self.api.sorted_bam_end(self.ctx)
        seconds["total"] = time.perf_counter() - started
        self.sorted_bam_seconds = seconds
        return {"records": int(info.records), "uncompressed_bytes": int(info.uncompressed_bytes), "file_bytes": int(written), "windows": int(info.windows), "indexed": indexed}

    def build_support_pool(self, names=None):
        """Phase 1 of --supporting-alignments: the records of the listed read names copied out of the record stream of the last read_chimeric_alignments into a pool that stays with
        this pipeline (agpu_support_pool_build).  names=None: the QNAMEs of the fragments of the batch (entry i is fragment i); else a list of names (bytes or str), entry i is names[i].
        Valid after read_chimeric_alignments and before the next one.  Returns {"names", "stream_records", "pooled_records", "pool_bytes"}."""
        if not self.device_ingest or not hasattr(self.api, "support_pool_build"):
            raise ArribaError("ERROR: the supporting alignments need the record stream of an ingest on the device (DevicePipeline(bam=...))")
        info = _capi.SupportPoolInfo()
        if names is None:
            self._check(self.api.support_pool_build(self.ctx, None, None, 0, byref(info)))
        else:
            encoded = [name.encode() if isinstance(name, str) else bytes(name) for name in names]
            offsets = np.zeros(len(encoded) + 1, np.uint64)
            offsets[1:] = np.cumsum([len(name) for name in encoded], dtype=np.uint64) if encoded else 0
            text = ctypes.create_string_buffer(b"".join(encoded), max(int(offsets[-1]), 1))
            self._check(self.api.support_pool_build(self.ctx, ctypes.cast(text, ctypes.c_void_p), offsets.ctypes.data, len(encoded), byref(info)))
        return {name: int(getattr(info, name)) for name in ("names", "stream_records", "pooled_records", "pool_bytes")}

    def virus_expression(self):
        """The counters of --virus-expression from the record stream of the last read_chimeric_alignments (agpu_virus_expression), for the viral contigs that the session's -v names
        in the header of its file.  Valid after read_chimeric_alignments and before the next one.  Returns (counters, contigs): counters {"total", "reads", "covered", "kmer_count"
        [n_viruses], "active" [n_active], "shared" [n_active, n_active], "candidates", "kmer_keys", "kmer_rounds", "peak_bytes", "seconds"}; contigs {"n_ref", "viral_ref",
        "viral_length", "names"}.  The two structures as the C ABI filled them are kept for write_virus_expression."""
        if not self.device_ingest or not hasattr(self.api, "virus_expression"):
            raise ArribaError("ERROR: a virus expression table needs the record stream of an ingest on the device (DevicePipeline(bam=...))")
        lib, handle = self.session._lib, self.session._session
        contigs = _capi.VirusContigs()
        if lib.ahost_virus_contigs_of_session(handle, byref(contigs)) != 0:
            raise ArribaError("ERROR: " + lib.ahost_last_error().decode())
        counters = _capi.VirusCounters()
        self._check(self.api.virus_expression(self.ctx, contigs.viral_ref, contigs.viral_length, contigs.n_viruses, contigs.n_ref, byref(counters)))
        self._virus = (counters, contigs)
        return virus_counters_of(counters), virus_contigs_of(contigs)

    def write_virus_expression(self, path):
        """--virus-expression: the table of the reference's scripts/quantify_virus_expression.sh (default parameters) as `path`, written through `path`.tmp; returns the counters"""
        counters, contigs = self.virus_expression()
        lib = self.session._lib
        if lib.ahost_virus_expression_write(byref(self._virus[0]), byref(self._virus[1]), path.encode()) != 0:
            raise ArribaError("ERROR: " + lib.ahost_last_error().decode())
        return counters

    def write_coverage(self, path):
        """--coverage: the per-base alignment depth of the records of the last read_chimeric_alignments as bedGraph text -- NAME START END DEPTH per run of equal depth > 0,
        contigs in header order --, computed and formatted on the device from the record stream that is still in HBM (agpu_depth_*).  Valid after
        read_chimeric_alignments and before the next one.  Written through `path`.tmp; returns the statistics {"records", "segments", "runs", "covered_positions", "aligned_bases",
        "max_depth", "text_bytes", "position_windows", "text_windows", "peak_bytes", "seconds"}."""
        import os
        if not self.device_ingest or not hasattr(self.api, "depth_begin"):
            raise ArribaError("ERROR: a coverage track needs the record stream of an ingest on the device (DevicePipeline(bam=...))")
        lib, handle = self.session._lib, self.session._session
        contigs = _capi.DepthContigs()
        if lib.ahost_depth_contigs_of_session(handle, byref(contigs)) != 0:
            raise ArribaError("ERROR: " + lib.ahost_last_error().decode())
        info, stats = _capi.DepthInfo(), _capi.DepthStats()
        self._check(self.api.depth_begin(self.ctx, contigs.length, contigs.names, contigs.name_offset, contigs.n_ref, byref(info)))  # (refused before anything is written)
        try:
            if getattr(self, "_depth_windows", None) is None or self._depth_windows[0] < info.window_bytes:  # two pinned buffers in turn: they stay with the pipeline
                self._free_depth_windows()
                buffers = [self.api.host_alloc(info.window_bytes) for _ in range(2)]
                self._depth_windows = (info.window_bytes, buffers)
                if not all(buffers):
                    self._free_depth_windows()
                    raise ArribaError("ERROR: " + self.api.last_error().decode())
            capacity, buffers = self._depth_windows
            with open(path + ".tmp", "wb") as out:
                got, turn = c_uint64(), 0
                while True:
                    self._check(self.api.depth_next(self.ctx, buffers[turn & 1], capacity, byref(got)))
                    if got.value == 0:
                        break
                    out.write((ctypes.c_char * got.value).from_address(buffers[turn & 1]))
                    turn += 1
            self._check(self.api.depth_end(self.ctx, byref(stats)))
            os.rename(path + ".tmp", path)
        except BaseException:
            self.api.depth_end(self.ctx, None)
            if os.path.exists(path + ".tmp"):
                os.remove(path + ".tmp")
            raise
        return depth_stats_of(stats)

    def gene_counts(self):
        """--gene-counts: reads per gene of the records of the last read_chimeric_alignments, counted on the device from the record stream that is still in HBM (agpu_gene_counts;
        DESIGN.md 4.15).  Valid after read_chimeric_alignments and before the next one.  Returns (counts, stats): counts[c][row], a uint64 array of shape (3, n_genes + 4) -- rows 0 .. 3
        are N_unmapped, N_multimapping, N_noFeature, N_ambiguous, row 4 + g is gene g of the session's table --, and {"records", "templates", "without_primary", "ends", "blocks",
        "peak_bytes", "seconds"}."""
        if not self.device_ingest or not hasattr(self.api, "gene_counts"):
            raise ArribaError("ERROR: gene counts need the record stream of an ingest on the device (DevicePipeline(bam=...))")
        lib, handle = self.session._lib, self.session._session
        contigs, n_genes = _capi.DepthContigs(), ctypes.c_uint32()
        if lib.ahost_depth_contigs_of_session(handle, byref(contigs)) != 0 or lib.ahost_gene_counts_genes(handle, byref(n_genes), None, None) != 0:
            raise ArribaError("ERROR: " + lib.ahost_last_error().decode())
        counts, stats = np.zeros((3, n_genes.value + 4), dtype=np.uint64), _capi.GeneCountStats()
        self._check(self.api.gene_counts(self.ctx, contigs.length, contigs.n_ref, counts.ctypes.data, byref(stats)))
        return counts, gene_count_stats_of(stats)

    def write_gene_counts(self, path):
        """--gene-counts: the table of `gene_counts` as the text of STAR's ReadsPerGene.out.tab, written through `path`.tmp; returns the statistics"""
        lib, handle = self.session._lib, self.session._session
        counts, stats = self.gene_counts()  # (refused before anything is written)
        if lib.ahost_gene_counts_write(handle, counts.ctypes.data, counts.size, path.encode()) != 0:
            raise ArribaError("ERROR: " + lib.ahost_last_error().decode())
        return stats

    def gene_counts_allocated_bytes(self):
        count = c_uint64()
        self._check(self.api.gene_counts_allocated_bytes(self.ctx, byref(count)))
        return int(count.value)

    def splice_junctions(self):
        """--splice-junctions: the splice junctions of the records of the last read_chimeric_alignments, made on the device from the record stream that is still in HBM
        (agpu_splice_junctions).  Valid after read_chimeric_alignments and before the next one.  Returns (rows, stats): rows a ctypes array of _capi.JunctionRow (a copy),
        ordered by (ref, start, end), and {"records", "contributing", "crossings", "pairs", "junctions", "annotated", "peak_bytes", "seconds"}."""
        if not self.device_ingest or not hasattr(self.api, "splice_junctions"):
            raise ArribaError("ERROR: splice junctions need the record stream of an ingest on the device (DevicePipeline(bam=...))")
        lib, handle = self.session._lib, self.session._session
        contigs = _capi.DepthContigs()
        if lib.ahost_depth_contigs_of_session(handle, byref(contigs)) != 0:
            raise ArribaError("ERROR: " + lib.ahost_last_error().decode())
        rows, n_rows, stats = ctypes.POINTER(_capi.JunctionRow)(), c_uint64(), _capi.JunctionStats()
        self._check(self.api.splice_junctions(self.ctx, contigs.length, contigs.n_ref, byref(rows), byref(n_rows), byref(stats)))
        copy = (_capi.JunctionRow * n_rows.value)()
        if n_rows.value:
            ctypes.memmove(copy, rows, ctypes.sizeof(copy))
        return copy, junction_stats_of(stats)

    def write_splice_junctions(self, path):
        """--splice-junctions: the rows of `splice_junctions` as the text of STAR's SJ.out.tab, written through `path`.tmp; returns the statistics"""
        lib, handle = self.session._lib, self.session._session
        rows, stats = self.splice_junctions()  # (refused before anything is written)
        contigs = _capi.DepthContigs()
        if lib.ahost_depth_contigs_of_session(handle, byref(contigs)) != 0 or lib.ahost_splice_junctions_write(byref(contigs), rows, len(rows), path.encode()) != 0:
            raise ArribaError("ERROR: " + lib.ahost_last_error().decode())
        return stats

    def splice_junctions_allocated_bytes(self):
        count = c_uint64()
        self._check(self.api.splice_junctions_allocated_bytes(self.ctx, byref(count)))
        return int(count.value)

    def allele_counts(self, sites_file, min_mapq=0, min_baseq=13):
        """--allele-counts: the bases the records of the last read_chimeric_alignments show at the sites of `sites_file`, counted on the device from the record stream that is still
        in HBM (agpu_allele_counts).  Valid after read_chimeric_alignments and before the next one.  Returns (rows, stats, sites): rows a ctypes array of
        _capi.AlleleRow (a copy), one per line of the sites file in its order; {"records", "contributing", "hits", "sites", "placed", "covered", "peak_bytes", "seconds"}; and the
        list of sites (_capi.AlleleSites), which the caller gives back with ahost_allele_sites_free."""
        if not self.device_ingest or not hasattr(self.api, "allele_counts"):
            raise ArribaError("ERROR: allele counts need the record stream of an ingest on the device (DevicePipeline(bam=...))")
        lib, handle = self.session._lib, self.session._session
        contigs, sites = _capi.DepthContigs(), _capi.AlleleSites()
        if lib.ahost_depth_contigs_of_session(handle, byref(contigs)) != 0 or lib.ahost_allele_sites_load(sites_file.encode(), None, 0, byref(sites)) != 0:
            raise ArribaError("ERROR: " + lib.ahost_last_error().decode())
        try:
            if lib.ahost_allele_sites_place_session(handle, byref(sites)) != 0:
                raise ArribaError("ERROR: " + lib.ahost_last_error().decode())
            rows, stats = ctypes.POINTER(_capi.AlleleRow)(), _capi.AlleleStats()
            self._check(self.api.allele_counts(self.ctx, sites.sites, sites.n_sites, contigs.length, contigs.n_ref, min_mapq, min_baseq, byref(rows), byref(stats)))
            copy = (_capi.AlleleRow * sites.n_sites)()
            if sites.n_sites:
                ctypes.memmove(copy, rows, ctypes.sizeof(copy))
        except Exception:
            lib.ahost_allele_sites_free(byref(sites))
            raise
        return copy, allele_stats_of(stats), sites

    def write_allele_counts(self, sites_file, path, min_mapq=0, min_baseq=13):
        """--allele-counts: the rows of `allele_counts` as the text of the file (a header line, then CONTIG POS REF A C G T N DEL SKIP LOWQ per line of the sites file), written
        through `path`.tmp; returns the statistics"""
        lib = self.session._lib
        rows, stats, sites = self.allele_counts(sites_file, min_mapq, min_baseq)  # (refused before anything is written)
        try:
            if lib.ahost_allele_counts_write(byref(sites), rows, len(rows), path.encode()) != 0:
                raise ArribaError("ERROR: " + lib.ahost_last_error().decode())
        finally:
            lib.ahost_allele_sites_free(byref(sites))
        return stats

    def allele_counts_allocated_bytes(self):
        count = c_uint64()
        self._check(self.api.allele_counts_allocated_bytes(self.ctx, byref(count)))
        return int(count.value)

    def variant_sites(self, min_mapq=20, min_baseq=13, min_alt=3, min_percent=5):
        """--variant-sites: the positions at which the records of the last read_chimeric_alignments show a base that differs from the assembly, found on the device from the record
        stream that is still in HBM (agpu_variant_sites).  Valid after read_chimeric_alignments and before the next one.  Returns (rows, stats): rows a ctypes array
        of _capi.VariantRow (a copy), ordered by (ref, pos), and {"records", "contributing", "events", "runs", "candidates", "reported", "inconsistent", "peak_bytes", "seconds"}."""
        if not self.device_ingest or not hasattr(self.api, "variant_sites"):
            raise ArribaError("ERROR: variant sites need the record stream of an ingest on the device (DevicePipeline(bam=...))")
        lib, handle = self.session._lib, self.session._session
        contigs = _capi.DepthContigs()
        if lib.ahost_depth_contigs_of_session(handle, byref(contigs)) != 0:
            raise ArribaError("ERROR: " + lib.ahost_last_error().decode())
        rows, n_rows, stats = ctypes.POINTER(_capi.VariantRow)(), c_uint64(), _capi.VariantStats()
        self._check(self.api.variant_sites(self.ctx, contigs.length, contigs.n_ref, min_mapq, min_baseq, min_alt, min_percent, byref(rows), byref(n_rows), byref(stats)))
        copy = (_capi.VariantRow * n_rows.value)()
        if n_rows.value:
            ctypes.memmove(copy, rows, ctypes.sizeof(copy))
        return copy, variant_stats_of(stats)

    def write_variant_sites(self, path, min_mapq=20, min_baseq=13, min_alt=3, min_percent=5):
        """--variant-sites: the rows of `variant_sites` as the text of the file (a header line, then CONTIG POS REF ALT A C G T N DEL SKIP LOWQ per site), written through
        `path`.tmp; returns the statistics"""
        lib, handle = self.session._lib, self.session._session
        rows, stats = self.variant_sites(min_mapq, min_baseq, min_alt, min_percent)  # (refused before anything is written)
        contigs = _capi.DepthContigs()
        if lib.ahost_depth_contigs_of_session(handle, byref(contigs)) != 0 or lib.ahost_variant_sites_write(byref(contigs), rows, len(rows), path.encode()) != 0:
            raise ArribaError("ERROR: " + lib.ahost_last_error().decode())
        return stats

    def variant_sites_allocated_bytes(self):
        count = c_uint64()
        self._check(self.api.variant_sites_allocated_bytes(self.ctx, byref(count)))
        return int(count.value)

    def indel_sites(self, min_mapq=20, min_alt=3, min_percent=5):
        """--indel-sites: the insertions and deletions the records of the last read_chimeric_alignments carry in their CIGARs, left-normalised against the assembly, found on the
        device from the record stream that is still in HBM (agpu_indel_sites).  Valid after read_chimeric_alignments and before the next one.  Returns (rows,
        stats): rows a ctypes array of _capi.IndelRow (a copy), ordered by (ref, pos, type, length, bases), and the statistics of indel_stats_of."""
        if not self.device_ingest or not hasattr(self.api, "indel_sites"):
            raise ArribaError("ERROR: indel sites need the record stream of an ingest on the device (DevicePipeline(bam=...))")
        lib, handle = self.session._lib, self.session._session
        contigs = _capi.DepthContigs()
        if lib.ahost_depth_contigs_of_session(handle, byref(contigs)) != 0:
            raise ArribaError("ERROR: " + lib.ahost_last_error().decode())
        rows, n_rows, stats = ctypes.POINTER(_capi.IndelRow)(), c_uint64(), _capi.IndelStats()
        self._check(self.api.indel_sites(self.ctx, contigs.length, contigs.n_ref, min_mapq, min_alt, min_percent, byref(rows), byref(n_rows), byref(stats)))
        copy = (_capi.IndelRow * n_rows.value)()
        if n_rows.value:
            ctypes.memmove(copy, rows, ctypes.sizeof(copy))
        return copy, indel_stats_of(stats)

    def write_indel_sites(self, path, min_mapq=20, min_alt=3, min_percent=5):
        """--indel-sites: the rows of `indel_sites` as the text of the file (a header line, then CONTIG POS REF TYPE LENGTH BASES SUPPORT DEPTH per event), written through
        `path`.tmp; returns the statistics"""
        lib, handle = self.session._lib, self.session._session
        rows, stats = self.indel_sites(min_mapq, min_alt, min_percent)  # (refused before anything is written)
        contigs = _capi.DepthContigs()
        if lib.ahost_depth_contigs_of_session(handle, byref(contigs)) != 0 or lib.ahost_indel_sites_write(handle, byref(contigs), rows, len(rows), path.encode()) != 0:
            raise ArribaError("ERROR: " + lib.ahost_last_error().decode())
        return stats

    def indel_sites_allocated_bytes(self):
        count = c_uint64()
        self._check(self.api.indel_sites_allocated_bytes(self.ctx, byref(count)))
        return int(count.value)

    def realign_split(self, realign_path, kept_path=None):
        """--realign-reads [--realign-kept]: the records of the last read_chimeric_alignments split into the templates that must be aligned again and the templates that are passed
        on, as SAM text (fields 1-11; `kept_path` behind a header with the contigs of the assembly), decided and formatted on the device from the record stream that is still in
        HBM (agpu_realign_*).  Valid after read_chimeric_alignments and before the next one.  Written through NAME.tmp; returns the statistics {"records",
        "templates", "realign_templates", "kept_templates", "dropped_secondary", "extra", "orphans", "placeholder_cigar", "realign_bytes", "kept_bytes", "layout", "peak_bytes",
        "seconds"}."""
        import os
        if not self.device_ingest or not hasattr(self.api, "realign_begin"):
            raise ArribaError("ERROR: a split for realignment needs the record stream of an ingest on the device (DevicePipeline(bam=...))")
        if kept_path is not None and os.path.abspath(kept_path) == os.path.abspath(realign_path):
            raise ArribaError("ERROR: --realign-reads and --realign-kept name the same file")
        lib, handle = self.session._lib, self.session._session
        contigs, plan = _capi.DepthContigs(), _capi.RealignPlan()
        if lib.ahost_depth_contigs_of_session(handle, byref(contigs)) != 0 or lib.ahost_realign_plan_of_session(handle, byref(plan)) != 0:
            raise ArribaError("ERROR: " + lib.ahost_last_error().decode())
        header = ctypes.string_at(plan.header, plan.header_bytes)
        info, stats = _capi.RealignInfo(), _capi.RealignStats()
        self._check(self.api.realign_begin(self.ctx, plan.in_assembly, contigs.names, contigs.name_offset, contigs.n_ref, int(kept_path is not None), byref(info)))  # (refused before anything is written)
        paths = [path for path in (realign_path, kept_path) if path is not None]
        try:
            if getattr(self, "_depth_windows", None) is None or self._depth_windows[0] < info.window_bytes:  # the two pinned buffers of write_coverage: they stay with the pipeline
                self._free_depth_windows()
                buffers = [self.api.host_alloc(info.window_bytes) for _ in range(2)]
                self._depth_windows = (info.window_bytes, buffers)
                if not all(buffers):
                    self._free_depth_windows()
                    raise ArribaError("ERROR: " + self.api.last_error().decode())
            capacity, buffers = self._depth_windows
            for which, path in enumerate(paths):
                with open(path + ".tmp", "wb") as out:
                    if which == 1:
                        out.write(header)
                    got, turn = c_uint64(), 0
                    while True:
                        self._check(self.api.realign_next(self.ctx, which, buffers[turn & 1], capacity, byref(got)))
                        if got.value == 0:
                            break
                        out.write((ctypes.c_char * got.value).from_address(buffers[turn & 1]))
                        turn += 1
            self._check(self.api.realign_end(self.ctx, byref(stats)))
            for path in paths:
                os.rename(path + ".tmp", path)
        except BaseException:
            self.api.realign_end(self.ctx, None)
            for path in paths:
                if os.path.exists(path + ".tmp"):
                    os.remove(path + ".tmp")
            raise
        return realign_stats_of(stats)

    def rna_metrics(self, rrna_intervals_file=None):
        """--rna-metrics: the alignment QC counters of the records of the last read_chimeric_alignments, summed on the device from the record stream that is still in HBM
        (agpu_rna_metrics) against the region track of the session for `rrna_intervals_file` (BED; None: no rRNA intervals), which is built when first asked for.
        Valid after read_chimeric_alignments and before the next one.  Returns (counters, stats): a uint64 array of _capi.RNA_METRICS_WORDS words -- the scalars of "## METRICS" in
        file order, two statistics, the MAPQ, insert-size and gene-body bins -- and {"records", "base_records", "blocks", "segments", "track_runs", "peak_bytes", "seconds"}."""
        if not self.device_ingest or not hasattr(self.api, "rna_metrics"):
            raise ArribaError("ERROR: rna metrics need the record stream of an ingest on the device (DevicePipeline(bam=...))")
        lib, handle = self.session._lib, self.session._session
        contigs, track = _capi.DepthContigs(), _capi.RegionTrack()
        if lib.ahost_region_track(handle, rrna_intervals_file.encode() if rrna_intervals_file else None, byref(track), None) != 0 or lib.ahost_depth_contigs_of_session(handle, byref(contigs)) != 0:
            raise ArribaError("ERROR: " + lib.ahost_last_error().decode())
        counters, stats = np.zeros(_capi.RNA_METRICS_WORDS, dtype=np.uint64), _capi.RnaMetricsStats()
        self._check(self.api.rna_metrics(self.ctx, byref(track), contigs.length, contigs.n_ref, counters.ctypes.data, byref(stats)))
        return counters, rna_metrics_stats_of(stats)

    def write_rna_metrics(self, path, rrna_intervals_file=None):
        """--rna-metrics: the counters of `rna_metrics` as the text of the table, written through `path`.tmp; returns the statistics"""
        lib = self.session._lib
        counters, stats = self.rna_metrics(rrna_intervals_file)  # (refused before anything is written)
        if lib.ahost_rna_metrics_write(counters.ctypes.data, counters.size, path.encode()) != 0:
            raise ArribaError("ERROR: " + lib.ahost_last_error().decode())
        return stats

    def rna_metrics_allocated_bytes(self):
        count = c_uint64()
        self._check(self.api.rna_metrics_allocated_bytes(self.ctx, byref(count)))
        return int(count.value)

    def realign_allocated_bytes(self):
        count = c_uint64()
        self._check(self.api.realign_allocated_bytes(self.ctx, byref(count)))
        return int(count.value)

    def _free_depth_windows(self):
        if getattr(self, "_depth_windows", None) is not None:
            for buffer in self._depth_windows[1]:
                if buffer:
                    self.api.host_free(buffer)
            self._depth_windows = None

    def depth_allocated_bytes(self):
        count = c_uint64()
        self._check(self.api.depth_allocated_bytes(self.ctx, byref(count)))
        return int(count.value)

    def virus_allocated_bytes(self):
        count = c_uint64()
        self._check(self.api.virus_allocated_bytes(self.ctx, byref(count)))
        return int(count.value)

    def release_support_pool(self):
        self._check(self.api.support_pool_release(self.ctx))

    def markdup_allocated_bytes(self):
        """bytes of the "markdup.*" buffers of the context: 0 outside write_sorted_bam, and always when --mark-duplicates is off"""
        count = c_uint64()
        self._check(self.api.markdup_allocated_bytes(self.ctx, byref(count)))
        return int(count.value)

    def sorted_bam_compression_allocated_bytes(self):
        """bytes of the device buffers that only --sorted-bam-compression 1 has: 0 as long as it was never used"""
        count = c_uint64()
        self._check(self.api.sorted_bam_compression_allocated_bytes(self.ctx, byref(count)))
        return int(count.value)

    def support_allocated_bytes(self):
        count = c_uint64()
        self._check(self.api.support_allocated_bytes(self.ctx, byref(count)))
        return int(count.value)

    def written_fusion_rows(self):
        """the data rows of the fusions file written last (not the discarded one) as the rows of write_supporting_alignments: {"ref" [n, 2], "breakpoint" [n, 2], "name_begin" [n + 1],
        "names"}: per row the references and 0-based positions of columns 5 and 6, and the fragments of its read_identifiers (the host writer's rows and the read lists of their candidates)"""
        lib, handle = self.session._lib, self.session._session
        n_rows, candidate, ref, breakpoint = c_uint32(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        if lib.ahost_written_fusion_rows(handle, byref(n_rows), byref(candidate), byref(ref), byref(breakpoint)) != 0:
            raise ArribaError("ERROR: " + lib.ahost_last_error().decode())
        n = n_rows.value
        if getattr(self, "_written_lists", None) is None:
            raise ArribaError("ERROR: no fusions file has been written by this pipeline")
        list_offset, read_lists = self._written_lists
        take = lambda pointer, count, dtype: np.ctypeslib.as_array(ctypes.cast(pointer, ctypes.POINTER(dtype)), (count,)).copy() if count else np.zeros(0, dtype)
        candidates = take(candidate, n, ctypes.c_uint32)
        begins, ends = list_offset[3 * candidates.astype(np.int64)], list_offset[3 * candidates.astype(np.int64) + 3]
        name_begin = np.zeros(n + 1, np.uint64)
        name_begin[1:] = np.cumsum(ends - begins, dtype=np.uint64)
        names = np.concatenate([read_lists[int(b):int(e)] for b, e in zip(begins, ends)] + [np.zeros(0, np.uint32)]).astype(np.uint32)
        return {"ref": take(ref, 2 * n, ctypes.c_int32).reshape(n, 2), "breakpoint": take(breakpoint, 2 * n, ctypes.c_int32).reshape(n, 2), "name_begin": name_begin, "names": names}

    def write_supporting_alignments(self, prefix, rows=None, window=1000000):
        """Phase 2 of --supporting-alignments: `prefix`_ID.bam and `prefix`_ID.bam.bai for every row (ID = 1-based rank), with the records of the pool whose QNAME the row lists and that
        overlap one of its two windows -- what scripts/extract_fusion-supporting_alignments.sh of the reference gets from samtools (agpu_supporting_*).  rows: {"ref" [n, 2],
        "breakpoint" [n, 2] 0-based, "name_begin" [n + 1], "names": entries of the names the pool was built from}; None: the rows of the fusions file written last.  Written
        through *.tmp; on a failure nothing of the prefix is left behind.  Returns {"rows", "records", "uncompressed_bytes", "file_bytes", "blocks", "windows", "indexed"}."""
        import time
        if not hasattr(self.api, "supporting_begin"):
            raise ArribaError("ERROR: the device library has no agpu_supporting_begin")
        if rows is None:
            rows = self.written_fusion_rows()
        lib, handle = self.session._lib, self.session._session
        ref = np.ascontiguousarray(rows["ref"], dtype=np.int32).reshape(-1)
        breakpoint = np.ascontiguousarray(rows["breakpoint"], dtype=np.int32).reshape(-1)
        name_begin = np.ascontiguousarray(rows["name_begin"], dtype=np.uint64)
        names = np.ascontiguousarray(rows["names"], dtype=np.uint32)
        n_rows = ref.size // 2
        if breakpoint.size != ref.size or name_begin.size != n_rows + 1 or (n_rows and int(name_begin[-1]) != names.size):
            raise ArribaError("ERROR: the rows of the supporting alignments do not fit together")
        view = _capi.SupportingRows(n_rows, ref.ctypes.data, breakpoint.ctypes.data, name_begin.ctypes.data, names.ctypes.data if names.size else None)
        started = time.perf_counter()
        info = _capi.SupportingInfo()
        self._check(self.api.supporting_begin(self.ctx, byref(view), int(window), byref(info)))  # (refused before anything is written: no pool)
        seconds = {"join": time.perf_counter() - started, "gather_and_copy": 0.0, "write": 0.0, "index": 0.0}
        writer = None
        try:
            framed, framed_bytes, lengths, n_ref = ctypes.c_void_p(), c_uint64(), ctypes.c_void_p(), ctypes.c_uint32()
            if lib.ahost_sorted_bam_header(handle, byref(framed), byref(framed_bytes), byref(lengths), byref(n_ref)) != 0:
                raise ArribaError("ERROR: " + lib.ahost_last_error().decode())
            ref_length = np.ctypeslib.as_array(ctypes.cast(lengths, ctypes.POINTER(ctypes.c_uint32)), (n_ref.value,)).copy() if n_ref.value else np.zeros(0, np.uint32)
            row_bytes = np.zeros(max(n_rows, 1), np.uint64)
            self._check(self.api.supporting_row_bytes(self.ctx, row_bytes.ctypes.data))
            writer = lib.ahost_supporting_writer_open(prefix.encode(), framed, framed_bytes.value, n_rows, row_bytes.ctypes.data)
            if not writer:
                raise ArribaError("ERROR: " + lib.ahost_last_error().decode())
            if getattr(self, "_sorted_windows", None) is None or self._sorted_windows[0] < info.window_bytes:  # (the two pinned buffers of --sorted-bam serve here as well)
                self._free_sorted_windows()
                buffers = [self.api.host_alloc(info.window_bytes) for _ in range(2)]
                self._sorted_windows = (info.window_bytes, buffers)
                if not all(buffers):
                    self._free_sorted_windows()
                    raise ArribaError("ERROR: " + self.api.last_error().decode())
            capacity, buffers = self._sorted_windows
            got, turn, written = c_uint64(), 0, 0
            while True:
                before = time.perf_counter()
                self._check(self.api.supporting_next(self.ctx, buffers[turn & 1], capacity, byref(got)))
                middle = time.perf_counter()
                seconds["gather_and_copy"] += middle - before
                if got.value == 0:
                    break
                if lib.ahost_supporting_writer_push(writer, buffers[turn & 1], got.value) != 0:
                    raise ArribaError("ERROR: " + lib.ahost_last_error().decode())
                seconds["write"] += time.perf_counter() - middle
                written += got.value
                turn += 1
            if written != info.file_bytes:
                raise ArribaError("ERROR: the record blocks of the supporting alignments have %d bytes, %d were announced" % (written, info.file_bytes))
            indexed = bool((ref_length <= self.MAX_BAI_REFERENCE).all())
            before = time.perf_counter()
            index = _capi.SupportingIndex()
            self._check(self.api.supporting_index(self.ctx, framed_bytes.value, byref(index)))
            arrays = {name: np.zeros(max(size, 1), dtype) for name, size, dtype in (("row_first", n_rows + 1, np.uint64), ("ref", index.n_records, np.int32), ("pos", index.n_records, np.int32),
                      ("end_flag", index.n_records, np.uint32), ("bin", index.n_records, np.uint32), ("begin", index.n_records, np.uint64), ("end", index.n_records, np.uint64))}
            for name, array in arrays.items():
                setattr(index, name, array.ctypes.data)
            self._check(self.api.supporting_index(self.ctx, framed_bytes.value, byref(index)))
            if lib.ahost_supporting_writer_index(writer, byref(index), ref_length.ctypes.data if n_ref.value else None, n_ref.value) != 0:
                raise ArribaError("ERROR: " + lib.ahost_last_error().decode())
            seconds["index"] = time.perf_counter() - before
            status, writer = lib.ahost_supporting_writer_close(writer, 1), None
            if status != 0:
                raise ArribaError("ERROR: " + lib.ahost_last_error().decode())
        finally:
            if writer:
                lib.ahost_supporting_writer_close(writer, 0)
            self.api.supporting_end(self.ctx)
        seconds["total"] = time.perf_counter() - started
        self.supporting_seconds = seconds
        return {"rows": int(info.rows), "records": int(info.records), "uncompressed_bytes": int(info.uncompressed_bytes), "file_bytes": int(info.file_bytes), "blocks": int(info.blocks), "windows": int(info.windows), "indexed": indexed}

    def _free_sorted_windows(self):
        if getattr(self, "_sorted_windows", None) is not None:
            for pointer in self._sorted_windows[1]:
                if pointer:
                    self.api.host_free(pointer)
            self._sorted_windows = None

    def batch_rows(self, fragments=None):
        """rows of the batch on the device as numpy arrays (fragments=None: all) -- what agpu_gather_rows_* hands to the host's writer; also the test's view of a batch built on the device"""
        if fragments is not None:
            fragments = np.ascontiguousarray(fragments, dtype=np.uint32)
        sizes = [c_uint64(), c_uint64(), c_uint64()]
        n = self.n if fragments is None else fragments.size
        self._check(self.api.gather_rows_begin(self.ctx, None if fragments is None else fragments.ctypes.data, n, byref(sizes[0]), byref(sizes[1]), byref(sizes[2])))
        rows = _capi.BatchRows()
        arrays = {"n_aln": np.zeros(max(n, 1), np.uint8), "fbits": np.zeros(max(n, 1), np.uint8), "group": np.zeros(max(n, 1), np.uint32),
                  "cigar_pool": np.zeros(max(sizes[0].value, 1), np.uint32), "seq_pool": np.zeros(max(sizes[1].value, 4), np.uint8), "name_offset": np.zeros(n + 1, np.uint32), "names": np.zeros(max(sizes[2].value, 1), np.uint8)}
        for slot in range(3):
            for name, dtype in (("contig", np.uint16), ("start", np.int32), ("end", np.int32), ("abits", np.uint8), ("cigar_offset", np.uint32), ("cigar_count", np.uint16)):
                arrays["%s%d" % (name, slot)] = np.zeros(max(n, 1), dtype)
                getattr(rows, name)[slot] = arrays["%s%d" % (name, slot)].ctypes.data
        for slot in range(2):
            for name in ("seq_offset", "seq_length"):
                arrays["%s%d" % (name, slot)] = np.zeros(max(n, 1), np.uint32)
                getattr(rows, name)[slot] = arrays["%s%d" % (name, slot)].ctypes.data
        for name in ("n_aln", "fbits", "group", "cigar_pool", "seq_pool", "name_offset", "names"):
            setattr(rows, name, arrays[name].ctypes.data)
        self._check(self.api.gather_rows_copy(self.ctx, byref(rows)))
        arrays["n"] = n
        arrays["cigar_pool"] = arrays["cigar_pool"][:rows.cigar_pool_size]; arrays["seq_pool"] = arrays["seq_pool"][:rows.seq_pool_size]; arrays["names"] = arrays["names"][:rows.names_size]
        for key in list(arrays):
            if key not in ("n", "cigar_pool", "seq_pool", "names", "name_offset"):
                arrays[key] = arrays[key][:n]
        return arrays, rows

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, status):
        if status != 0:
            raise ArribaError("ERROR: " + self.api.last_error().decode() + " (status %d)" % status)

    def _record(self, stage):
        import time
        now = time.perf_counter()
        self.wall_ms[stage] = self.wall_ms.get(stage, 0.0) + (now - self._last_record) * 1e3  # host wall time since the previous stage ended
        self._last_record = now
        ms, size = c_float(), c_uint64()
        self.api.last_kernel_ms(self.ctx, byref(ms))
        self.api.last_kernel_bytes(self.ctx, byref(size))
        self.timings[stage] = {"ms": ms.value, "bytes": size.value}

    def reset(self):
        """back to the state right after the upload (for repeated timed passes over the same resident batch)"""
        self._check(self.api.reset(self.ctx))
        self._record("reset")
        self.n_dummy_genes = 0

    # ---- stages, named after the reference functions they replace ---------------------------------

    def mark_multimappers(self):
        marked = c_uint64()
        self._check(self.api.mark_multimappers(self.ctx, byref(marked)))
        self._record("mark_multimappers")
        return marked.value

    def detect_strandedness(self):
        """reference: detect_strandedness, source/read_stats.cpp:94-143 -- on the host's batch, or on the device when the batch was built there"""
        if not self.device_ingest:
            return self.session.detect_strandedness()
        verdict = ctypes.c_int()
        self._check(self.api.detect_strandedness(self.ctx, byref(verdict)))
        return verdict.value

    def annotate_alignments(self, strandedness=None):
        if strandedness is None:
            strandedness = self.detect_strandedness()
        self.scalars["strandedness"] = strandedness
        self.params.strandedness = strandedness
        self._check(self.api.set_params(self.ctx, byref(self.params)))
        n_dummy = c_uint32()
        self._check(self.api.annotate(self.ctx, byref(n_dummy)))
        self._record("annotate")
        self.n_dummy_genes = n_dummy.value
        return self.n_dummy_genes

    def filter_duplicates_and_contigs(self, top_viral_contigs=5, viral_contig_min_covered_fraction=0.05):
        count = c_uint64()
        self._check(self.api.get_viral_integration_sites(self.ctx, None, 0, byref(count)))
        pairs = np.zeros(2 * max(count.value, 1), dtype=np.uint32)
        self._check(self.api.get_viral_integration_sites(self.ctx, pairs.ctypes.data, count.value, byref(count)))
        gene_bits = self.gene_table()["bits"]
        top, low = self.session.viral_verdicts(pairs[:2 * count.value], gene_bits, top_viral_contigs, viral_contig_min_covered_fraction)
        self._check(self.api.read_filters_stage1(self.ctx, top.ctypes.data, low.ctypes.data))
        self._record("read_filters_stage1")

    def estimate_fragment_length(self):
        gaps = np.zeros(100001, dtype=np.int32)
        n_samples, visited = c_uint32(), c_uint64()
        self._check(self.api.fragment_length_samples(self.ctx, gaps.ctypes.data, byref(n_samples), byref(visited)))
        self._record("fragment_length_samples")
        if self.device_ingest:
            # the reference's sequential float sum of the read lengths (hazard H4) runs on the host over the lengths of the fragments its loop visited
            count = min(visited.value, self.n)
            lengths = [np.zeros(max(count, 1), dtype=np.uint32), np.zeros(max(count, 1), dtype=np.uint32)]
            self._check(self.api.get_read_lengths(self.ctx, 0, count, lengths[0].ctypes.data, lengths[1].ctypes.data))
            lib = self.session._lib
            total = lib.ahost_read_length_sum_of(c_float(0), lengths[0].ctypes.data, lengths[1].ctypes.data, count)
            samples = np.ascontiguousarray(gaps[:n_samples.value], dtype=np.int32)
            mean, stddev, read_length, max_mate_gap = c_float(), c_float(), c_float(), c_int32()
            estimated = lib.ahost_estimate_fragment_length_from_sums(samples.ctypes.data, samples.size, c_float(total), count, self.params.fragment_length, byref(mean), byref(stddev), byref(read_length), byref(max_mate_gap))
            estimate = {"estimated": bool(estimated), "mate_gap_mean": mean.value, "mate_gap_stddev": stddev.value, "read_length_mean": read_length.value, "max_mate_gap": max_mate_gap.value}
        else:
            estimate = self.session.estimate_fragment_length(gaps[:n_samples.value], visited.value, self.params.fragment_length)
        self.scalars.update(estimate)
        self.scalars["mate_gap_samples"] = n_samples.value
        return estimate

    def filter_reads(self):
        remaining = np.zeros(_capi.FILTER_COUNT, dtype=np.uint64)
        self._check(self.api.read_filters_stage2(self.ctx, remaining.ctypes.data))
        self._record("read_filters_stage2")
        self.remaining = {_capi.FILTER_NAMES[f]: int(remaining[f]) for f in (1, 30, 31, 32, 33, 4, 2, 3, 6, 7, 5, 8, 10, 36)}
        return self.remaining

    def run_read_level(self, strandedness=None, top_viral_contigs=5, viral_contig_min_covered_fraction=0.05):
        """mark_multimappers ... filter_low_entropy (reference: source/arriba.cpp:141-409)."""
        self.scalars["marked_multimappers"] = self.mark_multimappers()
        self.annotate_alignments(strandedness)
        self.filter_duplicates_and_contigs(top_viral_contigs, viral_contig_min_covered_fraction)
        self.estimate_fragment_length()
        return self.filter_reads()

    def run_workflow(self, output_file, discarded_output_file=None, blacklist_file=None, known_fusions_file=None, tags_file=None, protein_domains_file=None, genomic_breakpoints_file=None,
                     max_genomic_breakpoint_distance=100000, strandedness=None, evalue_cutoff=0.3,
                     min_itd_support=10, min_itd_allele_fraction=0.07, high_expression_quantile=0.998, min_spliced_events=4, min_anchor_length=23,
                     max_homolog_identity=0.3, max_itd_length=100, fill_sequence_gaps=False, top_viral_contigs=5, viral_contig_min_covered_fraction=0.05,
                     print_extra_info_for_discarded_fusions=False, log=None, sorted_bam_file=None, supporting_alignments_prefix=None, supporting_alignments_window=1000000, virus_expression_file=None, coverage_file=None, mark_duplicates=False, gene_counts_file=None, splice_junctions_file=None, allele_sites_file=None, allele_counts_file=None, allele_min_mapq=0, allele_min_baseq=13, realign_reads_file=None, realign_kept_file=None, rna_metrics_file=None, rrna_intervals_file=None, variant_sites_file=None, variant_min_mapq=20, variant_min_baseq=13, variant_min_alt=3, variant_min_percent=5, indel_sites_file=None, indel_min_mapq=20, indel_min_alt=3, indel_min_percent=5):
        """The reference's main() behind read_chimeric_alignments (source/arriba.cpp:119-610) with its default parameters: the read-level cascade, find_fusions,
        every candidate-level filter in the reference's order, assign_confidence, and the two output files.  `log` receives (stage, remaining) pairs --
        the numbers the reference prints as "(remaining=N)".  Filters switched off with -f are skipped by the stages themselves (agpu_params.filter_enabled)."""
        note = log if log is not None else (lambda stage, remaining: None)
        if sorted_bam_file:  # first: the record stream is still in HBM (it is given back when the stages need the memory)
            self.write_sorted_bam(sorted_bam_file, mark_duplicates=mark_duplicates)
        elif mark_duplicates:
            raise ArribaError("ERROR: --mark-duplicates needs --sorted-bam: the marks are written into the sorted BAM file")
        if virus_expression_file:  # (--virus-expression: likewise from the stream)
            self.write_virus_expression(virus_expression_file)
        if coverage_file:  # (--coverage: likewise)
            self.write_coverage(coverage_file)
        if gene_counts_file:  # (--gene-counts: likewise)
            self.write_gene_counts(gene_counts_file)
        if splice_junctions_file:  # (--splice-junctions: likewise)
            self.write_splice_junctions(splice_junctions_file)
        if allele_sites_file or allele_counts_file:  # (--allele-counts: likewise)
            if not (allele_sites_file and allele_counts_file):
                raise ArribaError("ERROR: --allele-sites and --allele-counts need each other")
            self.write_allele_counts(allele_sites_file, allele_counts_file, allele_min_mapq, allele_min_baseq)
        if realign_reads_file or realign_kept_file:  # (--realign-reads: likewise)
            if not realign_reads_file:
                raise ArribaError("ERROR: --realign-kept needs --realign-reads")
            self.realign_split(realign_reads_file, realign_kept_file)
        if rna_metrics_file or rrna_intervals_file:  # (--rna-metrics: likewise)
            if not rna_metrics_file:
                raise ArribaError("ERROR: --rrna-intervals needs --rna-metrics")
            self.write_rna_metrics(rna_metrics_file, rrna_intervals_file)
        if not variant_sites_file and (variant_min_mapq, variant_min_baseq, variant_min_alt, variant_min_percent) != (20, 13, 3, 5):
            raise ArribaError("ERROR: --variant-min-alt, --variant-min-percent, --variant-min-mapq and --variant-min-baseq need --variant-sites: the file the sites go to")
        if variant_sites_file:  # (--variant-sites: likewise)
            self.write_variant_sites(variant_sites_file, variant_min_mapq, variant_min_baseq, variant_min_alt, variant_min_percent)
        if not indel_sites_file and (indel_min_mapq, indel_min_alt, indel_min_percent) != (20, 3, 5):
            raise ArribaError("ERROR: --indel-min-alt, --indel-min-percent and --indel-min-mapq need --indel-sites: the file the indels go to")
        if indel_sites_file:  # (--indel-sites: likewise)
            self.write_indel_sites(indel_sites_file, indel_min_mapq, indel_min_alt, indel_min_percent)
        if supporting_alignments_prefix:  # (--supporting-alignments, phase 1: the records of the names of the batch leave the stream while it is there)
            self.build_support_pool()
        self.run_read_level(strandedness, top_viral_contigs, viral_contig_min_covered_fraction)
        note("find_fusions", self.find_fusions())
        self.upload_coverage()
        if genomic_breakpoints_file:
            note("mark_genomic_support", self.mark_genomic_support(genomic_breakpoints_file, max_genomic_breakpoint_distance))
        note("merge_adjacent_fusions", self.merge_adjacent_fusions())
        note("filter_multimappers", self.filter_multimappers()[0])
        self.estimate_expected_fusions()
        self.filter_candidate_predicates()
        note("filter_relative_support", self.filter_relative_support())
        note("recover_internal_tandem_duplication", self.recover_internal_tandem_duplication(min_itd_support, min_itd_allele_fraction))
        note("filter_both_intronic", self.filter_both_intronic())
        if known_fusions_file:
            note("recover_known_fusions", self.recover_known_fusions(known_fusions_file))
        note("filter_in_vitro", self.filter_in_vitro(high_expression_quantile))
        note("recover_both_spliced", self.recover_both_spliced())
        note("select_most_supported_breakpoints", self.select_most_supported_breakpoints())
        note("filter_marginal_read_through", self.filter_marginal_read_through())
        note("recover_many_spliced", self.recover_many_spliced(min_spliced_events))
        if genomic_breakpoints_file:
            self.assign_confidence()  # filter_no_genomic_support looks at the confidence (source/arriba.cpp:516-523)
            note("filter_no_genomic_support", self.filter_no_genomic_support())
        if blacklist_file:
            note("filter_blacklisted_ranges", self.filter_blacklisted_ranges(blacklist_file, evalue_cutoff))
        note("filter_short_anchor", self.filter_short_anchor(min_anchor_length))
        note("filter_end_to_end", self.filter_end_to_end())
        note("filter_no_coverage", self.filter_no_coverage())
        self.make_kmer_index()
        note("filter_homologs", self.filter_homologs(max_homolog_identity))
        note("filter_mismappers", self.filter_mismappers()[0])
        if genomic_breakpoints_file:
            note("recover_genomic_support", self.recover_genomic_support())
        note("select_most_supported_breakpoints", self.select_most_supported_breakpoints())
        note("recover_isoforms", self.recover_isoforms())
        if tags_file:
            self.session.load_tags(tags_file)
        if protein_domains_file:
            self.session.load_protein_domains(protein_domains_file)
        self.write_fusions(output_file, discarded=False, max_itd_length=max_itd_length, fill_sequence_gaps=fill_sequence_gaps)
        if supporting_alignments_prefix:  # (phase 2: the rows of the file are fixed)
            self.write_supporting_alignments(supporting_alignments_prefix, None, supporting_alignments_window)
            self.release_support_pool()
        if discarded_output_file:
            self.write_fusions(discarded_output_file, discarded=True, print_extra_info=print_extra_info_for_discarded_fusions, max_itd_length=max_itd_length, fill_sequence_gaps=fill_sequence_gaps)

    def find_fusions(self, max_mate_gap=None):
        """reference: find_fusions, source/fusions.cpp:203-473; returns the number of candidates"""
        if max_mate_gap is None:
            max_mate_gap = self.scalars["max_mate_gap"]
        count = c_uint64()
        self._check(self.api.find_fusions(self.ctx, max_mate_gap, byref(count)))
        self._record("find_fusions")
        self.n_candidates = count.value
        return self.n_candidates

    def candidates(self, lists=True):
        """Candidate table in the reference's insertion order; lists as (offset[3n+1], reads).  lists=False: the columns only."""
        n = self.n_candidates
        u32 = lambda: np.zeros(max(n, 1), dtype=np.uint32)
        i32 = lambda: np.zeros(max(n, 1), dtype=np.int32)
        table = {"gene1": u32(), "gene2": u32(), "contigs": u32(), "breakpoint1": i32(), "breakpoint2": i32(), "flags": u32(), "filter": np.zeros(max(n, 1), dtype=np.uint8),
                 "split_reads1": u32(), "split_reads2": u32(), "discordant_mates": u32(), "anchor_start1": i32(), "anchor_start2": i32(), "list_offset": np.zeros(3 * n + 1, dtype=np.uint64)}
        order = ["gene1", "gene2", "contigs", "breakpoint1", "breakpoint2", "flags", "filter", "split_reads1", "split_reads2", "discordant_mates", "anchor_start1", "anchor_start2", "list_offset"]
        self._check(self.api.get_candidates(self.ctx, *[table[k].ctypes.data if (lists or k != "list_offset") else None for k in order]))
        if not lists:
            for key in order[:-1]:
                table[key] = table[key][:n]
            del table["list_offset"]
            return table
        total = c_uint64()
        self._check(self.api.get_candidate_read_lists(self.ctx, None, 0, byref(total)))
        reads = np.zeros(max(total.value, 1), dtype=np.uint32)
        self._check(self.api.get_candidate_read_lists(self.ctx, reads.ctypes.data, total.value, byref(total)))
        for key in order[:-1]:
            table[key] = table[key][:n]
        table["read_lists"] = reads[:total.value]
        return table

    def selected_candidates(self, discarded=False):
        """the candidates an output file holds (-o: filter == none, -O: the others), picked on the device with the columns the writer prints (agpu_select_candidates)"""
        count = c_uint64()
        self._check(self.api.select_candidates(self.ctx, int(discarded), byref(count)))
        n = count.value
        dtypes = {"candidate": np.uint32, "gene1": np.uint32, "gene2": np.uint32, "contigs": np.uint32, "breakpoint1": np.int32, "breakpoint2": np.int32, "flags": np.uint32, "filter": np.uint8, "split_reads1": np.uint32,
                  "split_reads2": np.uint32, "discordant_mates": np.uint32, "evalue": np.float32, "confidence": np.uint8, "iteration_rank": np.uint32, "closest_genomic_breakpoint1": np.int32, "closest_genomic_breakpoint2": np.int32}
        columns = {key: np.zeros(max(n, 1), dtype=dtype) for key, dtype in dtypes.items()}
        view = _capi.SelectedCandidates()
        for key, column in columns.items():
            setattr(view, key, column.ctypes.data)
        self._check(self.api.get_selected_candidates(self.ctx, byref(view)))
        return {key: column[:n] for key, column in columns.items()}

    def filters_of(self, fragments):
        """the filters of the given fragments (agpu_get_filters_of)"""
        fragments = np.ascontiguousarray(fragments, dtype=np.uint32)
        out = np.zeros(max(fragments.size, 1), dtype=np.uint8)
        self._check(self.api.get_filters_of(self.ctx, fragments.ctypes.data if fragments.size else None, fragments.size, out.ctypes.data))
        return out[:fragments.size]

    def candidate_read_lists_of(self, candidates):
        """(list_offset[3n+1] starting at 0, reads) of the given candidates only"""
        candidates = np.ascontiguousarray(candidates, dtype=np.uint32)
        n = candidates.size
        offsets = np.zeros(3 * n + 1, dtype=np.uint64)
        total = c_uint64()
        self._check(self.api.get_candidate_read_lists_of(self.ctx, candidates.ctypes.data if n else None, n, offsets.ctypes.data, None, 0, byref(total)))
        reads = np.zeros(max(total.value, 1), dtype=np.uint32)
        if total.value:
            self._check(self.api.get_candidate_read_lists_of(self.ctx, candidates.ctypes.data, n, offsets.ctypes.data, reads.ctypes.data, total.value, byref(total)))
        return offsets, reads[:total.value]

    def merge_adjacent_fusions(self, max_distance=5):
        """reference: merge_adjacent_fusions, source/merge_adjacent_fusions.cpp:19-108; returns the number of unfiltered candidates"""
        remaining = c_uint64()
        self._check(self.api.merge_adjacent_fusions(self.ctx, max_distance, byref(remaining)))
        self._record("merge_adjacent_fusions")
        return remaining.value

    def filter_multimappers(self):
        """reference: filter_multimappers, source/filter_multimappers.cpp:109-221; returns (remaining candidates, fragments discarded)"""
        remaining, discarded = c_uint64(), c_uint64()
        self._check(self.api.filter_multimappers(self.ctx, byref(remaining), byref(discarded)))
        self._record("filter_multimappers")
        return remaining.value, discarded.value

    # event-level predicates behind filter_relative_support (each returns the reference's "(remaining=N)")
    def upload_coverage(self):
        if self.device_ingest:
            return  # coverage_t was built on the device
        view = self.session._lib.ahost_coverage_view(self.session._session)
        if not view:
            raise ArribaError("ERROR: " + self.session._lib.ahost_last_error().decode())
        self._check(self.api.upload_coverage(self.ctx, view))

    def _event_stage(self, name, *arguments):
        remaining = c_uint64()
        self._check(getattr(self.api, name)(self.ctx, *arguments, byref(remaining)))
        self._record(name)
        return remaining.value

    def recover_internal_tandem_duplication(self, min_supporting_reads=10, min_fraction_of_coverage=0.07):
        """reference: recover_internal_tandem_duplication, source/recover_internal_tandem_duplication.cpp:11-85 (-Z, -z)"""
        return self._event_stage("recover_internal_tandem_duplication", min_supporting_reads, c_float(min_fraction_of_coverage))

    def filter_both_intronic(self):
        """reference: filter_both_intronic, source/filter_both_intronic.cpp:18-36"""
        return self._event_stage("filter_both_intronic")

    def filter_short_anchor(self, min_length=23):
        """reference: filter_short_anchor, source/filter_short_anchor.cpp:7-24 (-A, default 23)"""
        return self._event_stage("filter_short_anchor", min_length)

    def filter_end_to_end(self):
        """reference: filter_end_to_end_fusions, source/filter_end_to_end.cpp:28-78"""
        return self._event_stage("filter_end_to_end")

    def filter_no_coverage(self):
        """reference: filter_no_coverage, source/filter_no_coverage.cpp:9-103"""
        return self._event_stage("filter_no_coverage")

    def select_most_supported_breakpoints(self):
        """reference: select_most_supported_breakpoints, source/select_best.cpp:21-80"""
        return self._event_stage("select_most_supported_breakpoints")

    def filter_in_vitro(self, high_expression_quantile=0.998):
        """reference: filter_in_vitro, source/filter_in_vitro.cpp:82-228 (-Q, default 0.998)"""
        return self._event_stage("filter_in_vitro", c_float(high_expression_quantile))

    def recover_both_spliced(self, max_fusions_to_recover=200, high_expression_quantile=0.998, max_exon_size=1000, max_coverage=1000):
        """reference: recover_both_spliced, source/recover_both_spliced.cpp:72-182 (the arguments of the call at source/arriba.cpp:491)"""
        return self._event_stage("recover_both_spliced", max_fusions_to_recover, c_float(high_expression_quantile), max_exon_size, max_coverage)

    def load_range_rules(self, path, allow_keywords):
        """a blacklist (allow_keywords=True) or known-fusions file -> (pointer to rules, count); reference: parse_blacklist_item, source/filter_blacklisted_ranges.cpp:83-118"""
        rules, count = POINTER(_capi.RangeRule)(), c_uint32()
        if self.session._lib.ahost_load_range_rules(self.session._session, path.encode(), int(allow_keywords), byref(rules), byref(count)) != 0:
            raise ArribaError("ERROR: " + self.session._lib.ahost_last_error().decode())
        return rules, count.value

    def filter_blacklisted_ranges(self, path, evalue_cutoff=0.3, max_mate_gap=None):
        """reference: filter_blacklisted_ranges, source/filter_blacklisted_ranges.cpp:227-301 (-b)"""
        rules, count = self.load_range_rules(path, True)
        gap = int(self.scalars["max_mate_gap"] if max_mate_gap is None else max_mate_gap)
        return self._event_stage("filter_blacklisted_ranges", rules, count, c_float(evalue_cutoff), gap)

    def recover_known_fusions(self, path, max_mate_gap=None):
        """reference: recover_known_fusions, source/recover_known_fusions.cpp:14-100 (-k)"""
        rules, count = self.load_range_rules(path, False)
        gap = int(self.scalars["max_mate_gap"] if max_mate_gap is None else max_mate_gap)
        return self._event_stage("recover_known_fusions", rules, count, gap)

    def write_fusions(self, path, discarded=False, print_extra_info=None, max_itd_length=100, fill_sequence_gaps=False, detached=False):
        """reference: write_fusions_to_file, source/output_fusions.cpp:1043-1261 (-o / -O); the device's results are fetched and formatted by the host library.
        detached: the way the C++ session writes the last file of a sample beside the next sample -- what the writer reads of the sample leaves the host session first
        (ahost_detach_sample), which then holds no sample until its next ingest"""
        if print_extra_info is None:
            print_extra_info = not discarded
        import time
        marks = [("start", time.perf_counter())]
        mark = lambda name: marks.append((name, time.perf_counter()))
        # only the candidates the file will hold travel to the host with their read lists (fusions.tsv: the few thousand that passed every filter, of millions);
        # discarded.tsv counts the discarded reads of every discarded candidate by filter, so it takes the lists of all of them
        table = self.candidates(lists=False)
        mark("candidate columns")
        written = np.flatnonzero((table["filter"] != 0) if discarded else (table["filter"] == 0)).astype(np.uint32)
        list_offset, read_lists = self.candidate_read_lists_of(written)
        mark("read lists")
        n = written.size
        columns = {key: np.ascontiguousarray(table[key][written]) for key in ("gene1", "gene2", "contigs", "breakpoint1", "breakpoint2", "flags", "filter", "split_reads1", "split_reads2", "discordant_mates")}
        columns["list_offset"], columns["read_lists"] = list_offset, np.ascontiguousarray(read_lists)
        columns["evalue"] = np.ascontiguousarray(self.evalues()[written], dtype=np.float32)
        columns["confidence"] = np.ascontiguousarray(self.assign_confidence()[written])
        columns["iteration_rank"] = np.ascontiguousarray(self.candidate_iteration_order()[written], dtype=np.uint32)
        mark("evalue, confidence, order")
        columns["read_filter"] = np.ascontiguousarray(self.filters(), dtype=np.uint8)
        mark("read filters")
        columns["closest_genomic_breakpoint1"], columns["closest_genomic_breakpoint2"] = (np.ascontiguousarray(column[written]) for column in self.genomic_support())
        genes = self.gene_table()
        columns["gene_contig"], columns["gene_start"], columns["gene_end"] = (np.ascontiguousarray(genes[key]) for key in ("contig", "start", "end"))
        view = _capi.FusionTable()
        view.n_candidates = n
        view.n_genes = len(columns["gene_contig"])
        for key, column in columns.items():
            setattr(view, key, column.ctypes.data if column.size else None)
        if self.device_ingest and print_extra_info:
            # the host's writer works on the rows of the supporting reads of the candidates it writes: fetched from the device now
            lib = self.session._lib
            count = c_uint64()
            if lib.ahost_fusion_table_reads(byref(view), int(discarded), None, 0, byref(count)) != 0:
                raise ArribaError("ERROR: " + lib.ahost_last_error().decode())
            fragments = np.zeros(max(count.value, 1), dtype=np.uint32)
            if lib.ahost_fusion_table_reads(byref(view), int(discarded), fragments.ctypes.data, count.value, byref(count)) != 0:
                raise ArribaError("ERROR: " + lib.ahost_last_error().decode())
            fragments = fragments[:count.value]
            mark("reads of the table")
            arrays, rows = self.batch_rows(fragments)
            mark("rows from the device")
            if lib.ahost_set_batch_rows(self.session._session, byref(rows), fragments.ctypes.data if fragments.size else None) != 0:
                raise ArribaError("ERROR: " + lib.ahost_last_error().decode())
            mark("rows into the session")
        self._emit_fusions(view, path, discarded, print_extra_info, max_itd_length, fill_sequence_gaps, detached)
        if not discarded:
            self._written_lists = (np.asarray(list_offset), np.asarray(read_lists))  # (for written_fusion_rows: the fragments of the rows' read_identifiers)
        mark("ahost_write_fusions")
        self.writer_seconds = {name: round(at - marks[k][1], 4) for k, (name, at) in enumerate(marks[1:])}  # where the time of the output side went (bench.py reports it)

    def _emit_fusions(self, view, path, discarded, print_extra_info, max_itd_length, fill_sequence_gaps, detached=False):
        """the rows of the file from the table of the candidates it holds (the host library's writer)"""
        if detached:
            lib = self.session._lib
            sample = lib.ahost_detach_sample(self.session._session)
            if not sample:
                raise ArribaError("ERROR: " + lib.ahost_last_error().decode())
            status = lib.ahost_write_fusions_of(sample, byref(view), path.encode(), int(discarded), int(print_extra_info), max_itd_length, int(self.scalars["max_mate_gap"]), int(fill_sequence_gaps))
            message = lib.ahost_last_error().decode() if status != 0 else ""
            lib.ahost_release_sample(sample)
            if status != 0:
                raise ArribaError("ERROR: " + message)
            return
        if self.session._lib.ahost_write_fusions(self.session._session, byref(view), path.encode(), int(discarded), int(print_extra_info), max_itd_length, int(self.scalars["max_mate_gap"]), int(fill_sequence_gaps)) != 0:
            raise ArribaError("ERROR: " + self.session._lib.ahost_last_error().decode())

    def mark_genomic_support(self, path, max_distance=100000):
        """reference: mark_genomic_support, source/filter_genomic_support.cpp:81-219 (-d, -D); returns the number of candidates with a supporting structural variant"""
        variants, count, marked = POINTER(_capi.GenomicBreakpoint)(), c_uint32(), c_uint64()
        if self.session._lib.ahost_load_genomic_breakpoints(self.session._session, path.encode(), byref(variants), byref(count)) != 0:
            raise ArribaError("ERROR: " + self.session._lib.ahost_last_error().decode())
        self._check(self.api.mark_genomic_support(self.ctx, variants, count.value, max_distance, byref(marked)))
        self._record("mark_genomic_support")
        return marked.value

    def genomic_support(self):
        """closest genomic breakpoints of every candidate (-1 = none)"""
        closest1, closest2 = np.zeros(max(self.n_candidates, 1), dtype=np.int32), np.zeros(max(self.n_candidates, 1), dtype=np.int32)
        self._check(self.api.get_genomic_support(self.ctx, closest1.ctypes.data, closest2.ctypes.data))
        return closest1[:self.n_candidates], closest2[:self.n_candidates]

    def filter_no_genomic_support(self):
        """reference: filter_no_genomic_support, source/filter_genomic_support.cpp:401-417 (behind assign_confidence)"""
        return self._event_stage("filter_no_genomic_support")

    def recover_genomic_support(self):
        """reference: recover_genomic_support, source/filter_genomic_support.cpp:419-444"""
        return self._event_stage("recover_genomic_support")

    def assign_confidence(self):
        """reference: assign_confidence, source/filter_genomic_support.cpp:222-399; returns the confidence (0 low, 1 medium, 2 high) of every candidate"""
        confidence = np.zeros(max(self.n_candidates, 1), dtype=np.uint8)
        self._check(self.api.assign_confidence(self.ctx, confidence.ctypes.data))
        self._record("assign_confidence")
        return confidence[:self.n_candidates]

    def recover_isoforms(self):
        """reference: recover_isoforms, source/recover_isoforms.cpp:10-47"""
        return self._event_stage("recover_isoforms")

    def filter_homologs(self, max_identity_fraction=0.3):
        """reference: filter_homologs, source/filter_homologs.cpp:68-141 (-L, default 0.3); after make_kmer_index"""
        return self._event_stage("filter_homologs", c_float(max_identity_fraction))

    def recover_many_spliced(self, min_spliced_events=4):
        """reference: recover_many_spliced, source/recover_many_spliced.cpp:8-51 (-M, default 4)"""
        return self._event_stage("recover_many_spliced", min_spliced_events)

    def filter_marginal_read_through(self):
        """reference: filter_marginal_read_through, source/filter_marginal_read_through.cpp:8-46"""
        return self._event_stage("filter_marginal_read_through")

    def candidate_iteration_order(self):
        """rank of every candidate in the iteration order of the reference's fusions_t (hazard H2), computed on the device"""
        rank = np.zeros(max(self.n_candidates, 1), dtype=np.uint32)
        self._check(self.api.candidate_iteration_order(self.ctx, rank.ctypes.data))
        self._record("candidate_iteration_order")
        return rank[:self.n_candidates]

    def candidate_iteration_order_on_host(self, table=None):
        """the same order from the literal std::unordered_map of the host library (the check of the device computation)"""
        table = table if table is not None else self.candidates()
        rank = np.zeros(max(self.n_candidates, 1), dtype=np.uint32)
        columns = [np.ascontiguousarray(table[k]) for k in ("gene1", "gene2", "contigs", "breakpoint1", "breakpoint2", "flags")]
        if _capi.host_library().ahost_candidate_iteration_order(self.n_candidates, *[c.ctypes.data for c in columns], rank.ctypes.data) != 0:
            raise ArribaError("ERROR: " + _capi.host_library().ahost_last_error().decode())
        return rank[:self.n_candidates]

    def set_candidate_state(self, filter=None, split_reads1=None, split_reads2=None, discordant_mates=None):
        """push the columns an event-level host stage changed (reference: merge_adjacent_fusions, filter_multimappers)"""
        arrays = [None if a is None else np.ascontiguousarray(a, dtype=t) for a, t in ((filter, np.uint8), (split_reads1, np.uint32), (split_reads2, np.uint32), (discordant_mates, np.uint32))]
        self._check(self.api.set_candidate_state(self.ctx, *[None if a is None else a.ctypes.data for a in arrays]))

    def estimate_expected_fusions(self, mapped_reads=None, iteration_rank=None):
        """reference: estimate_expected_fusions, source/filter_relative_support.cpp:17-207; returns the e-values (float32)"""
        if mapped_reads is None:
            mapped_reads = self.session.mapped_reads
        if iteration_rank is None:
            self._check(self.api.candidate_iteration_order(self.ctx, None))
            self._record("candidate_iteration_order")
            pointer = None
        else:
            iteration_rank = np.ascontiguousarray(iteration_rank, dtype=np.uint32)
            pointer = iteration_rank.ctypes.data
        self._check(self.api.estimate_expected_fusions(self.ctx, mapped_reads, pointer))
        self._record("estimate_expected_fusions")
        evalue = np.zeros(max(self.n_candidates, 1), dtype=np.float32)
        self._check(self.api.get_evalues(self.ctx, evalue.ctypes.data))
        return evalue[:self.n_candidates]

    def evalues(self):
        """the e-value of every candidate (after estimate_expected_fusions)"""
        evalue = np.zeros(max(self.n_candidates, 1), dtype=np.float32)
        self._check(self.api.get_evalues(self.ctx, evalue.ctypes.data))
        return evalue[:self.n_candidates]

    def filter_candidate_predicates(self):
        """reference: filter_non_coding_neighbors, filter_intragenic_both_exonic, filter_min_support (source/arriba.cpp:437-455);
        returns the number of candidates each of the three discarded"""
        discarded = np.zeros(3, dtype=np.uint64)
        self._check(self.api.filter_candidate_predicates(self.ctx, discarded.ctypes.data))
        self._record("filter_candidate_predicates")
        return {"non_coding_neighbors": int(discarded[0]), "intragenic_exonic": int(discarded[1]), "min_support": int(discarded[2])}

    def filter_relative_support(self):
        remaining = c_uint64()
        self._check(self.api.filter_relative_support(self.ctx, byref(remaining)))
        self._record("filter_relative_support")
        return remaining.value

    def set_read_filters(self, filters):
        """push the read-level filter ids a host stage changed (reference: filter_multimappers)"""
        filters = np.ascontiguousarray(filters, dtype=np.uint8)
        assert filters.size == self.n
        self._check(self.api.set_read_filters(self.ctx, filters.ctypes.data))

    def make_kmer_index(self, padding=None):
        """reference: make_kmer_index, source/filter_mismappers.cpp:47-84; padding as in source/arriba.cpp:552"""
        if padding is None:
            padding = int(np.float32(self.scalars["max_mate_gap"]) + np.float32(2) * np.float32(self.scalars["read_length_mean"]))
        positions = c_uint64()
        self._check(self.api.make_kmer_index(self.ctx, padding, byref(positions)))
        self._record("make_kmer_index")
        return positions.value

    def filter_mismappers(self, max_mate_gap=None):
        """reference: filter_mismappers, source/filter_mismappers.cpp:272-359; returns (remaining candidates, reads discarded)"""
        if max_mate_gap is None:
            max_mate_gap = self.scalars["max_mate_gap"]
        remaining, discarded = c_uint64(), c_uint64()
        self._check(self.api.filter_mismappers(self.ctx, max_mate_gap, byref(remaining), byref(discarded)))
        self._record("filter_mismappers")
        return remaining.value, discarded.value

    def fusion_stats(self):
        stats = np.zeros(5, dtype=np.uint64)
        self._check(self.api.get_fusion_stats(self.ctx, stats.ctypes.data))
        return dict(zip(("emissions", "candidates", "list_entries", "discordant_emissions", "wave_buckets"), (int(v) for v in stats)))

    def set_profiling(self, enabled):
        """per-kernel HIP-event timing on the launch stream (reset on every call)"""
        self._check(self.api.set_profiling(self.ctx, int(enabled)))
        self._profiling_on = bool(enabled)

    def kernel_profile(self):
        """[(kernel name, ms, algorithmic bytes)] for every launch since set_profiling(True)"""
        count = c_uint32()
        self._check(self.api.get_kernel_profile(self.ctx, None, None, None, 0, byref(count)))
        n = count.value
        names = ctypes.create_string_buffer(max(n, 1) * _capi.KERNEL_NAME_LENGTH)
        ms = np.zeros(max(n, 1), dtype=np.float32)
        size = np.zeros(max(n, 1), dtype=np.uint64)
        self._check(self.api.get_kernel_profile(self.ctx, names, ms.ctypes.data, size.ctypes.data, n, byref(count)))
        raw = names.raw
        return [(raw[k * _capi.KERNEL_NAME_LENGTH:(k + 1) * _capi.KERNEL_NAME_LENGTH].split(b"\0")[0].decode(), float(ms[k]), int(size[k])) for k in range(n)]

    def discordant_swapped(self):
        out = np.zeros(self.n, dtype=np.uint8)
        self._check(self.api.get_discordant_swapped(self.ctx, out.ctypes.data))
        return out

    # ---- result access -------------------------------------------------------------------------------

    def filters(self):
        out = np.zeros(self.n, dtype=np.uint8)
        self._check(self.api.get_filters(self.ctx, out.ctypes.data))
        return out

    def alignment_bits(self, slot):
        out = np.zeros(self.n, dtype=np.uint8)
        self._check(self.api.get_alignment_bits(self.ctx, slot, out.ctypes.data))
        return out

    def fragment_bits(self):
        out = np.zeros(self.n, dtype=np.uint8)
        self._check(self.api.get_fragment_bits(self.ctx, out.ctypes.data))
        return out

    def gene_sets(self, slot):
        """Returns (count[n], genes[total]) -- CSR of the gene ids annotated to alignment `slot` of every fragment."""
        total = c_uint64()
        count = np.zeros(self.n, dtype=np.uint8)
        self._check(self.api.get_gene_sets(self.ctx, slot, count.ctypes.data, None, 0, byref(total)))
        genes = np.zeros(max(total.value, 1), dtype=np.uint32)
        self._check(self.api.get_gene_sets(self.ctx, slot, count.ctypes.data, genes.ctypes.data, total.value, byref(total)))
        return count, genes[:total.value]

    def gene_table(self):
        total = self.n_real_genes + self.n_dummy_genes
        table = {"contig": np.zeros(total, dtype=np.uint16), "start": np.zeros(total, dtype=np.int32), "end": np.zeros(total, dtype=np.int32),
                 "bits": np.zeros(total, dtype=np.uint8), "exonic_length": np.zeros(total, dtype=np.int32)}
        self._check(self.api.get_gene_table(self.ctx, 0, total, table["contig"].ctypes.data, table["start"].ctypes.data, table["end"].ctypes.data,
                                            table["bits"].ctypes.data, table["exonic_length"].ctypes.data))
        return table
