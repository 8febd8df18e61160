"""Every consumer of the record stream of the last ingest (--sorted-bam, --supporting-alignments, --virus-expression, --coverage, --gene-counts, --splice-junctions,
--allele-counts, --realign-reads, --rna-metrics) refuses a context that never ingested with the same sentence behind its own name, and leaves no buffer behind.  No kernel is
launched: the refusal comes before the device is touched."""
import ctypes

import numpy as np
import pytest

REFUSAL = (b"%s: the record stream of the last ingest is not on the device any more (it was given back under memory pressure, another ingest has begun, or there was no ingest)")


@pytest.fixture(scope="module")
def fresh(built):
    """a context that never saw an ingest"""
    from arriba_amd import _capi
    api, params = _capi.bind_device_api(_capi.device_library(), "agpu_"), _capi.Params()
    api.default_params(ctypes.byref(params))
    context = api.create(0, ctypes.byref(params))
    assert context, api.last_error()
    yield api, context
    api.destroy(context)


def _sorted_bam_begin(api, context, _capi):
    info = _capi.SortedBamInfo()
    return api.sorted_bam_begin(context, ctypes.byref(info))


def _support_pool_build(api, context, _capi):
    info, names, name_offset = _capi.SupportPoolInfo(), np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.uint64)
    return api.support_pool_build(context, names.ctypes.data, name_offset.ctypes.data, 0, ctypes.byref(info))


def _virus_expression(api, context, _capi):
    counters, viral_ref, viral_length = _capi.VirusCounters(), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.uint32)
    return api.virus_expression(context, viral_ref.ctypes.data, viral_length.ctypes.data, 0, 0, ctypes.byref(counters))


def _depth_begin(api, context, _capi):
    info, ref_length, names, name_offset = _capi.DepthInfo(), np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.uint32)
    return api.depth_begin(context, ref_length.ctypes.data, names.ctypes.data, name_offset.ctypes.data, 0, ctypes.byref(info))


def _gene_counts(api, context, _capi):
    stats, ref_length, counts = _capi.GeneCountStats(), np.zeros(1, dtype=np.uint32), np.zeros(3 * 4, dtype=np.uint64)
    return api.gene_counts(context, ref_length.ctypes.data, 0, counts.ctypes.data, ctypes.byref(stats))


def _splice_junctions(api, context, _capi):
    stats, ref_length, rows, n_rows = _capi.JunctionStats(), np.zeros(1, dtype=np.uint32), ctypes.POINTER(_capi.JunctionRow)(), ctypes.c_uint64(0)
    return api.splice_junctions(context, ref_length.ctypes.data, 0, ctypes.byref(rows), ctypes.byref(n_rows), ctypes.byref(stats))


def _allele_counts(api, context, _capi):
    stats, ref_length, sites, rows = _capi.AlleleStats(), np.zeros(1, dtype=np.uint32), (_capi.AlleleSite * 1)(), ctypes.POINTER(_capi.AlleleRow)()
    return api.allele_counts(context, sites, 0, ref_length.ctypes.data, 0, 0, 0, ctypes.byref(rows), ctypes.byref(stats))


def _realign_begin(api, context, _capi):
    info, in_assembly, names, name_offset = _capi.RealignInfo(), np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.uint8), np.zeros(1, dtype=np.uint32)
    return api.realign_begin(context, in_assembly.ctypes.data, names.ctypes.data, name_offset.ctypes.data, 0, 0, ctypes.byref(info))


def _rna_metrics(api, context, _capi):
    # (a zeroed track passes the null check; whether it is sound is asked only behind the stream)
    stats, track, ref_length, counters = _capi.RnaMetricsStats(), _capi.RegionTrack(), np.zeros(1, dtype=np.uint32), np.zeros(_capi.RNA_METRICS_WORDS, dtype=np.uint64)
    return api.rna_metrics(context, ctypes.byref(track), ref_length.ctypes.data, 0, counters.ctypes.data, ctypes.byref(stats))


ENTRY_POINTS = [
    ("agpu_sorted_bam_begin", _sorted_bam_begin, "sorted_bam_compression_allocated_bytes"),
    ("agpu_support_pool_build", _support_pool_build, "support_allocated_bytes"),
    ("agpu_virus_expression", _virus_expression, "virus_allocated_bytes"),
    ("agpu_depth_begin", _depth_begin, "depth_allocated_bytes"),
    ("agpu_gene_counts", _gene_counts, "gene_counts_allocated_bytes"),
    ("agpu_splice_junctions", _splice_junctions, "splice_junctions_allocated_bytes"),
    ("agpu_allele_counts", _allele_counts, "allele_counts_allocated_bytes"),
    ("agpu_realign_begin", _realign_begin, "realign_allocated_bytes"),
    ("agpu_rna_metrics", _rna_metrics, "rna_metrics_allocated_bytes"),
]


@pytest.mark.gpu
@pytest.mark.parametrize("entry, call, allocated_bytes", ENTRY_POINTS, ids=[entry for entry, _, _ in ENTRY_POINTS])
def test_a_context_that_never_ingested_is_refused(fresh, entry, call, allocated_bytes):
    from arriba_amd import _capi
    api, context = fresh
    status = call(api, context, _capi)
    message = api.last_error()
    assert status != 0
    assert message == REFUSAL % entry.encode()
    held = ctypes.c_uint64(1)
    assert getattr(api, allocated_bytes)(context, ctypes.byref(held)) == 0 and held.value == 0
