"""filter_multimappers under injected candidate support (test tooling for tests/test_multimapper_states.py).

The sample is rich in multi-mapping reads that two or more candidates list and in groups of alignments whose scores tie, so the support
order of the candidates (reference: fusion_has_more_support, source/filter_multimappers.cpp:79-107) decides many groups.  A STATE replaces
the counters (and filters) of the candidates behind merge_adjacent_fusions, so that the order is taken at supports no generated sample
reaches: above 2^17, at both ends of the 32-bit counter, at zero, with every support the same.
"""
import numpy as np

import parity

# 4 432 fragments, 2 350 candidates (224 of them with empty lists), 93 261 list entries, the longest lists of one candidate 687 entries, 1 179 reads listed by two or more candidates
SPEC = {"args": ["--seed", "11", "--fragments", "3000", "--contigs", "4", "--contig-len", "300000", "--junctions", "60", "--multimap", "0.3"]}

FILTER_NONE, FILTER_MULTIMAPPERS = 0, 9  # views.hpp
FILTER_INJECTED = 12  # relative_support; any id other than none would do: the stage only asks whether a candidate has one

SUPPORT_EDGES = np.array([0, 1, 2, 131070, 131071, 131072, 131073, 1 << 20, (1 << 31) - 1], dtype=np.int64)


def _columns(total):
    """a total split over split_reads1, split_reads2, discordant_mates"""
    total = np.asarray(total, dtype=np.int64)
    third = total // 3
    assert int(total.max()) < 1 << 32
    return third.astype(np.uint32), third.astype(np.uint32), (total - 2 * third).astype(np.uint32)


def _flat(value):
    def state(table, n):
        return (None, np.full(n, value, dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32))
    return state


def as_found(table, n):
    return (None, table["split_reads1"].copy(), table["split_reads2"].copy(), table["discordant_mates"].copy())


def above_2_17(table, n):
    r = np.random.RandomState(217).randint(0, 1000, n)
    return (None, (131072 + r).astype(np.uint32), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32))


def _mixed_totals(n):
    return SUPPORT_EDGES[np.random.RandomState(31).randint(0, len(SUPPORT_EDGES), n)]


def mixed(table, n):
    return (None,) + _columns(_mixed_totals(n))


def mixed_clamped(table, n):
    return (None,) + _columns(np.minimum(_mixed_totals(n), 131071))


def mixed_filtered(table, n):
    filters = np.zeros(n, dtype=np.uint8)
    filters[::5] = FILTER_INJECTED
    return (filters,) + _columns(_mixed_totals(n))


STATES = {"as_found": as_found, "flat_1": _flat(1), "flat_2_17": _flat(131072), "above_2_17": above_2_17, "mixed": mixed, "mixed_clamped": mixed_clamped, "mixed_filtered": mixed_filtered}
COMPARED_STATES = [name for name in STATES if name != "mixed_clamped"]
CANDIDATE_COLUMNS = ("split_reads1", "split_reads2", "discordant_mates", "filter")


def run_state(prefix, name, api=None, profile=False):
    """run_read_level -> find_fusions -> merge_adjacent_fusions -> the state -> filter_multimappers through `api` (None: the device library).
    Returns the candidate table in front of the stage (with its lists), the candidate columns behind it, the fragment filters in front of and behind it,
    `remaining` and `discarded`; with profile, the names of the kernels the stage launched (one entry per launch)."""
    session, pipeline = parity.run_read_level(parity.open_session, prefix, api=api)
    try:
        pipeline.find_fusions()
        pipeline.merge_adjacent_fusions()
        n = pipeline.n_candidates
        filters, split_reads1, split_reads2, discordant_mates = STATES[name](pipeline.candidates(lists=False), n)
        pipeline.set_candidate_state(filters, split_reads1, split_reads2, discordant_mates)
        before = pipeline.candidates()
        assert all(np.array_equal(before[key], column) for key, column in (("split_reads1", split_reads1), ("split_reads2", split_reads2), ("discordant_mates", discordant_mates)))
        assert filters is None or np.array_equal(before["filter"], filters)
        fragments_before = pipeline.filters().copy()
        if profile:
            pipeline.set_profiling(True)
        remaining, discarded = pipeline.filter_multimappers()
        launches = [kernel for kernel, _, _ in pipeline.kernel_profile()] if profile else None
        after = pipeline.candidates(lists=False)
        return {"n": n, "before": before, "after": {key: after[key].copy() for key in CANDIDATE_COLUMNS}, "fragments_before": fragments_before, "fragments": pipeline.filters().copy(),
                "remaining": remaining, "discarded": discarded, "launches": launches}
    finally:
        pipeline.close()
        session.close()


def recount(filters, split_reads1, split_reads2, discordant_mates, list_offset, read_lists, fragment_filters):
    """reference: source/filter_multimappers.cpp:188-219 on arrays.  The candidate filters and counters in front of the stage, the three lists of every candidate
    (list_offset[3 n + 1] into read_lists) and the filters of the fragments behind the stage give the counters and filters of the candidates behind it and `remaining`."""
    n = len(filters)
    offsets = np.asarray(list_offset, dtype=np.int64)
    lost_before = np.concatenate([[0], np.cumsum(np.asarray(fragment_filters)[np.asarray(read_lists, dtype=np.int64)] == FILTER_MULTIMAPPERS)]).astype(np.int64)
    lost = (lost_before[offsets[1:]] - lost_before[offsets[:-1]]).reshape(n, 3)  # per list: the listed reads that are multi-mappers now
    counters = np.stack([np.asarray(split_reads1), np.asarray(split_reads2), np.asarray(discordant_mates)], axis=1).astype(np.int64)
    looked_at = (np.asarray(filters) == FILTER_NONE) & (counters.sum(axis=1) != 0)  # :191
    counters = np.where(looked_at[:, None], np.maximum(counters - lost, 0), counters)  # :194-208, each list on its own counter, never below 0
    filters = np.array(filters, dtype=np.uint8)
    filters[looked_at & (counters.sum(axis=1) == 0)] = FILTER_MULTIMAPPERS  # :210-211
    return {"split_reads1": counters[:, 0].astype(np.uint32), "split_reads2": counters[:, 1].astype(np.uint32), "discordant_mates": counters[:, 2].astype(np.uint32), "filter": filters,
            "remaining": int((filters == FILTER_NONE).sum())}  # :215-219


def recount_of(result, fragment_filters=None):
    """the restatement on the lists and the state a run had in front of the stage, fed the fragment filters of that run (or of another)"""
    before = result["before"]
    return recount(before["filter"], before["split_reads1"], before["split_reads2"], before["discordant_mates"], before["list_offset"], before["read_lists"],
                   result["fragments"] if fragment_filters is None else fragment_filters)


def differences_from_recount(result):
    """what a run's candidate columns and `remaining` have that the restatement does not give"""
    expected = recount_of(result)
    problems = [(key, int((result["after"][key] != expected[key]).sum())) for key in CANDIDATE_COLUMNS if not np.array_equal(result["after"][key], expected[key])]
    if result["remaining"] != expected["remaining"]:
        problems.append(("remaining", result["remaining"], expected["remaining"]))
    return problems


def list_statistics(result):
    """shape of the read lists of a run: candidates, candidates with empty lists, entries of the longest candidate, reads listed by two or more candidates"""
    n, before = result["n"], result["before"]
    offsets = before["list_offset"].astype(np.int64)
    entries = offsets[3::3] - offsets[:-1:3]
    owner = np.repeat(np.arange(n, dtype=np.int64), entries)
    pairs = np.unique(owner << 32 | before["read_lists"].astype(np.int64))  # (candidate, read) once, whichever of its lists hold the read
    listed_by = np.bincount(pairs & 0xFFFFFFFF)
    return {"candidates": n, "empty": int((entries == 0).sum()), "longest": int(entries.max()), "entries": int(entries.sum()), "shared_reads": int((listed_by >= 2).sum())}
