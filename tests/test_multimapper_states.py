"""filter_multimappers under injected candidate support (reference: source/filter_multimappers.cpp:79-221).

Three pieces of the stage exist on the device only (agpu_multimappers.hip) and the host stepping harness (tests/emu) steps none of them: the support rank from four stable radix
sorts over packed keys (harness: std::sort with a comparator), the best rank per multi-mapping read and the recount by a wavefront per 64 candidates -- ballots for the owner of a
list entry, a stride unrolled four times, __shfl_up for the start of a lane's range (harness: two serial loops) -- and the bitmaps over the reads from ballots.  The generated
samples reach a support of a few hundred reads; here the counters are injected (tests/multimapper_states_lib.py: at 2^17 and above, at 0, 1, 2 and 2^31 - 1, all the same, with
filtered candidates in between) on a sample where the support order decides many groups of alignments.

CPU tier: the conditions on the sample (nothing passes by being absent), the harness against a numpy restatement of the recount, the harness against the live reference.
GPU tier: the device against the harness (the filter of every fragment, every candidate column, both counts) and against the restatement under every state, implicit discordant
lists in windows of 1 024 entries against explicit ones, the device against the live reference."""
import os

import numpy as np
import pytest

import datasets
import multimapper_states_lib as lib
import parity


@pytest.fixture(scope="module")
def sample(built, tmp_path_factory):
    return datasets.generate(lib.SPEC, str(tmp_path_factory.mktemp("multimapper_states")))


@pytest.fixture(scope="module")
def on_harness(sample, emu_api):
    """state -> the run of the host stepping harness (the expected value of both tiers); each state runs once per module and is left unchanged"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = lib.run_state(sample, name, api=emu_api)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def on_device(sample):
    """state -> the run of the HIP kernels with the lists in memory; once per module"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = lib.run_state(sample, name)
        return cache[name]
    return get


@pytest.fixture(scope="module")
def reference_dump(sample, tmp_path_factory):
    """the dumps of the reference run live on the sample (None where its oracle build is absent)"""
    if not datasets.reference_available():
        return None
    dump = str(tmp_path_factory.mktemp("multimapper_states_dump"))
    log = datasets.run_reference(sample, dump)
    with open(os.path.join(dump, "reference.log"), "w") as out:
        out.write(log)
    return dump


def fragments_marked_differently(a, b):
    return int((a["fragments"] != b["fragments"]).sum())


# ---- CPU tier ----------------------------------------------------------------------------------------------------------------------------------------

def test_the_sample_has_the_lists_the_kernels_need(on_harness):
    """more candidates than a workgroup of the list kernels takes and a last wavefront that is not full, candidates with empty lists, a list longer than one pass of the unrolled
    stride (256 entries), reads that several candidates list"""
    shape = lib.list_statistics(on_harness("as_found"))
    assert shape["candidates"] >= 2048 and shape["candidates"] % 64 != 0, shape
    assert shape["empty"] >= 100, shape
    assert shape["longest"] > 256, shape
    assert shape["shared_reads"] >= 500, shape


def test_the_states_change_what_the_stage_does(on_harness):
    """the support order above 2^17 decides groups of alignments: an order that ties there, or that is cut off there, marks other fragments"""
    above = fragments_marked_differently(on_harness("above_2_17"), on_harness("flat_2_17"))
    assert above >= 100, above
    clamped = fragments_marked_differently(on_harness("mixed"), on_harness("mixed_clamped"))
    assert clamped >= 30, clamped
    assert on_harness("flat_1")["remaining"] < on_harness("flat_2_17")["remaining"]  # a counter of 1 saturates at 0: the candidate is filtered
    filtered = on_harness("mixed_filtered")
    assert int((filtered["before"]["filter"] != 0).sum()) == (filtered["n"] + 4) // 5
    zero_support = on_harness("mixed")["before"]
    assert int((zero_support["split_reads1"].astype(np.int64) + zero_support["split_reads2"] + zero_support["discordant_mates"] == 0).sum()) >= 100


@pytest.mark.parametrize("state", list(lib.STATES))
def test_harness_recount_equals_the_restatement(state, on_harness):
    result = on_harness(state)
    assert result["discarded"] == int((result["fragments"] != result["fragments_before"]).sum())
    assert not lib.differences_from_recount(result)


@pytest.mark.skipif(not datasets.reference_available(), reason="oracle/_ref/arriba_ref_dump is not built")
def test_harness_as_found_against_the_live_reference(sample, emu_api, reference_dump):
    session, pipeline = parity.run_read_level(parity.open_session, sample, api=emu_api)
    assert parity.check_multimappers(session, pipeline, reference_dump) > 100
    pipeline.close(); session.close()


# ---- GPU tier ----------------------------------------------------------------------------------------------------------------------------------------

def assert_same_run(mine, expected, what):
    different = fragments_marked_differently(mine, expected)
    assert different == 0, "%s: %d of %d fragments have another filter (first: %s)" % (what, different, len(expected["fragments"]), np.flatnonzero(mine["fragments"] != expected["fragments"])[:10].tolist())
    for key in lib.CANDIDATE_COLUMNS:
        wrong = np.flatnonzero(mine["after"][key] != expected["after"][key])
        assert wrong.size == 0, "%s: %s differs for %d candidates (first: %s)" % (what, key, wrong.size, [(int(c), int(mine["after"][key][c]), int(expected["after"][key][c])) for c in wrong[:10]])
    assert (mine["remaining"], mine["discarded"]) == (expected["remaining"], expected["discarded"]), what


@pytest.mark.gpu
@pytest.mark.timeout(600, method="thread")
@pytest.mark.parametrize("state", lib.COMPARED_STATES)
def test_device_equals_the_host_stepping_under_every_state(state, on_device, on_harness):
    mine, expected = on_device(state), on_harness(state)
    assert mine["n"] == expected["n"]
    for key in ("list_offset", "read_lists") + lib.CANDIDATE_COLUMNS:  # both start from the same lists and the same state
        assert np.array_equal(mine["before"][key], expected["before"][key]), key
    assert_same_run(mine, expected, "device against harness under " + state)
    assert not lib.differences_from_recount(mine)


@pytest.mark.gpu
@pytest.mark.timeout(600, method="thread")
def test_implicit_list_windows_give_the_same_states(sample, on_device):
    """the discordant lists implicit and expanded in windows of 1 024 entries (some 90 windows whose first candidates are no multiples of 64): the list kernels start at the
    window's first candidate, and the recount walks lists whose entries were only zero-filled where the candidate is filtered"""
    for state in ("as_found", "above_2_17", "mixed_filtered"):
        with parity.implicit_lists(1024):
            windowed = lib.run_state(sample, state, profile=True)
        explicit = on_device(state)
        assert windowed["launches"].count("list_best_rank_kernel") > 50 and windowed["launches"].count("list_recount_kernel") > 50  # one launch per window
        assert np.array_equal(windowed["before"]["list_offset"], explicit["before"]["list_offset"]), state
        assert_same_run(windowed, explicit, "implicit against explicit lists under " + state)


@pytest.mark.gpu
@pytest.mark.timeout(600, method="thread")
def test_as_found_against_the_live_reference(sample, reference_dump):
    if reference_dump is None:
        return
    session, pipeline = parity.run_read_level(parity.open_session, sample)
    assert parity.check_multimappers(session, pipeline, reference_dump) > 100
    pipeline.close(); session.close()
