"""--sorted-bam-compression 1: the record blocks of --sorted-bam deflated, one deflate block per BGZF block (arriba_amd/csrc/device/deflate_out_core.hpp).

The independent decoder is tools/read_bam.py, which inflates every block with zlib and checks BSIZE (the distance to the next block), CRC-32, ISIZE and the end-of-file block.
The CPU tier runs the core header stepped on the host (ahost_sorted_bam_*_level), the GPU tier the kernels of agpu_sorted_bam.hip byte for byte against it.  What a level-1 file
must satisfy (`_checks_compressed`): the header rules, the record order and the index checks of tests/test_sorted_bam.py (the same region seeds), record blocks that inflate to
exactly 0xff00 bytes (the last one to less), no block larger than its stored form, and payloads that are byte for byte those of the level-0 file."""
import ctypes
import os
import random
import struct
import subprocess
import sys
import zlib

import pytest

import conftest
import test_sorted_bam as stored
from test_sorted_bam import DATASET_NAMES, FRAME, PAYLOAD, _expected_order, _record, _records, _references_of, _regions, _same_files, _write_bgzf, inputs  # noqa: F401 (inputs: the fixture)

sys.path.insert(0, os.path.join(conftest.ROOT, "tools"))
import read_bam  # noqa: E402

WORKFLOW = os.path.join(conftest.ROOT, "arriba_amd", "lib", "arriba_gpu_workflow")
NEW_KERNELS = ("sorted_bam_deflate_kernel", "sorted_bam_compact_kernel", "sorted_bam rocprim::exclusive_scan(blocks)", "sorted_bam rocprim::exclusive_scan(offsets)")


def _host_write(header, record_bytes, path, level):
    from arriba_amd import _capi
    lib, info = _capi.host_library(), _capi.SortedBamInfo()
    status = lib.ahost_sorted_bam_write_level(header, len(header), record_bytes, len(record_bytes), path.encode(), level, ctypes.byref(info))
    assert status == 0, lib.ahost_last_error()
    return info


def _record_blocks(path):
    """[(bytes of the block in the file, its payload)] of the record blocks: without the header blocks and the end-of-file block"""
    bam = read_bam.BamFile(path)
    offsets = [offset for offset, _ in bam.blocks] + [len(bam.raw)]
    sizes, header_blocks = [len(payload) for _, payload in bam.blocks], 0
    while sum(sizes[:header_blocks]) < bam.header_size:
        header_blocks += 1
    assert sum(sizes[:header_blocks]) == bam.header_size and sizes[-1] == 0
    return [(bam.raw[offsets[k]:offsets[k + 1]], bam.blocks[k][1]) for k in range(header_blocks, len(bam.blocks) - 1)]


def _checks_compressed(path, header, record_bytes, stored_path, seed=1):
    bam = read_bam.BamFile(path)  # (every block: BSIZE + 1 is the distance to the next one, the data inflates with nothing left over, CRC-32 and ISIZE hold, the EOF block ends the file)
    # the header rules of the stored file
    assert bam.references == _references_of(header)
    text_in = header[8:8 + struct.unpack_from("<i", header, 4)[0]]
    lines_in, lines_out = text_in.split(b"\n"), bam.text.split(b"\n")
    assert lines_out[0].startswith(b"@HD\t") and lines_out[0].split(b"\t").count(b"SO:coordinate") == 1 and sum(field.startswith(b"SO:") for field in lines_out[0].split(b"\t")) == 1
    if lines_in[0].startswith(b"@HD"):
        assert [f for f in lines_out[0].split(b"\t") if not f.startswith(b"SO:")] == [f for f in lines_in[0].split(b"\t") if not f.startswith(b"SO:")]
        lines_in = lines_in[1:]
    assert lines_out[1:] == lines_in
    # the records, in the order of samtools sort
    assert [record.bytes for record in bam.records] == _expected_order(_records(record_bytes))
    # the blocks
    blocks = _record_blocks(path)
    assert all(len(payload) == PAYLOAD for _, payload in blocks[:-1]) and all(0 < len(payload) <= PAYLOAD for _, payload in blocks[-1:]) and sum(len(payload) for _, payload in blocks) == len(record_bytes)
    assert all(len(block) <= len(payload) + FRAME for block, payload in blocks)
    stored_bam = read_bam.BamFile(stored_path)
    assert b"".join(payload for _, payload in bam.blocks) == b"".join(payload for _, payload in stored_bam.blocks)
    assert bam.raw[:bam.blocks[len(bam.blocks) - 1 - len(blocks)][0]] == stored_bam.raw[:stored_bam.blocks[len(stored_bam.blocks) - 1 - len(blocks)][0]]  # the header blocks stay as they are
    # the index: as `_checks` of the stored test
    bai = read_bam.BaiFile(path + ".bai")
    assert len(bai.references) == len(bam.references)
    for reference, index in enumerate(bai.references):
        mine = [record for record in bam.records if record.ref == reference]
        if mine:
            assert index["pseudo"][2:] == (sum(1 for r in mine if not r.flag & 4), sum(1 for r in mine if r.flag & 4))
            assert bam.uncompressed_offset(index["pseudo"][0]) == mine[0].start and bam.uncompressed_offset(index["pseudo"][1]) == mine[-1].start + len(mine[-1].bytes)
        else:
            assert index["pseudo"] is None and not index["bins"] and not index["linear"]
        for number, chunks in index["bins"].items():
            for begin, end in chunks:
                assert begin < end and all(record.ref == reference and read_bam.reg2bin(record.pos, record.end) == number for record in bam.records_between(begin, end))
    assert bai.n_no_coor == sum(1 for record in bam.records if record.ref < 0)
    for reference, begin, end in _regions(bam.references, bam.records, seed):
        found, expected = read_bam.query(bam, bai, reference, begin, end), read_bam.brute_force(bam, reference, begin, end)
        assert [record.start for record in found] == [record.start for record in expected], (reference, begin, end)
    return bam


@pytest.fixture(scope="module")
def host_files(inputs, tmp_path_factory):
    """(name, level) -> the file the host stepping makes of the input (next to its .bai): computed once"""
    cache = {}

    def get(name, level):
        if (name, level) not in cache:
            cache[(name, level)] = str(tmp_path_factory.mktemp("host_%s_%d" % (name, level)) / "sorted.bam")
            _host_write(*inputs(name), cache[(name, level)], level)
        return cache[(name, level)]
    return get


# ---- the hand-made payloads --------------------------------------------------------------------------------------------------------------------------------------

def _bytes_field(data):
    """an optional field that holds `data` as it is (a B array of uint8)"""
    return b"XPBC" + struct.pack("<I", len(data)) + bytes(data)


def _noise(generator, size):
    return bytes(generator.randrange(256) for _ in range(size))


def _filled_to(total, data_at_end=b""):
    """one record of exactly `total` bytes: noise in an optional field, `data_at_end` as its last bytes"""
    generator = random.Random(11)
    empty = len(_record("fill", 0, 1, 500, [(20, "M")], 20, aux=_bytes_field(b"")))
    record = _record("fill", 0, 1, 500, [(20, "M")], 20, aux=_bytes_field(_noise(generator, total - empty - len(data_at_end)) + data_at_end))
    assert len(record) == total
    return record


def _payload_cases():
    """name -> the records of a file; the block the case is about is the last record block"""
    generator = random.Random(5)
    far = random.Random(9)
    first, second = _noise(far, 64), _noise(far, 64)
    distances = bytearray(_noise(far, 62000))
    distances[1000:1064] = first; distances[1000 + 32768:1064 + 32768] = first      # a repeat at distance exactly 32 768
    distances[20000:20064] = second; distances[20000 + 32769:20064 + 32769] = second  # ... and one at 32 769: no match may reach that far
    return {
        "equal": _record("run", 0, 1, 500, [(20, "M")], 20, aux=stored._pad(60000)),
        "random": _record("noise", 0, 1, 500, [(20, "M")], 20, aux=_bytes_field(_noise(generator, 60000))),
        "distances": _record("far", 0, 1, 500, [(20, "M")], 20, aux=_bytes_field(distances)),
        "run_261": _record("short", 0, 1, 500, [(20, "M")], 20, aux=_bytes_field(b"y" * 261)),
        "one_byte": _filled_to(PAYLOAD + 1),
        "one_value": _filled_to(PAYLOAD + 3, b"zzz"),  # the last block: three literals of one value
    }


PAYLOAD_CASES = ["equal", "random", "distances", "run_261", "one_byte", "one_value"]


@pytest.fixture(scope="module")
def payload_files(inputs, tmp_path_factory):
    """case -> (header, record bytes, host file at level 0, host file at level 1)"""
    cache, cases = {}, _payload_cases()

    def get(name):
        if name not in cache:
            header, directory = inputs("toy3k")[0], tmp_path_factory.mktemp("payload_" + name)
            paths = [str(directory / ("level%d.bam" % level)) for level in (0, 1)]
            for level in (0, 1):
                _host_write(header, cases[name], paths[level], level)
            cache[name] = (header, cases[name], paths[0], paths[1])
        return cache[name]
    return get


# ---- CPU tier ----------------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", DATASET_NAMES + ["hand_made", "single", "no_mapped", "empty"])
def test_host_level_1_round_trip_and_index(name, built, inputs, host_files):
    header, record_bytes = inputs(name)
    path = host_files(name, 1)
    bam = _checks_compressed(path, header, record_bytes, host_files(name, 0))
    assert not os.path.exists(path + ".tmp") and not os.path.exists(path + ".bai.tmp")
    if name == "hand_made":
        assert len(_record_blocks(path)[-1][1]) == 40 and max(len(record.bytes) for record in bam.records) > 105000
    if name == "empty":
        assert not bam.records and not _record_blocks(path)


def test_level_1_announces_the_size_the_blocks_really_have(built, inputs, tmp_path):
    header, record_bytes = inputs("toy3k")
    info = _host_write(header, record_bytes, str(tmp_path / "sorted.bam"), 1)
    blocks = _record_blocks(str(tmp_path / "sorted.bam"))
    assert (info.records, info.uncompressed_bytes, info.file_bytes) == (len(_records(record_bytes)), len(record_bytes), sum(len(block) for block, _ in blocks))


def test_level_0_twin_is_the_stored_file(built, inputs, host_files, tmp_path):
    header, record_bytes = inputs("itd6k")
    path = str(tmp_path / "plain.bam")
    stored._host_write(header, record_bytes, path)
    _same_files(path, host_files("itd6k", 0))


@pytest.mark.parametrize("name", PAYLOAD_CASES)
def test_encodings_on_hand_made_payloads(name, built, payload_files):
    header, record_bytes, level0, level1 = payload_files(name)
    _checks_compressed(level1, header, record_bytes, level0)
    for (block, payload), (stored_block, _) in zip(_record_blocks(level1), _record_blocks(level0)):
        inflater = zlib.decompressobj(-15)
        assert inflater.decompress(block[18:-8]) + inflater.flush() == payload and inflater.eof and not inflater.unused_data
        assert len(block) <= len(stored_block)
    block, payload = _record_blocks(level1)[-1]
    if name == "equal":
        assert len(payload) > 60000 and len(block) * 100 < len(payload)  # distance 1, length 258, overlapping: ~233 matches of at most 3 bytes each and a header
    if name == "random":
        assert open(level1, "rb").read() == open(level0, "rb").read()  # incompressible: the stored block, exactly
    # ("distances": zlib has inflated the block above, which it refuses to do for a distance beyond 32 768)
    if name == "run_261":
        assert len(block) < len(payload)
    if name == "one_byte":
        assert len(payload) == 1
    if name == "one_value":
        assert payload == b"zzz" and not read_bam.is_stored(block, 0)


def test_the_same_input_twice_gives_the_same_bytes(built, inputs, host_files, tmp_path):
    header, record_bytes = inputs("shuffled2k")
    path = str(tmp_path / "again.bam")
    _host_write(header, record_bytes, path, 1)
    _same_files(path, host_files("shuffled2k", 1))


# our size over the size of zlib level 1 on the same blocks, measured with the host stepping (a deterministic function: a regression guard, not a noise margin), rounded up to the
# next 0.05.  Matches stay inside segments of 4 KiB, zlib's window is 32 KiB and it sends its code lengths run-length coded: the distance to 1.0 is that.
RATIO_PINS = {"toy3k": 1.10, "shuffled2k": 1.10, "itd6k": 1.10}  # measured: 1.0540, 1.0618, 1.0666 (and 0.158, 0.176, 0.148 of the stored size)


@pytest.mark.parametrize("name", DATASET_NAMES)
def test_ratio_against_zlib_level_1(name, built, inputs, host_files, tmp_path):
    blocks, stored_blocks = _record_blocks(host_files(name, 1)), _record_blocks(host_files(name, 0))
    sorted_payload = b"".join(payload for _, payload in stored_blocks)
    _write_bgzf(str(tmp_path / "zlib1.bam"), sorted_payload, 1)
    ours, theirs, plain = sum(len(block) for block, _ in blocks), os.path.getsize(str(tmp_path / "zlib1.bam")) - 28, sum(len(block) for block, _ in stored_blocks)
    print("%s: level 1 %d bytes, zlib level 1 %d bytes, stored %d bytes: ours / zlib %.4f, ours / stored %.4f" % (name, ours, theirs, plain, ours / theirs, ours / plain))
    assert theirs * 4 < plain * 3  # the precondition: the input is compressible at all
    assert ours < plain
    assert ours / theirs <= RATIO_PINS[name]


def _refused(arguments):
    result = subprocess.run(["timeout", "-k", "10", "60", WORKFLOW] + arguments, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
    assert result.returncode not in (0, 124, 137), result.stderr[-2000:]
    return result.stderr


def test_command_line_refusals(built, dataset_files, tmp_path):
    prefix = dataset_files("toy3k")
    common = ["-x", prefix + ".bam", "-g", prefix + ".gtf", "-a", prefix + ".fa", "-o", str(tmp_path / "fusions.tsv"), "-f", "blacklist"]
    assert "--sorted-bam-compression needs --sorted-bam" in _refused(common + ["--sorted-bam-compression", "1"])
    for level in ("2", "-1", "one"):
        assert "invalid argument to --sorted-bam-compression" in _refused(common + ["--sorted-bam", str(tmp_path / "out.bam"), "--sorted-bam-compression", level])
    assert not os.listdir(str(tmp_path))
    usage = subprocess.run([WORKFLOW, "-h"], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True).stdout
    assert "--sorted-bam-compression" in usage


@pytest.mark.parametrize("level", [2, -1])
def test_host_twins_refuse_other_levels(level, built, dataset_files, inputs, tmp_path):
    from arriba_amd import _capi
    lib = _capi.host_library()
    header, record_bytes = inputs("single")
    path = str(tmp_path / "refused.bam")
    assert lib.ahost_sorted_bam_write_level(header, len(header), record_bytes, len(record_bytes), path.encode(), level, None) != 0 and b"0 (stored) or 1" in lib.ahost_last_error()
    assert lib.ahost_sorted_bam_file_level((dataset_files("toy3k") + ".bam").encode(), path.encode(), level, None) != 0 and b"0 (stored) or 1" in lib.ahost_last_error()
    blocks, info = ctypes.c_void_p(), _capi.SortedBamInfo()
    assert lib.ahost_sorted_bam_level(record_bytes, len(record_bytes), 0, None, 0, level, ctypes.byref(blocks), ctypes.byref(info), None) != 0 and b"0 (stored) or 1" in lib.ahost_last_error()
    assert not os.listdir(str(tmp_path))


def test_host_reads_the_file_itself_at_level_1(built, dataset_files, host_files, tmp_path):
    """ahost_sorted_bam_file_level: what --host-ingest runs"""
    from arriba_amd import _capi
    path = str(tmp_path / "file.bam")
    assert _capi.host_library().ahost_sorted_bam_file_level((dataset_files("toy3k") + ".bam").encode(), path.encode(), 1, None) == 0
    _same_files(path, host_files("toy3k", 1))


# ---- GPU tier ----------------------------------------------------------------------------------------------------------------------------------------------------

def _toy_pipeline(dataset_files):
    from arriba_amd.pipeline import DevicePipeline, HostSession
    prefix = dataset_files("toy3k")
    return DevicePipeline(HostSession(prefix + ".fa", prefix + ".gtf"), bam=prefix + ".bam")


def _set(monkeypatch, window, ingest_windows):
    for knob, value in (("ARRIBA_SORTED_BAM_WINDOW", window), ("ARRIBA_INGEST_WINDOWS", ingest_windows)):
        if value is None:
            monkeypatch.delenv(knob, raising=False)
        else:
            monkeypatch.setenv(knob, value)


@pytest.mark.gpu
@pytest.mark.parametrize("name,window,ingest_windows", [(name, window, None) for name in DATASET_NAMES for window in (None, "131072")] + [("itd6k", "131072", "1048576,65536")])
def test_device_file_is_the_host_file_at_level_1(name, window, ingest_windows, built, dataset_files, inputs, host_files, tmp_path, monkeypatch):
    from arriba_amd.pipeline import DevicePipeline, HostSession
    _set(monkeypatch, window, ingest_windows)
    prefix = dataset_files(name)
    pipeline = DevicePipeline(HostSession(prefix + ".fa", prefix + ".gtf"), bam=prefix + ".bam", piece_bytes=1 << 20)
    path = str(tmp_path / "device.bam")
    written = pipeline.write_sorted_bam(path, compression=1)
    pipeline.close()
    header, record_bytes = inputs(name)
    blocks = (len(record_bytes) + PAYLOAD - 1) // PAYLOAD
    assert written["records"] == len(_records(record_bytes)) and written["windows"] == ((blocks + 1) // 2 if window else 1)
    assert written["file_bytes"] == sum(len(block) for block, _ in _record_blocks(path)) < len(record_bytes)
    _same_files(path, host_files(name, 1))
    _checks_compressed(path, header, record_bytes, host_files(name, 0))
    assert not os.path.exists(path + ".tmp") and not os.path.exists(path + ".bai.tmp")


@pytest.mark.gpu
def test_compaction_in_chunks_of_sixteen_blocks(built, dataset_files, inputs, host_files, tmp_path, monkeypatch):
    """one window of ~90 blocks packed by several launches of sorted_bam_compact_kernel (ARRIBA_WAVE_CHUNK): the same file"""
    from arriba_amd.pipeline import DevicePipeline, HostSession
    _set(monkeypatch, None, None)
    monkeypatch.setenv("ARRIBA_WAVE_CHUNK", "16")
    prefix = dataset_files("itd6k")
    pipeline = DevicePipeline(HostSession(prefix + ".fa", prefix + ".gtf"), bam=prefix + ".bam", piece_bytes=1 << 20)
    path = str(tmp_path / "device.bam")
    assert pipeline.write_sorted_bam(path, compression=1)["windows"] == 1 and len(_record_blocks(path)) > 48
    pipeline.close()
    _same_files(path, host_files("itd6k", 1))


@pytest.mark.gpu
@pytest.mark.parametrize("window", [None, "131072"])
def test_hand_made_files_through_the_device_at_level_1(window, built, dataset_files, inputs, host_files, tmp_path, monkeypatch):
    """hand_made (a read over three blocks, a record that ends on a block boundary, a last block of 40 bytes), single, no_mapped; at 131072 the windows hold two blocks"""
    _set(monkeypatch, window, None)
    pipeline = _toy_pipeline(dataset_files)
    for name in ("hand_made", "single", "no_mapped"):
        header, record_bytes = inputs(name)
        sample = str(tmp_path / (name + ".in.bam"))
        _write_bgzf(sample, header + record_bytes, 0)
        pipeline._ingest_records(sample, False, 100, 64 << 20)
        path = str(tmp_path / (name + ".bam"))
        pipeline.write_sorted_bam(path, compression=1)
        _same_files(path, host_files(name, 1))
        _checks_compressed(path, header, record_bytes, host_files(name, 0))
    pipeline.close()


@pytest.mark.gpu
def test_hand_made_payloads_through_the_device(built, dataset_files, payload_files, tmp_path):
    pipeline = _toy_pipeline(dataset_files)
    for name in ("equal", "random", "distances", "one_byte", "one_value", "run_261"):
        header, record_bytes, level0, level1 = payload_files(name)
        sample = str(tmp_path / (name + ".in.bam"))
        _write_bgzf(sample, header + record_bytes, 0)
        pipeline._ingest_records(sample, False, 100, 64 << 20)
        path = str(tmp_path / (name + ".bam"))
        pipeline.write_sorted_bam(path, compression=1)
        _same_files(path, level1)
        if name == "random":  # ... and the level-0 block of the device
            pipeline.write_sorted_bam(str(tmp_path / "random0.bam"))
            _same_files(path, str(tmp_path / "random0.bam"))
    pipeline.close()


@pytest.mark.gpu
def test_session_of_two_lanes_with_a_level_per_sample(built, dataset_files, inputs, host_files, tmp_path):
    from arriba_amd.pipeline import WorkflowSession
    prefixes = {name: dataset_files(name) for name in ("toy3k", "itd6k")}
    session = WorkflowSession(prefixes["toy3k"] + ".fa", prefixes["toy3k"] + ".gtf", params={"disable_filters": ["blacklist"]})
    samples = [(name, level, prefixes[name] + ".bam", str(tmp_path / ("fusions%d.tsv" % k)), str(tmp_path / ("sorted%d.bam" % k))) for k, (name, level) in enumerate((("toy3k", 1), ("itd6k", 0), ("toy3k", 1)))]
    session.submit(samples[0][2], sorted_bam_file=samples[0][4], sorted_bam_compression=samples[0][1])
    for k, (name, level, bam, output, path) in enumerate(samples):
        if k + 1 < len(samples):
            session.submit(samples[k + 1][2], sorted_bam_file=samples[k + 1][4], sorted_bam_compression=samples[k + 1][1])
        session.sample(bam, output)
    session.close()
    for name, level, bam, output, path in samples:
        _same_files(path, host_files(name, level))  # (level 0: the host's stored file, which tests/test_sorted_bam.py ties to the device of the commit before)
    stored._checks(samples[1][4], *inputs("itd6k"))
    assert open(samples[0][3]).read() == open(samples[2][3]).read()
    assert not [entry for entry in os.listdir(str(tmp_path)) if entry.endswith(".tmp")]


@pytest.mark.gpu
def test_off_means_off(built, dataset_files, tmp_path):
    """with the option off and at level 0 none of the new kernels runs and none of the new buffers exists; at level 1 they do (the probe sees them)"""
    prefix = dataset_files("toy3k")
    pipeline = _toy_pipeline(dataset_files)
    pipeline.set_profiling(True)
    pipeline.read_chimeric_alignments(prefix + ".bam")
    assert not [launch for launch in pipeline.kernel_profile() if launch[0].startswith("sorted_bam")] and pipeline.sorted_bam_compression_allocated_bytes() == 0
    pipeline.write_sorted_bam(str(tmp_path / "level0.bam"))
    names = {launch[0] for launch in pipeline.kernel_profile()}
    assert "sorted_bam_gather_kernel" in names and not names & set(NEW_KERNELS) and pipeline.sorted_bam_compression_allocated_bytes() == 0
    from arriba_amd.pipeline import ArribaError
    with pytest.raises(ArribaError, match="the level is 0 .stored blocks. or 1"):
        pipeline.write_sorted_bam(str(tmp_path / "level2.bam"), compression=2)
    pipeline.write_sorted_bam(str(tmp_path / "level1.bam"), compression=1)
    names = {launch[0] for launch in pipeline.kernel_profile()}
    assert set(NEW_KERNELS) <= names and pipeline.sorted_bam_compression_allocated_bytes() > 0
    pipeline.write_sorted_bam(str(tmp_path / "again0.bam"))  # the level holds for one begin ... end
    _same_files(str(tmp_path / "again0.bam"), str(tmp_path / "level0.bam"))
    pipeline.close()
    assert sorted(os.listdir(str(tmp_path))) == ["again0.bam", "again0.bam.bai", "level0.bam", "level0.bam.bai", "level1.bam", "level1.bam.bai"]


@pytest.mark.gpu
def test_index_before_the_last_window_is_refused(built, dataset_files, monkeypatch):
    from arriba_amd import _capi
    monkeypatch.setenv("ARRIBA_SORTED_BAM_WINDOW", "131072")
    pipeline = _toy_pipeline(dataset_files)
    info, index, lengths = _capi.SortedBamInfo(), _capi.SortedBamIndex(), (ctypes.c_uint32 * 1)(300000)
    pipeline._check(pipeline.api.sorted_bam_set_compression(pipeline.ctx, 1))
    pipeline._check(pipeline.api.sorted_bam_begin(pipeline.ctx, ctypes.byref(info)))
    assert info.windows > 1
    assert pipeline.api.sorted_bam_index(pipeline.ctx, 100, ctypes.addressof(lengths), 1, ctypes.byref(index)) != 0 and b"behind the agpu_sorted_bam_next that fetched the last window" in pipeline.api.last_error()
    pipeline._check(pipeline.api.sorted_bam_end(pipeline.ctx))
    pipeline.close()


@pytest.mark.gpu
def test_command_line_writes_a_compressed_file(built, dataset_files, inputs, host_files, tmp_path):
    prefix = dataset_files("toy3k")
    outputs = {}
    for level in (None, "1"):
        directory = tmp_path / ("level_%s" % level)
        directory.mkdir()
        outputs[level] = str(directory / "fusions.tsv")
        command = [WORKFLOW, "-x", prefix + ".bam", "-g", prefix + ".gtf", "-a", prefix + ".fa", "-o", outputs[level], "-f", "blacklist"] + (["--sorted-bam", str(directory / "out.bam"), "--sorted-bam-compression", level] if level else [])
        result = subprocess.run(["timeout", "-k", "10", "120"] + command, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True)
        assert result.returncode == 0, result.stderr[-2000:]
    assert open(outputs["1"]).read() == open(outputs[None]).read()
    path = str(tmp_path / "level_1" / "out.bam")
    _checks_compressed(path, *inputs("toy3k"), host_files("toy3k", 0))
    _same_files(path, host_files("toy3k", 1))
    assert sorted(os.listdir(str(tmp_path / "level_1"))) == ["fusions.tsv", "out.bam", "out.bam.bai"]
