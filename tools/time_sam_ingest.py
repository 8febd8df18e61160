#!/usr/bin/env python3
"""One-off measurement (not a test): the device ingest of one sample from SAM text against the same sample as uncompressed BAM.

The sample is the 1.2 M-fragment spec of tests/test_gpu_parity.py::test_device_ingest_at_scale_and_every_container; its BAM file is converted to text once
(tools/bam_to_sam.py, the records dealt to worker processes before the GPU is opened).  Prints one JSON object:
  kernels       per kernel of agpu_sam.hip: launches, ms per ingest (HIP events), GB/s over the bytes the launch declares (text + what it writes)
  seconds       feed / device / adopt seconds of DevicePipeline.read_chimeric_alignments, text against raw BAM, every repeat
  push_sam      seconds inside agpu_ingest_push_sam per ingest (the copy is waited for and the two read-backs of a piece are taken there) and the number of pieces

    python tools/time_sam_ingest.py [--repeats 3] [--piece-mb 64] > profiles/NAME.json"""
import argparse
import gzip
import json
import multiprocessing
import os
import struct
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
SPEC = {"args": ["--seed", "41", "--fragments", "1200000", "--normal-mult", "0.5", "--contigs", "8", "--contig-len", "2000000", "--junctions", "20000", "--dup", "0.2", "--shuffle"]}

_stream, _names = None, None


def _lines_of(span):
    import bam_to_sam
    return ("\n".join(bam_to_sam.record_lines(_stream, span[0], span[1], _names)) + "\n").encode("latin-1")


def write_text(bam, raw_path, text_path, processes):
    """the uncompressed BAM stream to raw_path, its SAM text to text_path"""
    global _stream, _names
    import bam_to_sam
    _stream = gzip.open(bam, "rb").read()
    open(raw_path, "wb").write(_stream)
    header_text, _names, lengths, at = bam_to_sam.parse_header(_stream)
    starts = []
    while at < len(_stream):
        starts.append(at)
        at += 4 + struct.unpack_from("<i", _stream, at)[0]
    starts.append(len(_stream))
    cuts = [starts[len(starts) * k // (4 * processes)] for k in range(4 * processes)] + [len(_stream)]
    with multiprocessing.get_context("fork").Pool(processes) as pool, open(text_path, "wb") as out:  # (the workers inherit the stream)
        out.write(header_text.rstrip(b"\n") + b"\n" if header_text else "".join("@SQ\tSN:%s\tLN:%d\n" % pair for pair in zip(_names, lengths)).encode())
        for part in pool.imap(_lines_of, [(cuts[k], cuts[k + 1]) for k in range(len(cuts) - 1) if cuts[k] < cuts[k + 1]]):
            out.write(part)
    _stream = None
    return len(starts) - 1


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--repeats", type=int, default=3)
    parser.add_argument("--piece-mb", type=int, default=64)
    arguments = parser.parse_args()
    import datasets
    directory = tempfile.mkdtemp(prefix="time_sam_")
    prefix = datasets.generate(SPEC, directory)
    raw_path, text_path = os.path.join(directory, "raw.bam"), os.path.join(directory, "sample.sam")
    started = time.perf_counter()
    records = write_text(prefix + ".bam", raw_path, text_path, min(16, os.cpu_count() or 1))
    result = {"records": records, "text_bytes": os.path.getsize(text_path), "raw_bam_bytes": os.path.getsize(raw_path), "piece_bytes": arguments.piece_mb << 20, "convert_seconds": round(time.perf_counter() - started, 1),
              "seconds": {"text": [], "raw_bam": []}, "push_sam": []}
    from arriba_amd.pipeline import DevicePipeline, HostSession
    session = HostSession(prefix + ".fa", prefix + ".gtf")
    pipeline = DevicePipeline(session, bam=raw_path, piece_bytes=arguments.piece_mb << 20)  # (warm: buffers, pinned pieces, the first launch of every kernel)
    pushing = {"seconds": 0.0, "pieces": 0}
    push_sam = pipeline.api.ingest_push_sam

    def timed_push(*call):
        before = time.perf_counter()
        status = push_sam(*call)
        pushing["seconds"] += time.perf_counter() - before
        pushing["pieces"] += 1
        return status
    pipeline.api.ingest_push_sam = timed_push
    fragments = pipeline.n
    pipeline.read_chimeric_alignments(text_path, piece_bytes=arguments.piece_mb << 20)  # (warm, text)
    assert pipeline.n == fragments
    kernels = {}
    for repeat in range(arguments.repeats):  # interleaved: raw BAM, text, raw BAM, text, ...
        for kind, path in (("raw_bam", raw_path), ("text", text_path)):
            pushing["seconds"], pushing["pieces"] = 0.0, 0
            pipeline.set_profiling(True)
            pipeline.read_chimeric_alignments(path, piece_bytes=arguments.piece_mb << 20)
            assert pipeline.n == fragments
            result["seconds"][kind].append({key: round(value, 4) for key, value in pipeline.ingest_seconds.items()})
            if kind == "text":
                result["push_sam"].append({"seconds": round(pushing["seconds"], 4), "pieces": pushing["pieces"]})
                for name, ms, size in pipeline.kernel_profile():
                    if name.startswith("sam_"):
                        entry = kernels.setdefault(name, {"launches": 0, "ms": 0.0, "bytes": 0})
                        entry["launches"] += 1
                        entry["ms"] += ms
                        entry["bytes"] += size
            pipeline.set_profiling(False)
    result["fragments"] = fragments
    result["kernels"] = {name: {"launches_per_ingest": entry["launches"] // arguments.repeats, "ms_per_ingest": round(entry["ms"] / arguments.repeats, 3),
                                "GB_per_s": round(entry["bytes"] / entry["ms"] / 1e6, 1) if entry["ms"] > 0 else None} for name, entry in sorted(kernels.items())}
    print(json.dumps(result))
    import shutil
    shutil.rmtree(directory, ignore_errors=True)


if __name__ == "__main__":
    main()
