#!/usr/bin/env python3
"""One-off measurement (not a test): --coverage on the sample of bench.py (its generator, its scratch directory), the output on tmpfs.

One DevicePipeline ingests the sample, writes the sorted file once (for sorted_bam_key_kernel of the same run) and, behind a second ingest of the same file, writes the track
`--repeats` + 1 times (the first repeat warms buffers and the first launch of every kernel and is reported apart).  Then a WorkflowSession runs the sample `--repeats` + 1 times
without the option -- what the parent commit does for a sample -- and as often with it.  Prints one JSON object:
  passes_seconds   marks | scan | runs | text and copies, from the HIP events of agpu_depth_* (the median of the repeats)
  kernels          per kernel / library call of agpu_depth.hip: launches and ms per repeat (HIP events)
  against          depth_mark_kernel beside sorted_bam_key_kernel (the same access pattern): ms, and GB/s over records x 72 bytes (the offset and the line that holds the head) for both
  counters         records, segments, runs, covered positions, maximum depth, bytes of text, windows, peak bytes of the "depth.*" buffers
  sample_seconds   the wall clock of arriba_workflow_sample without the option and with it (medians), and added_wall_seconds: what one sample alone pays for the option

    python tools/time_depth.py [--fragments 10000000] [--repeats 3] > profiles/NAME.json"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]


def _kernels(pipeline, prefixes):
    kernels = {}
    for name, ms, size in pipeline.kernel_profile():
        if name.startswith(prefixes):
            entry = kernels.setdefault(name, {"launches": 0, "ms": 0.0})
            entry["launches"] += 1; entry["ms"] += ms
    for entry in kernels.values():
        entry["ms"] = round(entry["ms"], 3)
    return kernels


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--fragments", type=int, default=10000000)
    parser.add_argument("--repeats", type=int, default=3)
    arguments = parser.parse_args()
    import bench
    from arriba_amd.pipeline import DevicePipeline, HostSession, WorkflowSession
    directory = bench.scratch_directory(arguments.fragments * 600)
    output = tempfile.mkdtemp(prefix="time_depth_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        prefix, generate_seconds = bench.generate_sample(arguments.fragments, 1000, directory)
        pipeline = DevicePipeline(HostSession(prefix + ".fa", prefix + ".gtf"), bam=prefix + ".bam", piece_bytes=256 << 20)
        records = int(pipeline.ingest_result.records)
        result = {"fragments": arguments.fragments, "bam_bytes": os.path.getsize(prefix + ".bam"), "records": records, "generate_seconds": round(generate_seconds, 1), "output_on": output, "repeats": []}
        pipeline.set_profiling(True)
        pipeline.write_sorted_bam(os.path.join(output, "sorted.bam"))
        key_ms = _kernels(pipeline, ("sorted_bam_key_kernel",)).get("sorted_bam_key_kernel", {}).get("ms")
        pipeline.set_profiling(False)
        os.remove(os.path.join(output, "sorted.bam")); os.remove(os.path.join(output, "sorted.bam.bai"))
        pipeline.read_chimeric_alignments(prefix + ".bam", piece_bytes=256 << 20)
        for repeat in range(arguments.repeats + 1):
            pipeline.set_profiling(True)  # (a new epoch: the launches of this repeat only)
            before = time.perf_counter()
            counters = pipeline.write_coverage(os.path.join(output, "track.bedgraph"))
            wall = time.perf_counter() - before
            result["repeats"].append({"warm_up": repeat == 0, "wall_seconds": round(wall, 4), "passes_seconds": {key: round(value, 6) for key, value in counters["seconds"].items()}, "kernels": _kernels(pipeline, ("depth",))})
            pipeline.set_profiling(False)
        result["counters"] = {key: counters[key] for key in ("records", "segments", "runs", "covered_positions", "aligned_bases", "max_depth", "text_bytes", "position_windows", "text_windows", "peak_bytes")}
        pipeline.close()
        timed = [entry for entry in result["repeats"] if not entry["warm_up"]]
        result["passes_seconds"] = {key: statistics.median(entry["passes_seconds"][key] for entry in timed) for key in timed[0]["passes_seconds"]}
        scan_ms = statistics.median(entry["kernels"]["depth_mark_kernel"]["ms"] for entry in timed)
        per_second = lambda ms: round(records * 72 / 1e6 / ms, 1) if ms else None  # noqa: E731
        result["against"] = {"depth_mark_kernel_ms": scan_ms, "sorted_bam_key_kernel_ms": key_ms, "depth_mark_kernel_GB_per_s": per_second(scan_ms), "sorted_bam_key_kernel_GB_per_s": per_second(key_ms)}
        session = WorkflowSession(prefix + ".fa", prefix + ".gtf", params={"disable_filters": ["blacklist"]})
        seconds = {"without": [], "with": []}
        for repeat in range(2 * (arguments.repeats + 1)):
            which = "with" if repeat % 2 else "without"
            before = time.perf_counter()
            session.sample(prefix + ".bam", os.path.join(output, "fusions.tsv"), coverage_file=os.path.join(output, "track.bedgraph") if which == "with" else None)
            if repeat >= 2:
                seconds[which].append(round(time.perf_counter() - before, 4))
        session.close()
        result["sample_seconds"] = {"without_the_option": seconds["without"], "with_the_option": seconds["with"], "median_without": statistics.median(seconds["without"]), "median_with": statistics.median(seconds["with"])}
        result["added_wall_seconds"] = round(result["sample_seconds"]["median_with"] - result["sample_seconds"]["median_without"], 4)
        print(json.dumps(result))
    finally:
        shutil.rmtree(output, ignore_errors=True)
        shutil.rmtree(directory, ignore_errors=True)


if __name__ == "__main__":
    main()
