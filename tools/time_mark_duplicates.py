#!/usr/bin/env python3
"""One-off measurement (not a test): --mark-duplicates on the sample of bench.py (its generator, its scratch directory), the output on tmpfs.

One DevicePipeline ingests the sample and writes the sorted file `--repeats` + 1 times without the option and as often with it, in turn (the first repeat of each warms buffers and
the first launch of every kernel and is reported apart).  Then a WorkflowSession runs the sample as often with --sorted-bam alone and with --sorted-bam --mark-duplicates.  Prints
one JSON object:
  passes_seconds   name ids and claims | ends | selection and the per-record bytes, from the HIP events of agpu_markdup.hip (the median of the repeats)
  kernels          per kernel / library call of agpu_markdup.hip: launches and ms per repeat (HIP events)
  gather_ms        sorted_bam_gather_kernel without and with the flag pointer, in the same process (medians of the sums over the windows of a file)
  counters         templates, pairs, fragments, duplicates, records flagged and changed, peak bytes of the "markdup.*" buffers
  sample_seconds   the wall clock of arriba_workflow_sample with --sorted-bam alone and with the option beside it (medians), and added_wall_seconds

    python tools/time_mark_duplicates.py [--fragments 10000000] [--repeats 3] > profiles/NAME.json"""
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
    output = tempfile.mkdtemp(prefix="time_markdup_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        prefix, generate_seconds = bench.generate_sample(arguments.fragments, 1000, directory)
        pipeline = DevicePipeline(HostSession(prefix + ".fa", prefix + ".gtf"), bam=prefix + ".bam", piece_bytes=256 << 20)
        records = int(pipeline.ingest_result.records)
        result = {"fragments": arguments.fragments, "bam_bytes": os.path.getsize(prefix + ".bam"), "records": records, "generate_seconds": round(generate_seconds, 1), "output_on": output, "repeats": []}
        counters = None
        for repeat in range(2 * (arguments.repeats + 1)):
            marked = repeat % 2 == 1
            pipeline.set_profiling(True)  # (a new epoch: the launches of this file only)
            before = time.perf_counter()
            pipeline.write_sorted_bam(os.path.join(output, "sorted.bam"), mark_duplicates=marked)
            wall = time.perf_counter() - before
            entry = {"warm_up": repeat < 2, "mark_duplicates": marked, "wall_seconds": round(wall, 4), "gather_ms": _kernels(pipeline, ("sorted_bam_gather_kernel",)).get("sorted_bam_gather_kernel", {}).get("ms")}
            if marked:
                counters = pipeline.markdup_counts
                entry["passes_seconds"] = {key: round(value, 6) for key, value in counters["seconds"].items()}
                entry["kernels"] = _kernels(pipeline, ("markdup",))
            result["repeats"].append(entry)
            pipeline.set_profiling(False)
        result["counters"] = {key: counters[key] for key in ("templates", "pairs", "fragments", "duplicate_pairs", "duplicate_fragments", "records_flagged", "records_changed", "peak_bytes")}
        pipeline.close()
        timed = [entry for entry in result["repeats"] if not entry["warm_up"]]
        with_marks, without = [entry for entry in timed if entry["mark_duplicates"]], [entry for entry in timed if not entry["mark_duplicates"]]
        result["passes_seconds"] = {key: statistics.median(entry["passes_seconds"][key] for entry in with_marks) for key in with_marks[0]["passes_seconds"]}
        result["gather_ms"] = {"without_the_flag_pointer": statistics.median(entry["gather_ms"] for entry in without), "with_the_flag_pointer": statistics.median(entry["gather_ms"] for entry in with_marks)}
        result["write_sorted_bam_seconds"] = {"without": statistics.median(entry["wall_seconds"] for entry in without), "with": statistics.median(entry["wall_seconds"] for entry in with_marks)}
        session = WorkflowSession(prefix + ".fa", prefix + ".gtf", params={"disable_filters": ["blacklist"]})
        seconds = {"without": [], "with": []}
        for repeat in range(2 * (arguments.repeats + 1)):
            which = "with" if repeat % 2 else "without"
            before = time.perf_counter()
            session.sample(prefix + ".bam", os.path.join(output, "fusions.tsv"), sorted_bam_file=os.path.join(output, "sorted.bam"), mark_duplicates=which == "with")
            if repeat >= 2:
                seconds[which].append(round(time.perf_counter() - before, 4))
        session.close()
        result["sample_seconds"] = {"sorted_bam_alone": seconds["without"], "with_the_option": seconds["with"], "median_alone": statistics.median(seconds["without"]), "median_with": statistics.median(seconds["with"])}
        result["added_wall_seconds"] = round(result["sample_seconds"]["median_with"] - result["sample_seconds"]["median_alone"], 4)
        print(json.dumps(result))
    finally:
        shutil.rmtree(output, ignore_errors=True)
        shutil.rmtree(directory, ignore_errors=True)


if __name__ == "__main__":
    main()
