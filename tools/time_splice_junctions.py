#!/usr/bin/env python3
"""One-off measurement (not a test): --splice-junctions on the 10^7-fragment sample of bench.py with 4 N ordinary proper pairs (its generator, its scratch directory), the output on
tmpfs.  The generator splices its reads over the exons of its annotation, so the records carry N operations as they are; `crossings_per_record` says how many.

One DevicePipeline ingests the sample, writes the coverage track once (for depth_mark_kernel) and counts reads per gene once (for genecount_assign_kernel) -- the yardsticks of the
same session: they do the same CIGAR walk over the same bytes --, then makes the junction table `--repeats` + 1 times (the first repeat warms buffers and the first launch of every
kernel and is reported apart).  Then a WorkflowSession runs the sample `--repeats` + 1 times without the option -- what the parent commit does for a sample -- and as often with
it.  Prints one JSON object:
  passes_seconds   count | names | emit | order | classify, from the HIP events of agpu_splice_junctions (the median of the repeats)
  kernels          per kernel and rocPRIM call of agpu_junctions.hip: launches and ms per repeat (HIP events), the medians in kernels_median_ms
  against          junction_count_kernel and junction_emit_kernel beside genecount_assign_kernel and depth_mark_kernel: ms, and GB/s over records x 72 bytes (the offset and the line
                   that holds the head of a record) for all four
  counters         the statistics, crossings per record, rows by motif
  sample_seconds   the wall clock of arriba_workflow_sample without the option and with it (medians), and added_wall_seconds: what one sample alone pays for the option

    python tools/time_splice_junctions.py [--fragments 10000000] [--normal-mult 4] [--repeats 3] > profiles/NAME.json"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
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
    parser.add_argument("--normal-mult", type=int, default=4, help="ordinary proper pairs per chimeric fragment (bench.py's leg value_with_normal_pairs: 4)")
    parser.add_argument("--repeats", type=int, default=3)
    arguments = parser.parse_args()
    import bench
    import datasets
    from arriba_amd.pipeline import DevicePipeline, HostSession, WorkflowSession
    directory = bench.scratch_directory(arguments.fragments * 600 * (1 + arguments.normal_mult))
    output = tempfile.mkdtemp(prefix="time_splice_junctions_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        prefix = os.path.join(directory, "bench")
        workload = bench.workload_args(arguments.fragments, 1000, 0, False)
        workload[workload.index("--normal-mult") + 1] = str(arguments.normal_mult)
        started = time.time()
        subprocess.run([datasets.GEN_SYNTH, "--out", prefix, "--threads", str(min(64, bench.cpu_budget()))] + workload, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        generate_seconds = time.time() - started
        pipeline = DevicePipeline(HostSession(prefix + ".fa", prefix + ".gtf"), bam=prefix + ".bam", piece_bytes=256 << 20)
        records = int(pipeline.ingest_result.records)
        result = {"fragments": arguments.fragments, "normal_mult": arguments.normal_mult, "bam_bytes": os.path.getsize(prefix + ".bam"), "records": records, "generate_seconds": round(generate_seconds, 1), "output_on": "tmpfs" if output.startswith("/dev/shm") else "the temporary directory"}
        # the yardsticks of the same session
        pipeline.set_profiling(True)
        pipeline.write_coverage(os.path.join(output, "track.bedgraph"))
        depth_ms = _kernels(pipeline, ("depth_mark_kernel",)).get("depth_mark_kernel", {}).get("ms")
        pipeline.set_profiling(False)
        os.remove(os.path.join(output, "track.bedgraph"))
        pipeline.set_profiling(True)
        pipeline.gene_counts()
        assign_ms = _kernels(pipeline, ("genecount_assign_kernel",)).get("genecount_assign_kernel", {}).get("ms")
        pipeline.set_profiling(False)
        repeats = []
        for repeat in range(arguments.repeats + 1):
            pipeline.set_profiling(True)  # (a new epoch: the launches of this repeat only)
            before = time.perf_counter()
            rows, stats = pipeline.splice_junctions()
            wall = time.perf_counter() - before
            repeats.append({"warm_up": repeat == 0, "wall_seconds": round(wall, 4), "passes_seconds": {key: round(value, 6) for key, value in stats["seconds"].items()}, "kernels": _kernels(pipeline, ("junction",))})
            pipeline.set_profiling(False)
        result["repeats"] = repeats
        motifs = [0] * 7
        for row in rows:
            motifs[row.motif] += 1
        pipeline.close()
        timed = [entry for entry in repeats if not entry["warm_up"]]
        result["passes_seconds"] = {key: statistics.median(entry["passes_seconds"][key] for entry in timed) for key in timed[0]["passes_seconds"]}
        result["wall_seconds"] = statistics.median(entry["wall_seconds"] for entry in timed)
        result["kernels_median_ms"] = {name: statistics.median(entry["kernels"][name]["ms"] for entry in timed) for name in timed[0]["kernels"]}
        count_ms, emit_ms = result["kernels_median_ms"].get("junction_count_kernel"), result["kernels_median_ms"].get("junction_emit_kernel")
        per_second = lambda ms: round(records * 72 / 1e6 / ms, 1) if ms else None  # noqa: E731
        result["against"] = {"junction_count_kernel_ms": count_ms, "junction_emit_kernel_ms": emit_ms, "genecount_assign_kernel_ms": assign_ms, "depth_mark_kernel_ms": depth_ms,
                             "junction_count_kernel_GB_per_s": per_second(count_ms), "junction_emit_kernel_GB_per_s": per_second(emit_ms), "genecount_assign_kernel_GB_per_s": per_second(assign_ms),
                             "depth_mark_kernel_GB_per_s": per_second(depth_ms)}
        result["counters"] = {key: stats[key] for key in ("records", "contributing", "crossings", "pairs", "junctions", "annotated", "peak_bytes")}
        result["counters"].update({"crossings_per_record": round(stats["crossings"] / max(records, 1), 4), "rows_by_motif": motifs})
        session = WorkflowSession(prefix + ".fa", prefix + ".gtf", params={"disable_filters": ["blacklist"]})
        seconds = {"without": [], "with": []}
        for repeat in range(2 * (arguments.repeats + 1)):
            which = "with" if repeat % 2 else "without"
            before = time.perf_counter()
            session.sample(prefix + ".bam", os.path.join(output, "fusions.tsv"), splice_junctions_file=os.path.join(output, "junctions.tab") if which == "with" else None)
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
