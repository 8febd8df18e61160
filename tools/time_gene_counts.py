#!/usr/bin/env python3
"""One-off measurement (not a test): --gene-counts on the 10^7-fragment sample of bench.py with 4 N ordinary proper pairs (its generator, its scratch directory), the output on tmpfs.

One DevicePipeline ingests the sample, writes the sorted file with duplicate marks once (for markdup_name_kernel of the same session) and the coverage track once (for
depth_mark_kernel), and, behind a second ingest of the same file, counts `--repeats` + 1 times (the first repeat warms buffers and the first launch of every kernel and is reported
apart), then as often with ARRIBA_GENECOUNT_PLAIN_ATOMICS=1 (one atomic per lane for the gene rows instead of the leader loop).  The hot case of tests/gene_counts_lib.py (70 001
templates on one gene) goes through both variants on the committed annotation.  Then a WorkflowSession runs the sample `--repeats` + 1 times without the option -- what the parent
commit does for a sample -- and as often with it.  Prints one JSON object:
  passes_seconds   names | assign, from the HIP events of agpu_gene_counts (the median of the repeats)
  kernels          per kernel of agpu_genecount.hip: launches and ms per repeat (HIP events)
  against          genecount_name_kernel beside markdup_name_kernel and genecount_assign_kernel beside depth_mark_kernel: ms, and GB/s over records x 72 bytes (the offset and the
                   line that holds the head of a record) for all four
  plain_atomics    the assign kernel with one atomic per lane: ms on the sample and on the hot case, beside the leader loop's
  counters         the statistics, the four special rows, the genes with reads, the largest gene row (per column), whether any record carries NH > 1
  sample_seconds   the wall clock of arriba_workflow_sample without the option and with it (medians), and added_wall_seconds: what one sample alone pays for the option

    python tools/time_gene_counts.py [--fragments 10000000] [--normal-mult 4] [--repeats 3] > profiles/NAME.json"""
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


def _repeats(pipeline, count):
    """-> (the repeats, the counts and the statistics of the last one)"""
    repeats = []
    for repeat in range(count + 1):
        pipeline.set_profiling(True)  # (a new epoch: the launches of this repeat only)
        before = time.perf_counter()
        counts, stats = pipeline.gene_counts()
        wall = time.perf_counter() - before
        repeats.append({"warm_up": repeat == 0, "wall_seconds": round(wall, 4), "passes_seconds": {key: round(value, 6) for key, value in stats["seconds"].items()}, "kernels": _kernels(pipeline, ("genecount",))})
        pipeline.set_profiling(False)
    return repeats, counts, stats


def _median_ms(repeats, kernel):
    return statistics.median(entry["kernels"][kernel]["ms"] for entry in repeats if not entry["warm_up"])


def _hot_case(repeats):
    """the hot case of the tests on the committed annotation, leader loop and plain atomics: ms of the assign kernel (medians)"""
    import gene_counts_lib as lib
    from arriba_amd.pipeline import DevicePipeline, HostSession
    directory = tempfile.mkdtemp(prefix="time_gene_counts_hot_")
    try:
        case = lib.hot_case()
        sample = os.path.join(directory, "hot.bam")
        lib.write_bgzf(sample, lib.bam_header(case[0]) + lib.bam_records(case), 0)
        pipeline = lib.stream_pipeline(HostSession(os.path.join(lib.GOLDEN, "hand_made.fa"), os.path.join(lib.GOLDEN, "hand_made.gtf"), interesting_contigs=lib.COMMITTED_CONTIGS), sample)
        out = {"templates": 70065}
        for name, knob in (("leader_loop", None), ("plain_atomics", "1")):
            if knob:
                os.environ["ARRIBA_GENECOUNT_PLAIN_ATOMICS"] = knob
            try:
                timed, counts, stats = _repeats(pipeline, repeats)
            finally:
                os.environ.pop("ARRIBA_GENECOUNT_PLAIN_ATOMICS", None)
            out[name + "_assign_ms"] = _median_ms(timed, "genecount_assign_kernel")
            assert int(counts[0].max()) == 70001
        pipeline.close()
        return out
    finally:
        shutil.rmtree(directory, ignore_errors=True)


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
    output = tempfile.mkdtemp(prefix="time_gene_counts_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        prefix = os.path.join(directory, "bench")
        workload = bench.workload_args(arguments.fragments, 1000, 0, False)
        workload[workload.index("--normal-mult") + 1] = str(arguments.normal_mult)
        started = time.time()
        subprocess.run([datasets.GEN_SYNTH, "--out", prefix, "--threads", str(min(64, bench.cpu_budget()))] + workload, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        generate_seconds = time.time() - started
        pipeline = DevicePipeline(HostSession(prefix + ".fa", prefix + ".gtf"), bam=prefix + ".bam", piece_bytes=256 << 20)
        records = int(pipeline.ingest_result.records)
        result = {"fragments": arguments.fragments, "normal_mult": arguments.normal_mult, "bam_bytes": os.path.getsize(prefix + ".bam"), "records": records, "generate_seconds": round(generate_seconds, 1), "output_on": output}
        # the yardsticks of the same session: markdup_name_kernel and depth_mark_kernel read the same bytes by the same access pattern
        pipeline.set_profiling(True)
        pipeline.write_sorted_bam(os.path.join(output, "sorted.bam"), mark_duplicates=True)
        markdup_ms = _kernels(pipeline, ("markdup_name_kernel",)).get("markdup_name_kernel", {}).get("ms")
        pipeline.set_profiling(False)
        os.remove(os.path.join(output, "sorted.bam")); os.remove(os.path.join(output, "sorted.bam.bai"))
        pipeline.read_chimeric_alignments(prefix + ".bam", piece_bytes=256 << 20)
        pipeline.set_profiling(True)
        pipeline.write_coverage(os.path.join(output, "track.bedgraph"))
        depth_ms = _kernels(pipeline, ("depth_mark_kernel",)).get("depth_mark_kernel", {}).get("ms")
        pipeline.set_profiling(False)
        os.remove(os.path.join(output, "track.bedgraph"))
        result["repeats"], counts, stats = _repeats(pipeline, arguments.repeats)
        os.environ["ARRIBA_GENECOUNT_PLAIN_ATOMICS"] = "1"
        try:
            plain, plain_counts, _ = _repeats(pipeline, arguments.repeats)
        finally:
            os.environ.pop("ARRIBA_GENECOUNT_PLAIN_ATOMICS", None)
        assert (plain_counts == counts).all()
        pipeline.close()
        timed = [entry for entry in result["repeats"] if not entry["warm_up"]]
        result["passes_seconds"] = {key: statistics.median(entry["passes_seconds"][key] for entry in timed) for key in timed[0]["passes_seconds"]}
        name_ms, assign_ms = _median_ms(timed, "genecount_name_kernel"), _median_ms(timed, "genecount_assign_kernel")
        per_second = lambda ms: round(records * 72 / 1e6 / ms, 1) if ms else None  # noqa: E731
        result["against"] = {"genecount_name_kernel_ms": name_ms, "markdup_name_kernel_ms": markdup_ms, "genecount_name_kernel_GB_per_s": per_second(name_ms), "markdup_name_kernel_GB_per_s": per_second(markdup_ms),
                             "genecount_assign_kernel_ms": assign_ms, "depth_mark_kernel_ms": depth_ms, "genecount_assign_kernel_GB_per_s": per_second(assign_ms), "depth_mark_kernel_GB_per_s": per_second(depth_ms)}
        result["counters"] = {key: stats[key] for key in ("records", "templates", "without_primary", "ends", "blocks", "peak_bytes")}
        result["counters"].update({"special_rows": [[int(counts[c][row]) for c in range(3)] for row in range(4)], "genes": int(counts.shape[1] - 4), "genes_with_reads": [int((counts[c][4:] > 0).sum()) for c in range(3)],
                                   "largest_gene_row": [int(counts[c][4:].max()) for c in range(3)], "records_carry_NH_above_1": bool(counts[0][1] > 0)})
        result["plain_atomics"] = {"sample_assign_ms": _median_ms(plain, "genecount_assign_kernel"), "sample_leader_loop_assign_ms": assign_ms, "hot_case": _hot_case(arguments.repeats)}
        session = WorkflowSession(prefix + ".fa", prefix + ".gtf", params={"disable_filters": ["blacklist"]})
        seconds = {"without": [], "with": []}
        for repeat in range(2 * (arguments.repeats + 1)):
            which = "with" if repeat % 2 else "without"
            before = time.perf_counter()
            session.sample(prefix + ".bam", os.path.join(output, "fusions.tsv"), gene_counts_file=os.path.join(output, "counts.tab") if which == "with" else None)
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
