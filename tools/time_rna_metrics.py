#!/usr/bin/env python3
"""One-off measurement (not a test): --rna-metrics on the 10^7-fragment sample of bench.py with 4 N ordinary proper pairs (its generator, its scratch directory), the output on tmpfs.

One DevicePipeline ingests the sample, writes the coverage track once (for depth_mark_kernel of the same session) and the gene counts once (for genecount_assign_kernel), and then
sums the metrics `--repeats` + 1 times (the first repeat warms buffers, copies the track and makes the first launch, and is reported apart), then as often with
ARRIBA_RNAMETRICS_PLAIN_ATOMICS=1 (every lane adds to global memory instead of the workgroup summing in LDS first).  The hot case of tests/rna_metrics_lib.py (20 000 identical records)
goes through both forms on a seeded annotation.  Then a WorkflowSession runs the sample `--repeats` + 1 times without the option -- what the parent commit does for a sample -- and
as often with it.  Prints one JSON object:
  kernel           rnametrics_record_kernel: ms per repeat from HIP events (the median), GB/s over records x 72 bytes (the offset and the line that holds the head of a record)
  against          depth_mark_kernel and genecount_assign_kernel of the same session, which walk the same bytes: ms and GB/s by the same yardstick
  plain_atomics    the kernel with global atomics per lane: ms on the sample and on the hot case, beside the LDS form's
  counters         the statistics, the scalar counters of the file, the peak of the "rnametrics.*" buffers, the runs of the track
  sample_seconds   the wall clock of arriba_workflow_sample without the option and with it (medians), and added_wall_seconds: what one sample alone pays for the option

    python tools/time_rna_metrics.py [--fragments 10000000] [--normal-mult 4] [--repeats 3] > profiles/NAME.json"""
import argparse
import ctypes
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
KERNEL = "rnametrics_record_kernel"


def _kernels(pipeline, prefixes):
    kernels = {}
    for name, ms, size in pipeline.kernel_profile():
        if name.startswith(prefixes):
            entry = kernels.setdefault(name, {"launches": 0, "ms": 0.0})
            entry["launches"] += 1; entry["ms"] += ms
    for entry in kernels.values():
        entry["ms"] = round(entry["ms"], 3)
    return kernels


def _repeats(pipeline, count, bed=None):
    """-> (the repeats, the counters and the statistics of the last one)"""
    repeats = []
    for repeat in range(count + 1):
        pipeline.set_profiling(True)  # (a new epoch: the launches of this repeat only)
        before = time.perf_counter()
        counters, stats = pipeline.rna_metrics(bed)
        wall = time.perf_counter() - before
        repeats.append({"warm_up": repeat == 0, "wall_seconds": round(wall, 4), "event_seconds": round(stats["seconds"]["kernel"], 6), "kernels": _kernels(pipeline, ("rnametrics",))})
        pipeline.set_profiling(False)
    return repeats, counters, stats


def _median_ms(repeats):
    return statistics.median(entry["kernels"][KERNEL]["ms"] for entry in repeats if not entry["warm_up"])


def _both_forms(pipeline, count, bed=None):
    timed, counters, stats = _repeats(pipeline, count, bed)
    os.environ["ARRIBA_RNAMETRICS_PLAIN_ATOMICS"] = "1"
    try:
        plain, plain_counters, _ = _repeats(pipeline, count, bed)
    finally:
        os.environ.pop("ARRIBA_RNAMETRICS_PLAIN_ATOMICS", None)
    assert (plain_counters == counters).all()
    return timed, plain, counters, stats


def _hot_case(repeats):
    """the hot case of the tests on a seeded annotation, both forms: ms of the kernel (medians)"""
    import rna_metrics_lib as lib
    from arriba_amd.pipeline import HostSession
    directory = tempfile.mkdtemp(prefix="time_rna_metrics_hot_")
    try:
        prefix = lib.write_seeded_annotation(1900, directory)
        annotation = lib.load_annotation(prefix + ".gtf", prefix + ".fa", prefix + ".bed")
        case = lib.hot_case(annotation)
        sample = os.path.join(directory, "hot.bam")
        lib.write_bgzf(sample, lib.bam_header(case[0]) + lib.bam_records(case), 0)
        pipeline = lib.stream_pipeline(HostSession(prefix + ".fa", prefix + ".gtf", interesting_contigs="s1 s2"), sample)
        timed, plain, counters, _ = _both_forms(pipeline, repeats, prefix + ".bed")
        pipeline.close()
        assert int(counters[0]) == 20000
        return {"records": 20000, "lds_ms": _median_ms(timed), "plain_atomics_ms": _median_ms(plain)}
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
    from arriba_amd import _capi
    from arriba_amd.pipeline import DevicePipeline, HostSession, WorkflowSession
    directory = bench.scratch_directory(arguments.fragments * 600 * (1 + arguments.normal_mult))
    output = tempfile.mkdtemp(prefix="time_rna_metrics_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
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
        # the yardsticks of the same session: depth_mark_kernel and genecount_assign_kernel walk the same bytes
        pipeline.set_profiling(True)
        pipeline.write_coverage(os.path.join(output, "track.bedgraph"))
        depth_ms = _kernels(pipeline, ("depth_mark_kernel",)).get("depth_mark_kernel", {}).get("ms")
        pipeline.set_profiling(False)
        os.remove(os.path.join(output, "track.bedgraph"))
        pipeline.set_profiling(True)
        pipeline.gene_counts()
        assign_ms = _kernels(pipeline, ("genecount_assign_kernel",)).get("genecount_assign_kernel", {}).get("ms")
        pipeline.set_profiling(False)
        started = time.perf_counter()
        track = _capi.RegionTrack()
        assert pipeline.session._lib.ahost_region_track(pipeline.session._session, None, ctypes.byref(track), None) == 0
        result["track"] = {"build_seconds": round(time.perf_counter() - started, 4), "runs": int(track.n_runs), "contigs": int(track.n_contigs), "genes": int(track.n_genes)}
        timed, plain, counters, stats = _both_forms(pipeline, arguments.repeats)
        result["repeats"], result["repeats_plain_atomics"] = timed, plain
        result["allocated_bytes_after"] = pipeline.rna_metrics_allocated_bytes()
        pipeline.close()
        kernel_ms = _median_ms(timed)
        per_second = lambda ms: round(records * 72 / 1e6 / ms, 1) if ms else None  # noqa: E731
        result["kernel"] = {"ms": kernel_ms, "GB_per_s": per_second(kernel_ms)}
        result["against"] = {"depth_mark_kernel_ms": depth_ms, "depth_mark_kernel_GB_per_s": per_second(depth_ms), "genecount_assign_kernel_ms": assign_ms, "genecount_assign_kernel_GB_per_s": per_second(assign_ms)}
        import rna_metrics_lib as lib
        result["counters"] = {key: stats[key] for key in ("records", "base_records", "blocks", "segments", "track_runs", "peak_bytes")}
        result["counters"]["scalars"] = dict(zip(lib.SCALARS, (int(x) for x in counters[:len(lib.SCALARS)])))
        result["plain_atomics"] = {"sample_ms": _median_ms(plain), "sample_lds_ms": kernel_ms, "hot_case": _hot_case(arguments.repeats)}
        session = WorkflowSession(prefix + ".fa", prefix + ".gtf", params={"disable_filters": ["blacklist"]})
        seconds = {"without": [], "with": []}
        for repeat in range(2 * (arguments.repeats + 1)):
            which = "with" if repeat % 2 else "without"
            before = time.perf_counter()
            session.sample(prefix + ".bam", os.path.join(output, "fusions.tsv"), rna_metrics_file=os.path.join(output, "metrics.tsv") if which == "with" else None)
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
