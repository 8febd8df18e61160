#!/usr/bin/env python3
"""One-off measurement (not a test): --indel-sites on the synthetic sample of bench.py (its generator, its scratch directory; 2 x 100 bases) with --indels, 10^7 fragments by
default.  Ingests the sample once, then finds indel sites `--repeats` + 1 times per setting (the default thresholds; min_alt 1 without a percent test, where every event is a
candidate) (the first repeat warms buffers and the first launch of every kernel and is reported apart).  Prints one JSON line:
  passes_seconds     count | fill | group | counters | rows, from the HIP events of agpu_indel_sites, medians
  kernels_median_ms  per kernel and rocPRIM call of agpu_indels.hip and the reused counter kernels
  must_read          the bytes a pass of indel_event_kernel has to read, from the sample: per record the offset (8) and the head with the CIGAR (36 + 4 per operation, name
                     skipped; the generator's records have two operations, three with an indel); per event the SEQ bytes of an insertion (2 at the most for 1 to 3 bases) and the
                     assembly under the normalisation (2 bytes a step of a deletion, 1 of an insertion; a handful: 8 is taken)
  event_kernel_GB_per_s, share_of_hbm_peak   those bytes over the time of each pass, against 8 TB/s
  fill_over_count    the fill pass against the count pass of the same run

    python tools/time_indel_sites.py [--fragments 10000000] [--indels 0.02] [--normal-mult 0] [--repeats 3] > profiles/NAME.json"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
HBM_PEAK_GB_PER_S = 8000.0
COUNTERS = ("records", "contributing", "operations", "events", "unkeyed_insertions", "shift_capped", "runs", "candidates", "sites", "reported", "peak_bytes")


def _kernels(pipeline, prefixes):
    kernels = {}
    for name, ms, size in pipeline.kernel_profile():
        if name.startswith(prefixes):
            entry = kernels.setdefault(name, {"launches": 0, "ms": 0.0})
            entry["launches"] += 1; entry["ms"] += ms
    return kernels


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--fragments", type=int, default=10000000)
    parser.add_argument("--indels", type=float, default=0.02)
    parser.add_argument("--normal-mult", type=int, default=0)
    parser.add_argument("--repeats", type=int, default=3)
    parser.add_argument("--min-mapq", type=int, default=20)
    arguments = parser.parse_args()
    import bench
    import datasets
    from arriba_amd.pipeline import DevicePipeline, HostSession
    directory = bench.scratch_directory(arguments.fragments * 600 * (1 + arguments.normal_mult))
    try:
        prefix = os.path.join(directory, "bench")
        workload = bench.workload_args(arguments.fragments, 1000, 0, False) + ["--indels", str(arguments.indels)]
        workload[workload.index("--normal-mult") + 1] = str(arguments.normal_mult)
        started = time.time()
        subprocess.run([datasets.GEN_SYNTH, "--out", prefix, "--threads", str(min(64, bench.cpu_budget()))] + workload, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        result = {"fragments": arguments.fragments, "indels": arguments.indels, "normal_mult": arguments.normal_mult, "bam_bytes": os.path.getsize(prefix + ".bam"), "generate_seconds": round(time.time() - started, 1), "min_mapq": arguments.min_mapq}
        pipeline = DevicePipeline(HostSession(prefix + ".fa", prefix + ".gtf"), bam=prefix + ".bam", piece_bytes=256 << 20)
        result["records"] = records = int(pipeline.ingest_result.records)
        result["stream_bytes"] = int(pipeline.ingest_result.stream_bytes)
        result["settings"] = {}
        for name, min_alt, min_percent in (("defaults", 3, 5), ("every_event_a_candidate", 1, 0)):  # (the second: the counters and the rows over as many sites as there are events)
            repeats = []
            for repeat in range(arguments.repeats + 1):
                pipeline.set_profiling(True)  # (a new epoch: the launches of this repeat only)
                before = time.perf_counter()
                rows, stats = pipeline.indel_sites(arguments.min_mapq, min_alt, min_percent)
                wall = time.perf_counter() - before
                repeats.append({"warm_up": repeat == 0, "wall_seconds": round(wall, 4), "passes_seconds": {key: round(value, 6) for key, value in stats["seconds"].items()},
                                "kernels": {kernel: round(entry["ms"], 3) for kernel, entry in _kernels(pipeline, ("indel", "allele")).items()}})
                pipeline.set_profiling(False)
            timed = [entry for entry in repeats if not entry["warm_up"]]
            entry = {"min_alt": min_alt, "min_percent": min_percent, "repeats": repeats}
            entry["counters"] = {key: stats[key] for key in COUNTERS}
            entry["passes_seconds"] = {key: statistics.median(one["passes_seconds"][key] for one in timed) for key in timed[0]["passes_seconds"]}
            entry["kernels_median_ms"] = {kernel: statistics.median(one["kernels"][kernel] for one in timed) for kernel in timed[0]["kernels"]}
            entry["wall_seconds"] = statistics.median(one["wall_seconds"] for one in timed)
            result["settings"][name] = entry
        pipeline.close()
        operations = result["settings"]["defaults"]["counters"]["operations"]
        must = {"offsets_heads_cigars": records * (8 + 36 + 4 * 2) + operations * 4, "seq_of_events": operations * 2, "assembly_of_events": operations * 8}
        must["total"] = sum(must.values())
        result["must_read"] = must
        for which in ("count", "fill"):
            seconds = result["settings"]["defaults"]["passes_seconds"][which]
            if seconds > 0:
                result["event_kernel_%s_GB_per_s" % which] = round(must["total"] / 1e9 / seconds, 1)
                result["event_kernel_%s_share_of_hbm_peak" % which] = round(must["total"] / 1e9 / seconds / HBM_PEAK_GB_PER_S, 4)
        passes = result["settings"]["defaults"]["passes_seconds"]
        if passes["count"] > 0:
            result["fill_over_count"] = round(passes["fill"] / passes["count"], 3)
        print(json.dumps(result))
    finally:
        shutil.rmtree(directory, ignore_errors=True)


if __name__ == "__main__":
    main()
