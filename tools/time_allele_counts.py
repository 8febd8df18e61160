#!/usr/bin/env python3
"""One-off measurement (not a test): --allele-counts on the 10^7-fragment sample of bench.py with 4 N ordinary proper pairs (its generator, its scratch directory), the output on
tmpfs.  The sites are seeded: half of them inside exons of the generated annotation (where the reads are, so these are the deep ones), half anywhere on the references of the
header.

One DevicePipeline ingests the sample and writes the coverage track once (for depth_mark_kernel, the project's yardstick for one pass over the records: the same CIGAR walk over
the same bytes), then counts alleles `--repeats` + 1 times per setting (the first repeat warms buffers and the first launch of every kernel and is reported apart): 10^5 and 10^6
sites; at 10^5 sites also without the window bitmap (ARRIBA_ALLELE_NO_BITMAP=1) and with one atomic per lane instead of the leader loop (ARRIBA_ALLELE_PLAIN_ATOMICS=1) -- the
exonic half of the sites is the hot-site case: `deepest` says how many records the deepest site takes.  Then a WorkflowSession runs the sample `--repeats` + 1 times without the
option -- what the parent commit does for a sample -- and as often with it (10^5 sites).  Prints one JSON object:
  settings         per setting: passes_seconds (sites | count | rows, from the HIP events of agpu_allele_counts, medians), kernels_median_ms per kernel and rocPRIM call of
                   agpu_alleles.hip, wall_seconds, the statistics, the deepest site
  against          allele_count_kernel of every setting beside depth_mark_kernel: ms, and GB/s over records x 72 bytes (the offset and the line that holds the head of a record)
  sample_seconds   the wall clock of arriba_workflow_sample without the option and with it (medians), and added_wall_seconds: what one sample alone pays for the option

    python tools/time_allele_counts.py [--fragments 10000000] [--normal-mult 4] [--repeats 3] > profiles/NAME.json"""
import argparse
import ctypes
import json
import os
import random
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
KNOBS = ("ARRIBA_ALLELE_NO_BITMAP", "ARRIBA_ALLELE_PLAIN_ATOMICS")


def _kernels(pipeline, prefixes):
    kernels = {}
    for name, ms, size in pipeline.kernel_profile():
        if name.startswith(prefixes):
            entry = kernels.setdefault(name, {"launches": 0, "ms": 0.0})
            entry["launches"] += 1; entry["ms"] += ms
    for entry in kernels.values():
        entry["ms"] = round(entry["ms"], 3)
    return kernels


def _write_sites(path, count, exons, references, seed):
    """`count` seeded sites, half of them inside exons; references: [(name, LN)]"""
    generator = random.Random(seed)
    total = sum(length for _, length in references)
    with open(path, "w") as out:
        for k in range(count):
            if k % 2 == 0 and exons:
                contig, start, end = exons[generator.randrange(len(exons))]
                out.write("%s\t%d\n" % (contig, generator.randint(start, end)))
            else:
                at = generator.randrange(total)
                for name, length in references:
                    if at < length:
                        out.write("%s\t%d\n" % (name, at + 1))
                        break
                    at -= length


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
    output = tempfile.mkdtemp(prefix="time_allele_counts_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
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
        # the sites: exons of the annotation, references of the header
        contigs = _capi.DepthContigs()
        assert pipeline.session._lib.ahost_depth_contigs_of_session(pipeline.session._session, ctypes.byref(contigs)) == 0
        lengths = ctypes.cast(contigs.length, ctypes.POINTER(ctypes.c_uint32))
        offsets = ctypes.cast(contigs.name_offset, ctypes.POINTER(ctypes.c_uint32))
        names = ctypes.string_at(contigs.names, offsets[contigs.n_ref]).decode()
        references = [(names[offsets[t]:offsets[t + 1]], int(lengths[t])) for t in range(contigs.n_ref)]
        length_of = dict(references)
        exons = []
        for line in open(prefix + ".gtf"):
            fields = line.split("\t")
            if len(fields) > 4 and fields[2] == "exon" and fields[0] in length_of:
                exons.append((fields[0], int(fields[3]), min(int(fields[4]), length_of[fields[0]])))
        result["references"] = len(references); result["reference_bases"] = sum(length for _, length in references); result["exons"] = len(exons)
        sites_of = {}
        for count in (100000, 1000000):
            sites_of[count] = os.path.join(output, "sites_%d.tsv" % count)
            _write_sites(sites_of[count], count, exons, references, count)
        # the yardstick of the same session
        pipeline.set_profiling(True)
        pipeline.write_coverage(os.path.join(output, "track.bedgraph"))
        depth_ms = _kernels(pipeline, ("depth_mark_kernel",)).get("depth_mark_kernel", {}).get("ms")
        pipeline.set_profiling(False)
        os.remove(os.path.join(output, "track.bedgraph"))
        settings = [("sites_1e5", 100000, {}), ("sites_1e6", 1000000, {}), ("sites_1e5_without_the_bitmap", 100000, {"ARRIBA_ALLELE_NO_BITMAP": "1"}),
                    ("sites_1e5_plain_atomics", 100000, {"ARRIBA_ALLELE_PLAIN_ATOMICS": "1"}), ("sites_1e6_plain_atomics", 1000000, {"ARRIBA_ALLELE_PLAIN_ATOMICS": "1"})]
        result["settings"] = {}
        per_second = lambda ms: round(records * 72 / 1e6 / ms, 1) if ms else None  # noqa: E731
        result["against"] = {"depth_mark_kernel_ms": depth_ms, "depth_mark_kernel_GB_per_s": per_second(depth_ms)}
        for name, count, knobs in settings:
            for knob in KNOBS:
                os.environ.pop(knob, None)
            os.environ.update(knobs)
            repeats = []
            for repeat in range(arguments.repeats + 1):
                pipeline.set_profiling(True)  # (a new epoch: the launches of this repeat only)
                before = time.perf_counter()
                rows, stats, sites = pipeline.allele_counts(sites_of[count], 0, 13)
                wall = time.perf_counter() - before
                pipeline.session._lib.ahost_allele_sites_free(ctypes.byref(sites))
                repeats.append({"warm_up": repeat == 0, "wall_seconds": round(wall, 4), "passes_seconds": {key: round(value, 6) for key, value in stats["seconds"].items()}, "kernels": _kernels(pipeline, ("allele",))})
                pipeline.set_profiling(False)
            timed = [entry for entry in repeats if not entry["warm_up"]]
            entry = {"sites": count, "knobs": knobs, "repeats": repeats}
            entry["passes_seconds"] = {key: statistics.median(one["passes_seconds"][key] for one in timed) for key in timed[0]["passes_seconds"]}
            entry["wall_seconds"] = statistics.median(one["wall_seconds"] for one in timed)
            entry["kernels_median_ms"] = {kernel: statistics.median(one["kernels"][kernel]["ms"] for one in timed) for kernel in timed[0]["kernels"]}
            entry["counters"] = {key: stats[key] for key in ("records", "contributing", "hits", "sites", "placed", "covered", "peak_bytes")}
            entry["deepest"] = max((row.a + row.c + row.g + row.t + row.n + row.del_ + row.skip + row.lowq for row in rows), default=0)
            result["settings"][name] = entry
            count_ms = entry["kernels_median_ms"].get("allele_count_kernel")
            result["against"][name + "_allele_count_kernel_ms"] = count_ms
            result["against"][name + "_allele_count_kernel_GB_per_s"] = per_second(count_ms)
        for knob in KNOBS:
            os.environ.pop(knob, None)
        pipeline.close()
        session = WorkflowSession(prefix + ".fa", prefix + ".gtf", params={"disable_filters": ["blacklist"]})
        seconds = {"without": [], "with": []}
        for repeat in range(2 * (arguments.repeats + 1)):
            which = "with" if repeat % 2 else "without"
            before = time.perf_counter()
            if which == "with":
                session.sample(prefix + ".bam", os.path.join(output, "fusions.tsv"), allele_sites_file=sites_of[100000], allele_counts_file=os.path.join(output, "alleles.tsv"))
            else:
                session.sample(prefix + ".bam", os.path.join(output, "fusions.tsv"))
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
