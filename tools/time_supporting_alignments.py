#!/usr/bin/env python3
"""One-off measurement (not a test): --supporting-alignments on the sample of bench.py (its generator, its scratch directory), the output on tmpfs.

One DevicePipeline ingests the sample, writes the sorted file once (for sorted_bam_key_kernel and sorted_bam_gather_kernel of the same run) and runs the stages up to
fusions.tsv; behind a second ingest of the same file the pool is built `--repeats` + 1 times and the files are written behind each build (the first repeat warms buffers and
the first launch of every kernel and is reported apart).  Prints one JSON object:
  kernels        per kernel / library call of agpu_supporting.hip: launches and ms per repeat (HIP events), GB/s over the bytes the launch declares
  parts_ms       name table + mark | compact + sort | join | gather + frame | copy back, from those events
  against        support_mark_kernel beside sorted_bam_key_kernel (the same access pattern: ms, and ms per 10^6 records); supporting_gather_kernel beside
                 sorted_bam_gather_kernel in GB/s as (bytes read + bytes written) / time
  seconds        build_support_pool and write_supporting_alignments by part, wall clock of the calling thread
  added_wall_seconds   what one sample alone pays for the option: pool + files, the median

    python tools/time_supporting_alignments.py [--fragments 10000000] [--repeats 3] > profiles/NAME.json"""
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

PARTS = (("name_table_mark", ("support_name_insert_kernel", "support_mark_kernel")),
         ("compact_sort", ("support rocprim::exclusive_scan(marks)", "support_compact_kernel", "support rocprim::radix_sort_pairs(pool)", "support_meta_kernel", "support rocprim::exclusive_scan(pool sizes)", "support_pool_copy_kernel")),
         ("join", ("support_pair_kernel", "support rocprim::radix_sort_keys(pairs)", "support_join_kernel(count)", "support rocprim::exclusive_scan(emissions)", "support_join_kernel(emit)", "support rocprim::radix_sort_keys(emissions)",
                   "support_emission_size_kernel", "support rocprim::exclusive_scan(emission sizes)", "support_row_kernel", "support_block_table_kernel")),
         ("gather_frame", ("supporting_gather_kernel",)),
         ("copy_back", ("supporting copy back",)))


def _kernels(pipeline, prefixes):
    kernels = {}
    for name, ms, size in pipeline.kernel_profile():
        if name.startswith(prefixes):
            entry = kernels.setdefault(name, {"launches": 0, "ms": 0.0, "bytes": 0})
            entry["launches"] += 1; entry["ms"] += ms; entry["bytes"] += size
    for entry in kernels.values():
        entry["GB_per_s"] = round(entry["bytes"] / 1e6 / entry["ms"], 1) if entry["ms"] > 0 else None
        entry["ms"] = round(entry["ms"], 3)
    return kernels


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--fragments", type=int, default=10000000)
    parser.add_argument("--repeats", type=int, default=3)
    arguments = parser.parse_args()
    import bench
    from arriba_amd.pipeline import DevicePipeline, HostSession
    directory = bench.scratch_directory(arguments.fragments * 600)
    output = tempfile.mkdtemp(prefix="time_supporting_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        prefix, generate_seconds = bench.generate_sample(arguments.fragments, 1000, directory)
        bam_bytes = os.path.getsize(prefix + ".bam")
        pipeline = DevicePipeline(HostSession(prefix + ".fa", prefix + ".gtf"), bam=prefix + ".bam", piece_bytes=256 << 20)
        records = int(pipeline.ingest_result.records)
        result = {"fragments": arguments.fragments, "bam_bytes": bam_bytes, "records": records, "generate_seconds": round(generate_seconds, 1), "output_on": output, "repeats": []}
        pipeline.set_profiling(True)
        pipeline.write_sorted_bam(os.path.join(output, "sorted.bam"))
        sorted_kernels = _kernels(pipeline, ("sorted_bam_key_kernel", "sorted_bam_gather_kernel"))
        pipeline.set_profiling(False)
        os.remove(os.path.join(output, "sorted.bam")); os.remove(os.path.join(output, "sorted.bam.bai"))
        pipeline.run_workflow(os.path.join(output, "fusions.tsv"))
        rows = pipeline.written_fusion_rows()
        result["rows"], result["listed_names"] = int(rows["ref"].shape[0]), int(rows["names"].size)
        pipeline.read_chimeric_alignments(prefix + ".bam", piece_bytes=256 << 20)  # (the stream again; the batch is the same, so the rows' fragments still say the same names)
        for repeat in range(arguments.repeats + 1):
            pipeline.set_profiling(True)  # (a new epoch: the launches of this repeat only)
            before = time.perf_counter()
            pool = pipeline.build_support_pool()
            pool_seconds = time.perf_counter() - before
            written = pipeline.write_supporting_alignments(os.path.join(output, "support"), rows)
            kernels = _kernels(pipeline, ("support",))
            parts = {part: round(sum(kernels[name]["ms"] for name in names if name in kernels), 3) for part, names in PARTS}
            seconds = dict({key: round(value, 4) for key, value in pipeline.supporting_seconds.items()}, pool=round(pool_seconds, 4))
            result["repeats"].append({"warm_up": repeat == 0, "pool": pool, "written": written, "seconds": seconds, "parts_ms": parts, "kernels": kernels})
            pipeline.set_profiling(False)
        timed = [entry for entry in result["repeats"] if not entry["warm_up"]]
        result["added_wall_seconds"] = round(statistics.median(entry["seconds"]["pool"] + entry["seconds"]["total"] for entry in timed), 4)
        mark = statistics.median(entry["kernels"]["support_mark_kernel"]["ms"] for entry in timed)
        gathers = [entry["kernels"]["supporting_gather_kernel"]["GB_per_s"] for entry in timed if "supporting_gather_kernel" in entry["kernels"]]
        result["against"] = {"support_mark_kernel_ms": mark, "sorted_bam_key_kernel_ms": sorted_kernels.get("sorted_bam_key_kernel", {}).get("ms"), "mark_ms_per_million_records": round(mark / max(records, 1) * 1e6, 4),
                             "supporting_gather_kernel_GB_per_s": statistics.median(gathers) if gathers else None, "sorted_bam_gather_kernel_GB_per_s": sorted_kernels.get("sorted_bam_gather_kernel", {}).get("GB_per_s")}
        pipeline.close()
        print(json.dumps(result))
    finally:
        shutil.rmtree(output, ignore_errors=True)
        shutil.rmtree(directory, ignore_errors=True)


if __name__ == "__main__":
    main()
