#!/usr/bin/env python3
"""One-off measurement (not a test): --sorted-bam on the sample of bench.py (its generator, its scratch directory), the output on tmpfs.

One DevicePipeline ingests the sample; write_sorted_bam runs `--repeats` times behind it (the first one warms buffers, pinned windows and the first launch of every kernel and
is reported apart).  Prints one JSON object:
  kernels        per kernel / library call of agpu_sorted_bam.hip: launches and ms per repeat (HIP events), GB/s over the bytes the launch declares
                 (gather: bytes read + bytes written)
  parts_ms       key + sort + scan | gather + frame | index | copy back, from those events
  seconds        write_sorted_bam by part, wall clock of the calling thread: sort, gather_and_copy (waiting for windows), write (to tmpfs), index, total
  feed           the ingest of the same run: seconds of the feed and its GB/s, to set the copy back against
  added_wall_seconds   what one sample alone pays for the option: the median total

    python tools/time_sorted_bam.py [--fragments 10000000] [--repeats 3] [--compression 1] > profiles/NAME.json
--compression 1 adds "compression": the same repeats at level 1 -- seconds of gather + compress + compact from HIP events, bytes out over bytes in, the copy-back
seconds, the wall seconds one sample pays -- next to the level-0 numbers of the same session and to zlib level 1 on the same blocks on the host (bytes and seconds)."""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

PARTS = (("key_sort_scan", ("sorted_bam_key_kernel", "sorted_bam rocprim::radix_sort_pairs(records)", "sorted_bam rocprim::exclusive_scan(sizes)", "sorted_bam_block_first_kernel")),
         ("gather_frame", ("sorted_bam_gather_kernel",)),
         ("gather_compress_compact", ("sorted_bam_deflate_kernel", "sorted_bam rocprim::exclusive_scan(blocks)", "sorted_bam_compact_kernel")),
         ("index", ("sorted_bam_index_record_kernel", "sorted_bam rocprim::exclusive_scan(run heads)", "sorted_bam_index_chunk_kernel", "sorted_bam rocprim::radix_sort_pairs(chunks)", "sorted_bam_index_fill_kernel", "sorted_bam rocprim::exclusive_scan(offsets)")),
         ("copy_back", ("sorted_bam copy back",)))


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--fragments", type=int, default=10000000)
    parser.add_argument("--repeats", type=int, default=3)
    parser.add_argument("--compression", type=int, choices=(0, 1), default=0, help="1: also time --sorted-bam-compression 1, next to the level-0 run of the same session and to zlib level 1 on the host")
    parser.add_argument("--zlib-blocks", type=int, default=2000, help="record blocks of the level-0 file that zlib level 1 compresses on the host (one thread); its seconds are scaled to the file")
    arguments = parser.parse_args()
    import bench
    from arriba_amd.pipeline import DevicePipeline, HostSession
    directory = bench.scratch_directory(arguments.fragments * 600)
    output = tempfile.mkdtemp(prefix="time_sorted_bam_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    try:
        prefix, generate_seconds = bench.generate_sample(arguments.fragments, 1000, directory)
        bam_bytes = os.path.getsize(prefix + ".bam")
        session = HostSession(prefix + ".fa", prefix + ".gtf")
        pipeline = DevicePipeline(session, bam=prefix + ".bam", piece_bytes=256 << 20)
        result = {"fragments": arguments.fragments, "bam_bytes": bam_bytes, "records": int(pipeline.ingest_result.records), "generate_seconds": round(generate_seconds, 1),
                  "feed": {"seconds": round(pipeline.ingest_seconds["feed"], 3), "GB_per_s": round(bam_bytes / 1e9 / max(pipeline.ingest_seconds["feed"], 1e-9), 2), "device_seconds": round(pipeline.ingest_seconds["device"], 3)},
                  "output_on": output, "repeats": []}
        path = os.path.join(output, "sorted.bam")

        def timed_repeats(level):
            repeats = []
            for repeat in range(arguments.repeats + 1):
                pipeline.set_profiling(True)  # (a new epoch: the launches of this repeat only)
                written = pipeline.write_sorted_bam(path, compression=level)
                kernels = {}
                for name, ms, size in pipeline.kernel_profile():
                    if name.startswith("sorted_bam"):
                        entry = kernels.setdefault(name, {"launches": 0, "ms": 0.0, "bytes": 0})
                        entry["launches"] += 1; entry["ms"] += ms; entry["bytes"] += size
                for entry in kernels.values():
                    entry["GB_per_s"] = round(entry["bytes"] / 1e6 / entry["ms"], 1) if entry["ms"] > 0 else None
                    entry["ms"] = round(entry["ms"], 3)
                parts = {part: round(sum(kernels[name]["ms"] for name in names if name in kernels), 3) for part, names in PARTS}
                repeats.append({"warm_up": repeat == 0, "written": written, "seconds": {key: round(value, 4) for key, value in pipeline.sorted_bam_seconds.items()}, "parts_ms": parts, "kernels": kernels})
                pipeline.set_profiling(False)
            return repeats

        result["repeats"] = timed_repeats(0)
        timed = [entry for entry in result["repeats"] if not entry["warm_up"]]
        result["added_wall_seconds"] = round(statistics.median(entry["seconds"]["total"] for entry in timed), 4)
        result["file_bytes"] = os.path.getsize(path)
        if arguments.compression == 1:  # level 1 next to the level-0 run of the same session, and zlib level 1 on the host over (a sample of) the same blocks
            import time
            import zlib
            import read_bam
            raw = open(path, "rb").read(arguments.zlib_blocks * 65311 + (1 << 20))  # (the level-0 file: header blocks, then stored record blocks)
            payloads, at = [], 0
            while at + 18 <= len(raw) and len(payloads) < arguments.zlib_blocks:
                size = int.from_bytes(raw[at + 16:at + 18], "little") + 1
                if at + size > len(raw):
                    break
                if read_bam.is_stored(raw, at) and size > 31:
                    payloads.append(raw[at + 23:at + size - 8])
                at += size
            started, deflated = time.perf_counter(), 0
            for payload in payloads:
                deflater = zlib.compressobj(1, zlib.DEFLATED, -15)
                deflated += len(deflater.compress(payload) + deflater.flush()) + 26
            zlib_seconds = time.perf_counter() - started
            payload_bytes = sum(len(payload) for payload in payloads)
            level1 = timed_repeats(1)
            timed1 = [entry for entry in level1 if not entry["warm_up"]]
            median = lambda values: round(statistics.median(values), 4)
            result["compression"] = {
                "repeats": level1,
                "gather_compress_compact_seconds": median([entry["parts_ms"]["gather_compress_compact"] / 1e3 for entry in timed1]),
                "level0_gather_frame_seconds": median([entry["parts_ms"]["gather_frame"] / 1e3 for entry in timed]),
                "bytes_in": timed1[0]["written"]["uncompressed_bytes"], "bytes_out": timed1[0]["written"]["file_bytes"],
                "bytes_out_over_bytes_in": round(timed1[0]["written"]["file_bytes"] / max(timed1[0]["written"]["uncompressed_bytes"], 1), 4),
                "copy_back_seconds": median([entry["parts_ms"]["copy_back"] / 1e3 for entry in timed1]), "level0_copy_back_seconds": median([entry["parts_ms"]["copy_back"] / 1e3 for entry in timed]),
                "added_wall_seconds": median([entry["seconds"]["total"] for entry in timed1]), "level0_added_wall_seconds": result["added_wall_seconds"],
                "file_bytes": os.path.getsize(path),
                "zlib_level_1_on_the_host": {"blocks": len(payloads), "bytes_in": payload_bytes, "bytes_out": deflated, "bytes_out_over_bytes_in": round(deflated / max(payload_bytes, 1), 4), "seconds": round(zlib_seconds, 3),
                                             "seconds_scaled_to_the_file": round(zlib_seconds * timed1[0]["written"]["uncompressed_bytes"] / max(payload_bytes, 1), 2), "threads": 1}}
        pipeline.close()
        print(json.dumps(result))
    finally:
        shutil.rmtree(output, ignore_errors=True)
        shutil.rmtree(directory, ignore_errors=True)


if __name__ == "__main__":
    main()
