#!/usr/bin/env python3
"""One-off measurement (not a test): --realign-reads on the 10^7-fragment sample of bench.py (its generator, its scratch directory), once as the chimeric-only mix and once with
4 N ordinary proper pairs, which is the workload the option is for.

Per mix one DevicePipeline ingests the sample and writes the coverage track once (for depth_mark_kernel, the project's yardstick for one pass over the records), then splits the
stream `--repeats` + 1 times per form of the text kernel (the first repeat warms buffers and the first launch of every kernel and is reported apart): the wavefront form, which is
the default, and the lane form (ARRIBA_REALIGN_TEXT_FORM=lane).  The windows of text of both files are fetched into the two pinned buffers and dropped: no file is written, so that
the numbers are those of the device and of the copies.  Prints one JSON object:
  mixes   per mix and form: passes_seconds (name | verdict | scan | text with its copies, from the HIP events of agpu_realign_*, medians), kernels_median_ms per kernel and
          rocPRIM call of agpu_realign.hip, text_GB_per_s (output bytes over the time of the text kernel alone) and its fraction of the achievable HBM bandwidth, wall_seconds,
          the statistics; and depth_mark_kernel of the same sample

    python tools/time_realign_split.py [--fragments 10000000] [--repeats 2] > profiles/NAME.json"""
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
ACHIEVABLE_HBM_GB_PER_S = 6300.0  # (what a streaming copy reaches on the MI355X; the peak of the specification is 8 000)


def _kernels(pipeline, prefixes):
    kernels = {}
    for name, ms, size in pipeline.kernel_profile():
        if name.startswith(prefixes):
            entry = kernels.setdefault(name, {"launches": 0, "ms": 0.0})
            entry["launches"] += 1; entry["ms"] += ms
    for entry in kernels.values():
        entry["ms"] = round(entry["ms"], 3)
    return kernels


def _split(pipeline, buffers, capacity):
    """agpu_realign_begin, every window of both files, agpu_realign_end -> the statistics"""
    from arriba_amd import _capi
    from arriba_amd.pipeline import realign_stats_of
    lib, handle, api = pipeline.session._lib, pipeline.session._session, pipeline.api
    contigs, plan, info, stats, got = _capi.DepthContigs(), _capi.RealignPlan(), _capi.RealignInfo(), _capi.RealignStats(), ctypes.c_uint64()
    assert lib.ahost_depth_contigs_of_session(handle, ctypes.byref(contigs)) == 0 and lib.ahost_realign_plan_of_session(handle, ctypes.byref(plan)) == 0
    pipeline._check(api.realign_begin(pipeline.ctx, plan.in_assembly, contigs.names, contigs.name_offset, contigs.n_ref, 1, ctypes.byref(info)))
    try:
        assert info.window_bytes <= capacity
        for which in (0, 1):
            turn = 0
            while True:
                pipeline._check(api.realign_next(pipeline.ctx, which, buffers[turn & 1], capacity, ctypes.byref(got)))
                if got.value == 0:
                    break
                turn += 1
    finally:
        pipeline._check(api.realign_end(pipeline.ctx, ctypes.byref(stats)))
    return realign_stats_of(stats)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--fragments", type=int, default=10000000)
    parser.add_argument("--repeats", type=int, default=2)
    parser.add_argument("--mixes", default="0,4", help="ordinary proper pairs per chimeric fragment, one sample each (bench.py's leg value_with_normal_pairs: 4)")
    arguments = parser.parse_args()
    import bench
    import datasets
    from arriba_amd.pipeline import DevicePipeline, HostSession
    result = {"fragments": arguments.fragments, "achievable_hbm_GB_per_s": ACHIEVABLE_HBM_GB_PER_S, "mixes": {}}
    for normal_mult in [int(value) for value in arguments.mixes.split(",")]:
        directory = bench.scratch_directory(arguments.fragments * 600 * (1 + normal_mult))
        output = tempfile.mkdtemp(prefix="time_realign_split_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
        try:
            prefix = os.path.join(directory, "bench")
            workload = bench.workload_args(arguments.fragments, 1000, 0, False)
            workload[workload.index("--normal-mult") + 1] = str(normal_mult)
            subprocess.run([datasets.GEN_SYNTH, "--out", prefix, "--threads", str(min(64, bench.cpu_budget()))] + workload, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            pipeline = DevicePipeline(HostSession(prefix + ".fa", prefix + ".gtf"), bam=prefix + ".bam", piece_bytes=256 << 20)
            records = int(pipeline.ingest_result.records)
            mix = {"normal_mult": normal_mult, "bam_bytes": os.path.getsize(prefix + ".bam"), "records": records, "forms": {}}
            pipeline.set_profiling(True)
            pipeline.write_coverage(os.path.join(output, "track.bedgraph"))
            mix["depth_mark_kernel_ms"] = _kernels(pipeline, ("depth_mark_kernel",)).get("depth_mark_kernel", {}).get("ms")
            pipeline.set_profiling(False)
            os.remove(os.path.join(output, "track.bedgraph"))
            capacity = 16 << 20
            buffers = [pipeline.api.host_alloc(capacity) for _ in range(2)]
            assert all(buffers)
            for form in ("wave", "lane"):
                os.environ["ARRIBA_REALIGN_TEXT_FORM"] = form
                repeats = []
                for repeat in range(arguments.repeats + 1):
                    pipeline.set_profiling(True)  # (a new epoch: the launches of this repeat only)
                    before = time.perf_counter()
                    stats = _split(pipeline, buffers, capacity)
                    wall = time.perf_counter() - before
                    repeats.append({"warm_up": repeat == 0, "wall_seconds": round(wall, 4), "passes_seconds": {key: round(value, 6) for key, value in stats["seconds"].items()}, "kernels": _kernels(pipeline, ("realign",))})
                    pipeline.set_profiling(False)
                timed = [entry for entry in repeats if not entry["warm_up"]]
                entry = {"repeats": repeats}
                entry["passes_seconds"] = {key: statistics.median(one["passes_seconds"][key] for one in timed) for key in timed[0]["passes_seconds"]}
                entry["wall_seconds"] = statistics.median(one["wall_seconds"] for one in timed)
                entry["kernels_median_ms"] = {kernel: statistics.median(one["kernels"][kernel]["ms"] for one in timed) for kernel in timed[0]["kernels"]}
                entry["counters"] = {key: value for key, value in stats.items() if key != "seconds"}
                text_ms = entry["kernels_median_ms"].get("realign_text_kernel<%s>" % form)
                entry["text_bytes"] = stats["realign_bytes"] + stats["kept_bytes"]
                entry["text_GB_per_s"] = round(entry["text_bytes"] / 1e6 / text_ms, 1) if text_ms else None
                entry["text_fraction_of_achievable_hbm"] = round(entry["text_GB_per_s"] / ACHIEVABLE_HBM_GB_PER_S, 4) if text_ms else None
                entry["text_kernel_against_depth_mark_kernel"] = round(text_ms / mix["depth_mark_kernel_ms"], 2) if text_ms and mix["depth_mark_kernel_ms"] else None
                mix["forms"][form] = entry
            os.environ.pop("ARRIBA_REALIGN_TEXT_FORM", None)
            for buffer in buffers:
                pipeline.api.host_free(buffer)
            pipeline.close()
            result["mixes"]["normal_mult_%d" % normal_mult] = mix
        finally:
            shutil.rmtree(output, ignore_errors=True)
            shutil.rmtree(directory, ignore_errors=True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
