#!/usr/bin/env python3
"""Times -c beside the one-file input: one gen_synth sample as STAR --chimOutType WithinBAM would write it, and the same sample split by tools/split_chimeric.py (variant clean)
through -c, three runs each through a resident session of the workflow library (arriba_workflow_sample / arriba_workflow_sample_separate: what arriba_workflow_run does per sample),
on one MI355X.  Writes the seconds of every run and, from a profiled run of each, the kernel times of the ingest -- the role instantiations of record_parse_kernel and
group_replay_kernel, the keys of the name look-up (separate_name_key_kernel and its sort) and the sorts of the merge -- as JSON.

    python tools/time_separate_chimeric.py [--fragments 10000000] [--out profiles/separate_chimeric_time_10m.json] [--keep DIRECTORY]

Known gap: the sorts of agpu_separate_adopt and of the merge are timed on the device but are not in the profile this tool reads behind the sample.
The split is pure Python over the whole file: minutes at 10^7 fragments, and not part of what is timed."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import split_chimeric  # noqa: E402

INGEST_KERNELS = ("record_parse_kernel", "group_replay_kernel", "separate_name_key_kernel", "names of the separate chimeric file", "name chunk of the merged batch", "fragment_pack_kernel", "record keys")


def kernel_times(launches):
    """{label: [launches, ms]} of the launches of the ingest"""
    times = {}
    for name, ms, _ in launches:
        if any(part in name for part in INGEST_KERNELS):
            entry = times.setdefault(name, [0, 0.0])
            entry[0] += 1
            entry[1] += ms
    return {name: {"launches": count, "ms": round(ms, 3)} for name, (count, ms) in sorted(times.items())}


def main():
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--fragments", type=int, default=10000000)
    parser.add_argument("--out", default=os.path.join(ROOT, "profiles", "separate_chimeric_time_10m.json"))
    parser.add_argument("--keep", help="directory for the sample (default: a temporary one, removed at the end)")
    parser.add_argument("--runs", type=int, default=3)
    args = parser.parse_args()
    from arriba_amd.pipeline import WorkflowSession
    scratch = tempfile.TemporaryDirectory(prefix="time_separate_", dir="/dev/shm" if os.path.isdir("/dev/shm") else None) if not args.keep else None
    directory = args.keep or scratch.name
    os.makedirs(directory, exist_ok=True)
    prefix = os.path.join(directory, "sample")
    subprocess.run([os.path.join(ROOT, "arriba_amd", "lib", "gen_synth"), "--out", prefix, "--seed", "5", "--fragments", str(args.fragments), "--normal-mult", "0.4", "--contigs", "24",
                    "--contig-len", "2000000", "--junctions", str(max(60, args.fragments // 2000))], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    started = time.perf_counter()
    chimeric, main_file, moved = split_chimeric.split(open(prefix + ".bam", "rb").read(), "clean")
    for path, data in ((prefix + ".C.bam", chimeric), (prefix + ".R.bam", main_file)):
        with open(path, "wb") as out:
            out.write(data)
    result = {"fragments": args.fragments, "records_moved_to_c": moved, "split_seconds": round(time.perf_counter() - started, 2), "runs": args.runs, "whole": {}, "separate": {}}
    session = WorkflowSession(prefix + ".fa", prefix + ".gtf", params={"disable_filters": ["blacklist"]})
    try:
        outputs = (prefix + ".fusions.tsv", prefix + ".discarded.tsv")
        samples = {"whole": lambda: session.sample(prefix + ".bam", *outputs), "separate": lambda: session.sample_separate(prefix + ".C.bam", prefix + ".R.bam", *outputs)}
        for kind, sample in samples.items():
            sample()  # (warm-up: the lane allocates its buffers with its first sample)
            seconds = []
            for _ in range(args.runs):
                before = time.perf_counter()
                report = sample()
                seconds.append(round(time.perf_counter() - before, 4))
            result[kind] = {"seconds": seconds, "median_seconds": statistics.median(seconds), "fragments_read": dict(report).get("read_chimeric_alignments"), "timing": {k: round(v, 4) for k, v in session.timing.items() if v}}
            session.set_profiling(True)
            sample()
            result[kind]["kernels"] = kernel_times(session.kernel_profile())
            session.set_profiling(False)
    finally:
        session.close()
    with open(args.out, "w") as out:
        json.dump(result, out, indent=1, sort_keys=True)
        out.write("\n")
    print(json.dumps({kind: result[kind]["median_seconds"] for kind in ("whole", "separate")}))
    if scratch:
        scratch.cleanup()


if __name__ == "__main__":
    main()
