#!/usr/bin/env python3
"""Writes tests/golden/separate_<dataset>/: what the unmodified reference makes of `-c C -x R`, with C and R split off the generated WithinBAM file of the dataset by
tools/split_chimeric.py (variant clean).  Only its log and its two output files are kept; meta.json holds the command.  Needs the oracle build of the reference
(oracle/_ref/arriba_ref) and the built tools (gen_synth).

    python tools/make_separate_golden.py [dataset ...]"""
import gzip
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import datasets  # noqa: E402
import separate_chimeric_lib as lib  # noqa: E402


def main():
    for name in sys.argv[1:] or lib.DATASETS:
        directory = tempfile.mkdtemp(prefix="separate_" + name + "_")
        prefix = datasets.generate(datasets.DATASETS[name], directory)
        chimeric, main_file = lib.split_files(prefix, "clean")
        outputs = (prefix + ".fusions.tsv", prefix + ".discarded.tsv")
        log, command = lib.run_reference(prefix, chimeric, main_file, outputs)
        golden = lib.golden_directory(name)
        os.makedirs(golden, exist_ok=True)
        with open(os.path.join(golden, "reference.log"), "w") as out:
            out.write(log)
        for path, file_name in zip(outputs, ("fusions.tsv", "discarded.tsv")):
            with gzip.GzipFile(os.path.join(golden, file_name + ".gz"), "wb", mtime=0) as out:
                out.write(open(path, "rb").read())
        with open(os.path.join(golden, "meta.json"), "w") as out:
            json.dump({"dataset": name, "spec": datasets.DATASETS[name], "split": "tools/split_chimeric.py --variant clean", "command": ["arriba_ref"] + command[1:],
                       "reference": "suhrig/arriba v2.5.1, built by oracle/Makefile"}, out, indent=1, sort_keys=True)
        print(name, lib.totals_of(log))


if __name__ == "__main__":
    main()
