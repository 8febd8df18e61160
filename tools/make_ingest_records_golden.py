#!/usr/bin/env python3
"""tools/make_ingest_records_golden.py -- regenerate tests/golden/ingest_records/<dataset>/ (test tooling).

For every dataset of tests/ingest_records_lib.py: the generator's BAM file, re-dressed (new QNAMEs and aux blocks, see the library), written as a raw BAM stream and read by
the oracle build of the UNMODIFIED reference (oracle/_ref/arriba_ref_dump).  Kept: the read table behind annotation (gzipped), the log, and meta.json with the SHA-256 of the
re-dressed file -- the tests regenerate the file and assert the checksum, so the fixtures cannot drift.  Needs oracle/_ref; the tests only need the committed files.
"""
import gzip
import hashlib
import json
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import datasets  # noqa: E402
import ingest_records_lib  # noqa: E402


def main():
    only = sys.argv[1:]
    for name, spec in ingest_records_lib.DATASETS.items():
        if only and name not in only:
            continue
        work = tempfile.mkdtemp(prefix="golden_" + name + "_")
        base = datasets.generate(spec, work)
        prefix, table = ingest_records_lib.write_dressed(base, os.path.join(work, "dressed"))
        dump = os.path.join(work, "dump")
        os.makedirs(dump)
        os.environ["ARRIBA_ORACLE_DUMP_LISTS"] = "0"
        log = datasets.run_reference(prefix, dump, spec)
        target = os.path.join(ROOT, "tests", "golden", "ingest_records", name)
        shutil.rmtree(target, ignore_errors=True)
        os.makedirs(target)
        for entry in sorted(os.listdir(dump)):
            if entry.startswith("reads.") and entry.endswith("_annotated.tsv"):
                with open(os.path.join(dump, entry), "rb") as source, gzip.GzipFile(os.path.join(target, entry + ".gz"), "wb", mtime=0) as out:
                    shutil.copyfileobj(source, out)
        with open(os.path.join(target, "reference.log"), "w") as out:
            out.write(log)
        meta = {"dataset": name, "spec": spec, "bam_sha256": hashlib.sha256(open(prefix + ".bam", "rb").read()).hexdigest(),
                "reference": "suhrig/arriba v2.5.1 sources, built by oracle/Makefile"}
        with open(os.path.join(target, "meta.json"), "w") as out:
            json.dump(meta, out, indent=1, sort_keys=True)
        print("%s: %s, %.1f KiB" % (name, sorted(os.listdir(target)), sum(os.path.getsize(os.path.join(target, f)) for f in os.listdir(target)) / 1024.0))
        shutil.rmtree(work)


if __name__ == "__main__":
    main()
