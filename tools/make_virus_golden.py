#!/usr/bin/env python3
"""Makes the fixtures of tests/test_virus_expression.py under tests/golden/virus_expression: the SAM text of every case of tests/virus_expression_lib.py and the table that the
reference's scripts/quantify_virus_expression.sh writes for it -- the script itself, run from a checkout of the reference with `LC_ALL=C`, mawk as awk, and a stand-in for
`samtools` that this tool writes into a temporary directory (it answers `--version-only` and prints the SAM text of `view -F 4 -h FILE`: the @SQ lines and the lines whose flag
has bit 4 clear).  The text given to the script holds the @SQ lines only: the script counts every other header line into its total (the first deviation).

    python tools/make_virus_golden.py /path/to/reference [--toy3k PREFIX_OF_THE_DATASET]

Nothing of the script is copied anywhere; no test, smoke() or bench leg calls this tool.  toy3k: the dataset's BAM as SAM text (tools/bam_to_sam.py), tables only (default
patterns, and VIRAL_CONTIGS='^GL' for the -v test): its input is the dataset the tests generate, not a fixture."""
import argparse
import os
import stat
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import virus_expression_lib as lib  # noqa: E402

STAND_IN = """#!/usr/bin/env python3
import sys
if "--version-only" in sys.argv: print("1.19"); sys.exit(0)
sys.stdout.writelines(line for line in open(sys.argv[-1]) if line.startswith("@SQ\\t") or (not line.startswith("@") and not int(line.split("\\t")[1]) & 4))
"""


def run_script(script, sam_path, viral_contigs=None):
    with tempfile.TemporaryDirectory() as scratch:
        stand_in = os.path.join(scratch, "samtools")
        open(stand_in, "w").write(STAND_IN)
        os.chmod(stand_in, os.stat(stand_in).st_mode | stat.S_IXUSR)
        os.symlink("/usr/bin/mawk", os.path.join(scratch, "awk"))
        environment = dict(os.environ, PATH=scratch + os.pathsep + os.environ["PATH"], LC_ALL="C")
        if viral_contigs is not None:
            environment["VIRAL_CONTIGS"] = viral_contigs
        out = os.path.join(scratch, "table.tsv")
        subprocess.run(["bash", script, sam_path, out], check=True, env=environment, stdin=subprocess.DEVNULL)
        return open(out, "rb").read()


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument("reference", help="a checkout of the reference (scripts/quantify_virus_expression.sh is run from there)")
    parser.add_argument("--toy3k", help="prefix of the generated toy3k dataset (PREFIX.bam)")
    parser.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "virus_expression"))
    arguments = parser.parse_args()
    script = os.path.join(arguments.reference, "scripts", "quantify_virus_expression.sh")
    os.makedirs(arguments.out, exist_ok=True)
    for name, case in sorted(lib.fixture_cases().items()):
        sam_path = os.path.join(arguments.out, name + ".sam")
        open(sam_path, "wb").write(lib.sam_text(case))
        table = run_script(script, sam_path)
        open(os.path.join(arguments.out, name + ".tsv"), "wb").write(table)
        print("%-10s %6d bytes of SAM text, %2d rows, restatement %s" % (name, os.path.getsize(sam_path), table.count(b"\n") - 1, "equal" if lib.restate(case)[0] == table else "DIFFERS"))
    if arguments.toy3k:
        from bam_to_sam import bam_to_sam
        with tempfile.TemporaryDirectory() as scratch:
            sam_path = os.path.join(scratch, "toy3k.sam")
            text = bam_to_sam(open(arguments.toy3k + ".bam", "rb").read())[0]
            open(sam_path, "wb").write(b"".join(line + b"\n" for line in text.split(b"\n") if line and (line.startswith(b"@SQ\t") or not line.startswith(b"@"))))
            for suffix, pattern in (("", None), ("_GL", "^GL")):
                table = run_script(script, sam_path, pattern)
                open(os.path.join(arguments.out, "toy3k%s.tsv" % suffix), "wb").write(table)
                print("toy3k%-5s %2d rows: %s" % (suffix, table.count(b"\n") - 1, table.decode().split("\n")[1:-1]))


if __name__ == "__main__":
    main()
