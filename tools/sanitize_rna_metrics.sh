#!/bin/bash
# tools/sanitize_rna_metrics.sh -- the host side of --rna-metrics under AddressSanitizer and UBSan (test tooling): a stand-alone program (tools/rna_metrics_main.cpp) built together
# with the host sources, run on the committed case of tests/golden/rna_metrics as SAM text, on the same case as a raw BAM stream, on one seeded case and the record with 601 CIGAR
# operations of tests/rna_metrics_lib.py on a seeded annotation (TLEN at both ends of its range, POS 0, reads past the end of a reference, optional fields of several types), on
# those streams cut short inside their last records, and on the interval files cut short; the tables it writes are compared with the committed one and with the restatement's.
# CPU only: nothing is loaded into python, nothing goes through a GPU.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
WORK=$(mktemp -d /tmp/sanitize_rna_metrics_XXXXXX)
trap 'rm -rf $WORK' EXIT
GOLDEN=$ROOT/tests/golden/rna_metrics
# (python only writes the inputs and the expected tables here)
python3 - $ROOT $WORK <<'PY'
import os, sys
root, work = sys.argv[1], sys.argv[2]
sys.path[:0] = [os.path.join(root, "tests")]
import rna_metrics_lib as lib
committed = lib.load_annotation()
prefix = lib.write_seeded_annotation(1900, work)
seeded = lib.load_annotation(prefix + ".gtf", prefix + ".fa", prefix + ".bed")
for name, annotation, case in (("hand_made", committed, lib.parse_sam(open(os.path.join(lib.GOLDEN, "hand_made.sam"), "rb").read())), ("seed1900", seeded, lib.random_case(1900, seeded)),
                               ("long_cigar", seeded, lib.long_cigar_case(seeded))):
    open(os.path.join(work, name + ".raw"), "wb").write(lib.bam_header(case[0]) + lib.bam_records(case))
    open(os.path.join(work, name + ".expected"), "wb").write(lib.restate(annotation, case)[0])
    open(os.path.join(work, name + ".reference"), "w").write(os.path.join(lib.GOLDEN, "hand_made") if annotation is committed else prefix)
PY
g++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$ROOT/include -I$ROOT/arriba_amd/csrc/host -o $WORK/rna_metrics_main $ROOT/tools/rna_metrics_main.cpp $ROOT/arriba_amd/csrc/host/*.cpp -lz
echo "== -fsanitize=address,undefined: hand_made.sam"
ASAN_OPTIONS=detect_leaks=0 $WORK/rna_metrics_main $GOLDEN/hand_made.fa $GOLDEN/hand_made.gtf "r1 r2" $GOLDEN/hand_made.sam $GOLDEN/hand_made.bed $WORK/text.tsv
cmp $WORK/text.tsv $GOLDEN/hand_made.tsv
for RAW in $WORK/*.raw; do
	NAME=$(basename $RAW .raw)
	REFERENCE=$(cat $WORK/$NAME.reference)
	echo "== -fsanitize=address,undefined: $NAME"
	ASAN_OPTIONS=detect_leaks=0 $WORK/rna_metrics_main $REFERENCE.fa $REFERENCE.gtf "r1 r2 s1 s2" $RAW $REFERENCE.bed $WORK/$NAME.tsv
	cmp $WORK/$NAME.tsv $WORK/$NAME.expected
	test ! -e $WORK/$NAME.tsv.tmp
done
cmp $WORK/hand_made.tsv $GOLDEN/hand_made.tsv
echo "sanitize_rna_metrics: clean"
