#!/bin/bash
# tools/sanitize_allele_counts.sh -- the host side of --allele-counts under AddressSanitizer and UBSan (test tooling): a stand-alone program (tools/allele_counts_main.cpp) built
# together with the host sources, run on the committed case of tests/golden/allele_counts as SAM text, on the same case, on one seeded case and on the record with 601 CIGAR
# operations of tests/allele_counts_lib.py as raw BAM streams (SEQ with every code, QUAL with 0xFF, reads past the end of a reference, CIGARs that disagree with l_seq), on those
# streams cut short inside their last records -- SEQ and QUAL end mid-record there -- and on the sites files cut short; the tables it writes are compared with the committed one
# and with the restatement's.
# CPU only: nothing is loaded into python, nothing goes through a GPU.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
WORK=$(mktemp -d /tmp/sanitize_allele_counts_XXXXXX)
trap 'rm -rf $WORK' EXIT
GOLDEN=$ROOT/tests/golden/allele_counts
# (python only writes the inputs and the expected tables here)
python3 - $ROOT $WORK <<'PY'
import os, sys
root, work = sys.argv[1], sys.argv[2]
sys.path[:0] = [os.path.join(root, "tests")]
import allele_counts_lib as lib
assembly = lib.load_assembly()
for name, case in (("hand_made", lib.committed_case()), ("seed1700", lib.random_case(1700)), ("long_cigar", lib.long_cigar_case()), ("dense", lib.dense_case())):
    open(os.path.join(work, name + ".raw"), "wb").write(lib.bam_header(case["references"]) + lib.bam_records(case))
    open(os.path.join(work, name + ".sites"), "wb").write(case["sites"])
    open(os.path.join(work, name + ".thresholds"), "w").write("%d %d\n" % (case["min_mapq"], case["min_baseq"]))
    open(os.path.join(work, name + ".expected"), "wb").write(lib.restate(assembly, case)[0])
PY
g++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$ROOT/include -I$ROOT/arriba_amd/csrc/host -o $WORK/allele_counts_main $ROOT/tools/allele_counts_main.cpp $ROOT/arriba_amd/csrc/host/*.cpp -lz
echo "== -fsanitize=address,undefined: hand_made.sam"
ASAN_OPTIONS=detect_leaks=0 $WORK/allele_counts_main $GOLDEN/hand_made.fa $GOLDEN/hand_made.gtf "a1 2" $GOLDEN/hand_made.sam $GOLDEN/hand_made.sites 20 13 $WORK/text.tsv
cmp $WORK/text.tsv $GOLDEN/hand_made.tsv
for RAW in $WORK/*.raw; do
	NAME=$(basename $RAW .raw)
	echo "== -fsanitize=address,undefined: $NAME"
	ASAN_OPTIONS=detect_leaks=0 $WORK/allele_counts_main $GOLDEN/hand_made.fa $GOLDEN/hand_made.gtf "a1 2" $RAW $WORK/$NAME.sites $(cat $WORK/$NAME.thresholds) $WORK/$NAME.tsv
	cmp $WORK/$NAME.tsv $WORK/$NAME.expected
	test ! -e $WORK/$NAME.tsv.tmp
done
cmp $WORK/hand_made.tsv $GOLDEN/hand_made.tsv
echo "sanitize_allele_counts: clean"
