#!/bin/bash
# tools/sanitize_splice_junctions.sh -- the host side of --splice-junctions under AddressSanitizer and UBSan (test tooling): a stand-alone program
# (tools/splice_junctions_main.cpp) built together with the host sources, run on the committed case of tests/golden/splice_junctions as SAM text, on the same case and on one
# seeded case of tests/splice_junctions_lib.py as raw BAM streams (optional fields of every type, introns past the end of a reference, 601 CIGAR operations), and on those
# streams cut short inside their last records; the tables it writes are compared with the committed one and with the restatement's.
# CPU only: nothing is loaded into python, nothing goes through a GPU.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
WORK=$(mktemp -d /tmp/sanitize_splice_junctions_XXXXXX)
trap 'rm -rf $WORK' EXIT
GOLDEN=$ROOT/tests/golden/splice_junctions
# (python only writes the inputs and the expected tables here)
python3 - $ROOT $WORK <<'PY'
import os, sys
root, work = sys.argv[1], sys.argv[2]
sys.path[:0] = [os.path.join(root, "tests")]
import splice_junctions_lib as lib
annotation = lib.load_annotation()
for name, case in (("hand_made", lib.parse_sam(open(os.path.join(lib.GOLDEN, "hand_made.sam"), "rb").read())), ("seed1600", lib.random_case(1600, annotation)), ("long_cigar", lib.long_cigar_case())):
    open(os.path.join(work, name + ".raw"), "wb").write(lib.bam_header(case[0]) + lib.bam_records(case))
    open(os.path.join(work, name + ".expected"), "wb").write(lib.restate(annotation, case)[0])
PY
g++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$ROOT/include -I$ROOT/arriba_amd/csrc/host -o $WORK/splice_junctions_main $ROOT/tools/splice_junctions_main.cpp $ROOT/arriba_amd/csrc/host/*.cpp -lz
echo "== -fsanitize=address,undefined: hand_made.sam"
ASAN_OPTIONS=detect_leaks=0 $WORK/splice_junctions_main $GOLDEN/hand_made.fa $GOLDEN/hand_made.gtf "j1 j2 j3" $GOLDEN/hand_made.sam $WORK/text.tab
cmp $WORK/text.tab $GOLDEN/hand_made.tab
for RAW in $WORK/*.raw; do
	NAME=$(basename $RAW .raw)
	echo "== -fsanitize=address,undefined: $NAME"
	ASAN_OPTIONS=detect_leaks=0 $WORK/splice_junctions_main $GOLDEN/hand_made.fa $GOLDEN/hand_made.gtf "j1 j2 j3" $RAW $WORK/$NAME.tab
	cmp $WORK/$NAME.tab $WORK/$NAME.expected
	test ! -e $WORK/$NAME.tab.tmp
done
cmp $WORK/hand_made.tab $GOLDEN/hand_made.tab
echo "sanitize_splice_junctions: clean"
