#!/bin/bash
# tools/sanitize_realign_split.sh -- the host side of --realign-reads under AddressSanitizer and UBSan (test tooling): a stand-alone program (tools/realign_split_main.cpp) built
# together with the host sources, run on the committed cases of tests/golden/realign_split as SAM text, on the same cases, on one seeded case of either layout and on the record
# with 601 CIGAR operations of tests/realign_split_lib.py as raw BAM streams, and on those streams cut short inside their last records -- name, CIGAR, SEQ and QUAL end mid-record
# there; the files it writes are compared with the committed ones and with the restatement's.
# CPU only: nothing is loaded into python, nothing goes through a GPU.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
WORK=$(mktemp -d /tmp/sanitize_realign_split_XXXXXX)
trap 'rm -rf $WORK' EXIT
GOLDEN=$ROOT/tests/golden/realign_split
# (python only writes the inputs and the expected files here)
python3 - $ROOT $WORK <<'PY'
import os, sys
root, work = sys.argv[1], sys.argv[2]
sys.path[:0] = [os.path.join(root, "tests")]
import realign_split_lib as lib
assembly = lib.load_assembly()
for name, case in (("hand_made", lib.committed_case()), ("hand_made_se", lib.committed_case("hand_made_se")), ("seed1801", lib.random_case(1801)), ("seed1802", lib.random_case(1802)), ("long_cigar", lib.long_cigar_case())):
    open(os.path.join(work, name + ".raw"), "wb").write(lib.bam_header(case["references"]) + lib.bam_records(case))
    realign, kept, _ = lib.restate(assembly, case)
    open(os.path.join(work, name + ".realign.expected"), "wb").write(realign)
    open(os.path.join(work, name + ".kept.expected"), "wb").write(kept)
PY
g++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$ROOT/include -I$ROOT/arriba_amd/csrc/host -o $WORK/realign_split_main $ROOT/tools/realign_split_main.cpp $ROOT/arriba_amd/csrc/host/*.cpp -lz
for NAME in hand_made hand_made_se; do
	echo "== -fsanitize=address,undefined: $NAME.sam"
	ASAN_OPTIONS=detect_leaks=0 $WORK/realign_split_main $GOLDEN/hand_made.fa $GOLDEN/hand_made.gtf "a1 2" $GOLDEN/$NAME.sam $WORK/text.realign.sam $WORK/text.kept.sam
	cmp $WORK/text.realign.sam $GOLDEN/$NAME.realign.sam
	cmp $WORK/text.kept.sam $GOLDEN/$NAME.kept.sam
done
for RAW in $WORK/*.raw; do
	NAME=$(basename $RAW .raw)
	echo "== -fsanitize=address,undefined: $NAME"
	ASAN_OPTIONS=detect_leaks=0 $WORK/realign_split_main $GOLDEN/hand_made.fa $GOLDEN/hand_made.gtf "a1 2" $RAW $WORK/$NAME.realign.sam $WORK/$NAME.kept.sam
	cmp $WORK/$NAME.realign.sam $WORK/$NAME.realign.expected
	cmp $WORK/$NAME.kept.sam $WORK/$NAME.kept.expected
	test ! -e $WORK/$NAME.realign.sam.tmp
	test ! -e $WORK/$NAME.kept.sam.tmp
done
cmp $WORK/hand_made.realign.sam $GOLDEN/hand_made.realign.sam
cmp $WORK/hand_made_se.kept.sam $GOLDEN/hand_made_se.kept.sam
echo "sanitize_realign_split: clean"
