#!/bin/bash
# tools/sanitize_virus.sh -- the host side of --virus-expression under AddressSanitizer and UBSan (test tooling): a stand-alone program (tools/virus_main.cpp) built together
# with the host sources, run on every committed case of tests/golden/virus_expression (the hand-made file: reads of 11 to 13 bases, `*` sequences, odd lengths, the first and the
# last base of a contig, word boundaries of the bitmap) and on streams cut short inside their last records; the tables it writes are compared with the committed ones.
# CPU only: nothing is loaded into python, nothing goes through a GPU.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
WORK=$(mktemp -d /tmp/sanitize_virus_XXXXXX)
trap 'rm -rf $WORK' EXIT
# (python only writes the inputs here: the uncompressed streams)
python3 - $ROOT $WORK <<'PY'
import glob, os, sys
root, work = sys.argv[1], sys.argv[2]
sys.path[:0] = [os.path.join(root, "tests")]
import virus_expression_lib as lib
for path in sorted(glob.glob(os.path.join(root, "tests", "golden", "virus_expression", "*.sam"))):
    case = lib.parse_sam(open(path, "rb").read())
    open(os.path.join(work, os.path.basename(path)[:-4] + ".raw"), "wb").write(lib.bam_header(case[0]) + lib.bam_records(case))
PY
g++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$ROOT/include -I$ROOT/arriba_amd/csrc/host -o $WORK/virus_main $ROOT/tools/virus_main.cpp $ROOT/arriba_amd/csrc/host/*.cpp -lz
for RAW in $WORK/*.raw; do
	NAME=$(basename $RAW .raw)
	echo "== -fsanitize=address,undefined: $NAME"
	ASAN_OPTIONS=detect_leaks=0 $WORK/virus_main $RAW $WORK/$NAME.tsv
	cmp $WORK/$NAME.tsv $ROOT/tests/golden/virus_expression/$NAME.tsv
	test ! -e $WORK/$NAME.tsv.tmp
done
echo "sanitize_virus: clean"
