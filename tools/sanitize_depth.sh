#!/bin/bash
# tools/sanitize_depth.sh -- the host side of --coverage under AddressSanitizer and UBSan (test tooling): a stand-alone program (tools/depth_main.cpp) built together with the
# host sources, run on the committed case of tests/golden/coverage (records at position 0, at and past the end of a contig, every CIGAR operation, records that do not count) and
# on streams cut short inside their last records; the track it writes is compared with the committed one.
# CPU only: nothing is loaded into python, nothing goes through a GPU.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
WORK=$(mktemp -d /tmp/sanitize_depth_XXXXXX)
trap 'rm -rf $WORK' EXIT
# (python only writes the inputs here: the uncompressed streams)
python3 - $ROOT $WORK <<'PY'
import glob, os, sys
root, work = sys.argv[1], sys.argv[2]
sys.path[:0] = [os.path.join(root, "tests")]
import virus_expression_lib as lib
for path in sorted(glob.glob(os.path.join(root, "tests", "golden", "coverage", "*.sam"))):
    case = lib.parse_sam(open(path, "rb").read())
    open(os.path.join(work, os.path.basename(path)[:-4] + ".raw"), "wb").write(lib.bam_header(case[0]) + lib.bam_records(case))
PY
g++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$ROOT/include -I$ROOT/arriba_amd/csrc/host -o $WORK/depth_main $ROOT/tools/depth_main.cpp $ROOT/arriba_amd/csrc/host/*.cpp -lz
for RAW in $WORK/*.raw; do
	NAME=$(basename $RAW .raw)
	echo "== -fsanitize=address,undefined: $NAME"
	ASAN_OPTIONS=detect_leaks=0 $WORK/depth_main $RAW $WORK/$NAME.bedgraph
	cmp $WORK/$NAME.bedgraph $ROOT/tests/golden/coverage/$NAME.bedgraph
	test ! -e $WORK/$NAME.bedgraph.tmp
done
echo "sanitize_depth: clean"
