#!/bin/bash
# tools/sanitize_markdup.sh -- the host side of --mark-duplicates under AddressSanitizer and UBSan (test tooling): a stand-alone program (tools/markdup_main.cpp) built together with
# the host sources, run on the committed case of tests/golden/mark_duplicates (clips on both strands, u < 0, qualities of `*`, records without a reference, secondary and
# supplementary records) and on streams cut short inside their last records; the marks it writes are compared with the committed ones.
# CPU only: nothing is loaded into python, nothing goes through a GPU.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
WORK=$(mktemp -d /tmp/sanitize_markdup_XXXXXX)
trap 'rm -rf $WORK' EXIT
# (python only writes the inputs here: the uncompressed streams)
python3 - $ROOT $WORK <<'PY'
import glob, os, sys
root, work = sys.argv[1], sys.argv[2]
sys.path[:0] = [os.path.join(root, "tests")]
import markdup_lib as lib
for path in sorted(glob.glob(os.path.join(root, "tests", "golden", "mark_duplicates", "*.sam"))):
    case = lib.parse_sam(open(path, "rb").read())
    open(os.path.join(work, os.path.basename(path)[:-4] + ".raw"), "wb").write(lib.bam_header(case[0]) + lib.bam_records(case))
PY
g++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$ROOT/include -I$ROOT/arriba_amd/csrc/host -o $WORK/markdup_main $ROOT/tools/markdup_main.cpp $ROOT/arriba_amd/csrc/host/*.cpp -lz
for RAW in $WORK/*.raw; do
	NAME=$(basename $RAW .raw)
	echo "== -fsanitize=address,undefined: $NAME"
	ASAN_OPTIONS=detect_leaks=0 $WORK/markdup_main $RAW $WORK/$NAME.marks
	cmp $WORK/$NAME.marks $ROOT/tests/golden/mark_duplicates/$NAME.expected
done
echo "sanitize_markdup: clean"
