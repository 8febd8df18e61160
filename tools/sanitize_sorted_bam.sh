#!/bin/bash
# tools/sanitize_sorted_bam.sh -- the host side of --sorted-bam under AddressSanitizer and UBSan (test tooling): a stand-alone program (tools/sorted_bam_main.cpp) built together
# with the host sources, run on the hand-made file of tests/test_sorted_bam.py (records without a coordinate, a read of 70 000 bases over three blocks, a record that ends on a
# block boundary, a last block of 40 bytes) and on the dataset toy3k; the two files it writes are read back by tools/read_bam.py.  CPU only: nothing is loaded into python,
# nothing goes through a GPU.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
WORK=$(mktemp -d /tmp/sanitize_sorted_bam_XXXXXX)
trap 'rm -rf $WORK' EXIT
$ROOT/arriba_amd/lib/gen_synth --out $WORK/toy3k --seed 11 --fragments 3000 --contigs 4 --contig-len 300000 --junctions 60 > /dev/null 2>&1
# (python only writes the input here: the hand-made records of the test module on the references of toy3k, as a BGZF file of stored blocks)
python3 - $ROOT $WORK <<'PY'
import gzip, os, sys
root, work = sys.argv[1], sys.argv[2]
sys.path[:0] = [os.path.join(root, "tests"), os.path.join(root, "tools")]
import test_sorted_bam as t
header, _ = t._split(gzip.open(os.path.join(work, "toy3k.bam"), "rb").read())
t._write_bgzf(os.path.join(work, "hand_made.bam"), header + b"".join(t._hand_made(t._references_of(header))), 0)
PY
g++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$ROOT/include -I$ROOT/arriba_amd/csrc/host -o $WORK/sorted_bam_main $ROOT/tools/sorted_bam_main.cpp $ROOT/arriba_amd/csrc/host/*.cpp -lz
for NAME in hand_made toy3k; do
	echo "== -fsanitize=address,undefined: $NAME"
	ASAN_OPTIONS=detect_leaks=0 $WORK/sorted_bam_main $WORK/$NAME.bam $WORK/$NAME.sorted.bam
	python3 $ROOT/tools/read_bam.py $WORK/$NAME.sorted.bam
	test -s $WORK/$NAME.sorted.bam.bai
done
echo "sanitize_sorted_bam: clean"
