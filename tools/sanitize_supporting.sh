#!/bin/bash
# tools/sanitize_supporting.sh -- the host side of --supporting-alignments under AddressSanitizer and UBSan (test tooling): a stand-alone program (tools/supporting_main.cpp) built
# together with the host sources, run on the hand-made records of tests/test_supporting_alignments.py (window boundaries, the clamp, twins, an empty file, a read over three
# blocks, a file that ends on a block boundary, a last block of 40 bytes; once more with ARRIBA_SUPPORT_HASH_BITS=4) and on the dataset toy3k with the rows of its golden
# fusions.tsv; the files it writes are read back by tools/read_bam.py.  CPU only: nothing is loaded into python, nothing goes through a GPU.
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
WORK=$(mktemp -d /tmp/sanitize_supporting_XXXXXX)
trap 'rm -rf $WORK' EXIT
$ROOT/arriba_amd/lib/gen_synth --out $WORK/toy3k --seed 11 --fragments 3000 --contigs 4 --contig-len 300000 --junctions 60 > /dev/null 2>&1
# (python only writes the inputs here: the uncompressed streams, and the names and rows as text)
python3 - $ROOT $WORK <<'PY'
import gzip, os, sys
root, work = sys.argv[1], sys.argv[2]
sys.path[:0] = [os.path.join(root, "tests"), os.path.join(root, "tools")]
import test_supporting_alignments as t
stream = gzip.open(os.path.join(work, "toy3k.bam"), "rb").read()
header, record_bytes = t._split(stream)
text = gzip.open(os.path.join(root, "tests", "golden", "toy3k", "fusions.tsv.gz"), "rt").read()
for name, case in (("hand_made", t._hand_made(header)), ("toy3k", t.Case(header, record_bytes, t._rows_of_fusions(text, t._references_of(header))))):
    open(os.path.join(work, name + ".raw"), "wb").write(case.header + case.record_bytes)
    with open(os.path.join(work, name + ".rows"), "wb") as out:
        for entry in case.names:
            out.write(b"N " + entry + b"\n")
        for row, (_, breakpoints) in enumerate(case.rows):
            fields = [str(value) for ref, position in breakpoints for value in (ref, position - 1)] + [str(entry) for entry in case.entries[case.name_begin[row]:case.name_begin[row + 1]]]
            out.write(("R " + " ".join(fields) + "\n").encode())
PY
g++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -I$ROOT/include -I$ROOT/arriba_amd/csrc/host -o $WORK/supporting_main $ROOT/tools/supporting_main.cpp $ROOT/arriba_amd/csrc/host/*.cpp -lz
for RUN in "hand_made 1000 64" "hand_made 1000 4" "toy3k 1000000 64" "toy3k 2000 64"; do
	set -- $RUN
	echo "== -fsanitize=address,undefined: $1, window $2, $3 bits of the hash"
	mkdir -p $WORK/out_$1_$2_$3
	ARRIBA_SUPPORT_HASH_BITS=$3 ASAN_OPTIONS=detect_leaks=0 $WORK/supporting_main $WORK/$1.raw $WORK/$1.rows $2 $WORK/out_$1_$2_$3/support
	for FILE in $WORK/out_$1_$2_$3/support_*.bam; do python3 $ROOT/tools/read_bam.py $FILE > /dev/null; test -s $FILE.bai; done
	test -z "$(ls $WORK/out_$1_$2_$3 | grep -v '^support_[0-9]*\.bam\(\.bai\)\?$')"
done
cmp $WORK/out_hand_made_1000_64/support_1.bam $WORK/out_hand_made_1000_4/support_1.bam
echo "sanitize_supporting: clean"
