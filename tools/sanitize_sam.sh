#!/bin/bash
# tools/sanitize_sam.sh -- the SAM text transcoder (arriba_amd/csrc/device/sam_core.hpp stepped on the host) under AddressSanitizer/UBSan, as tools/sanitize_host.sh does it
# for the ingest: the malformed texts of tests/test_sam_input.py, every line parsed from a heap copy of exactly its size (ARRIBA_SAM_ISOLATE_LINES=1), so that a read outside
# a line is reported.  Each file must come back with status -1 and the line number its name begins with; then the text of a whole dataset (no malformed line).
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
WORK=$(mktemp -d /tmp/sanitize_sam_XXXXXX)
g++ -std=c++17 -O1 -g -pthread -fsanitize=address,undefined -fno-omit-frame-pointer -I$ROOT/include -I$ROOT/arriba_amd/csrc/host -o $WORK/sam_transcode $ROOT/tools/sam_transcode_main.cpp $ROOT/arriba_amd/csrc/host/*.cpp -lz
python3 -c "import sys; sys.path[:0] = ['$ROOT/tests', '$ROOT/tools']; import test_sam_input; test_sam_input.write_malformed_cases('$WORK')"
FAILED=0
for FILE in $WORK/*.sam; do
	EXPECTED=$(basename $FILE | cut -d_ -f1)
	RESULT=$(ARRIBA_SAM_ISOLATE_LINES=1 ASAN_OPTIONS=detect_leaks=0 $WORK/sam_transcode $FILE 2>&1) || { echo "$RESULT"; FAILED=1; continue; }
	set -- $RESULT
	if [ "$2" != "-1" ] || [ "$3" != "$EXPECTED" ]; then echo "UNEXPECTED: $RESULT (expected line $EXPECTED)"; FAILED=1; fi
done
$ROOT/arriba_amd/lib/gen_synth --out $WORK/data --seed 17 --fragments 3000 --contigs 3 --contig-len 200000 --junctions 50 > /dev/null 2>&1
python3 $ROOT/tools/bam_to_sam.py $WORK/data.bam > $WORK/data.sam
RESULT=$(ARRIBA_SAM_ISOLATE_LINES=1 ASAN_OPTIONS=detect_leaks=0 $WORK/sam_transcode $WORK/data.sam 2>&1) || { echo "$RESULT"; FAILED=1; }
echo "$RESULT" | sed "s|$WORK/||"
set -- $RESULT
if [ "$2" != "0" ]; then FAILED=1; fi
rm -rf $WORK
if [ $FAILED = 0 ]; then echo "sanitize_sam: all malformed texts told with their line, no report from the sanitizers"; else echo "sanitize_sam: FAILED"; exit 1; fi
