#!/bin/bash
# Builds tools/separate_chimeric_main.cpp with the host sources under AddressSanitizer + UndefinedBehaviorSanitizer (linked in; nothing is preloaded, no Python runs) and runs it
# on the toy dataset split by tools/split_chimeric.py.  CPU only.      tools/sanitize_separate_chimeric.sh [scratch directory]
set -euo pipefail
root="$(cd "$(dirname "$0")/.." && pwd)"
scratch="${1:-$(mktemp -d)}"
mkdir -p "$scratch"
g++ -std=c++17 -O1 -g -fno-omit-frame-pointer -fsanitize=address,undefined -fno-sanitize-recover=undefined -pthread -Wno-parentheses \
    -o "$scratch/separate_chimeric_main" "$root/tools/separate_chimeric_main.cpp" "$root"/arriba_amd/csrc/host/*.cpp -lz
"$root/arriba_amd/lib/gen_synth" --out "$scratch/data" --seed 11 --fragments 600 --contigs 4 --contig-len 300000 --junctions 60 > /dev/null 2>&1
python3 "$root/tools/split_chimeric.py" "$scratch/data.bam" "$scratch/C.bgzf.bam" "$scratch/R.bgzf.bam" --variant full
python3 -c "import sys; sys.path.insert(0, '$root/tools'); from bam_to_sam import inflate_all; [open('$scratch/' + name + '.bam', 'wb').write(inflate_all(open('$scratch/' + name + '.bgzf.bam', 'rb').read())) for name in ('C', 'R')]"
ASAN_OPTIONS=detect_leaks=1 "$scratch/separate_chimeric_main" "$scratch/data.fa" "$scratch/data.gtf" "$scratch/C.bam" "$scratch/R.bam" "$scratch"
echo "sanitize_separate_chimeric: nothing reported"
