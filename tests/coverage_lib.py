"""What tests/test_coverage_track.py shares with tools/: a restatement of the rule of --coverage in plain Python and numpy -- a depth array per contig, every
record added in a loop, the result run-length encoded --, and the cases that are made at test time.  The restatement is written from the rule, not from depth_core.hpp; it is the
independent side for inputs made at test time only because it gives tests/golden/coverage/hand_made.bedgraph, which a reader can check by eye, from hand_made.sam.

A case is (references, records) as in tests/virus_expression_lib.py, whose SAM reader and BAM writers are used: references a list of (name, LN); records a list of
(qname, flag, rname or "*", 1-based pos, cigar text or "*", seq text or "*")."""
import random
import re

import numpy as np

COVERS, ADVANCES = "M=XD", "N"  # I, S, H and P neither advance nor cover


def restate(case):
    """-> (bedGraph text, {"records", "runs", "covered_positions", "aligned_bases", "max_depth", "text_bytes"})"""
    references, records = case
    depth = [np.zeros(length, np.int64) for _, length in references]
    index_of = {name: k for k, (name, _) in enumerate(references)}
    counted = 0
    for qname, flag, rname, pos, cigar, seq in records:
        if flag & 4 or rname == "*" or cigar == "*":
            continue
        counted += 1
        contig, at = depth[index_of[rname]], pos - 1
        for length, op in re.findall(r"(\d+)([MIDNSHP=X])", cigar):
            length = int(length)
            if op in COVERS:
                contig[max(at, 0):max(min(at + length, len(contig)), 0)] += 1
            if op in COVERS or op in ADVANCES:
                at += length
    lines, covered, aligned, deepest = [], 0, 0, 0
    for (name, _), contig in zip(references, depth):
        if len(contig) == 0:
            continue
        edges = np.concatenate(([0], np.flatnonzero(np.diff(contig)) + 1, [len(contig)]))
        for start, end in zip(edges[:-1], edges[1:]):
            value = int(contig[start])
            if value > 0:
                lines.append("%s\t%d\t%d\t%d\n" % (name, start, end, value))
                covered += int(end - start); aligned += int(end - start) * value; deepest = max(deepest, value)
    text = "".join(lines).encode()
    return text, {"records": counted, "runs": len(lines), "covered_positions": covered, "aligned_bases": aligned, "max_depth": deepest, "text_bytes": len(text)}


def random_case(seed, n_records=150):
    """three to six contigs (one of at least 2000 bases, so that a window of 997 positions is not the only one), records that pile up around a few anchors, abut, run past the end of
    their contig, are split by N, carry every operation; some are unmapped, without a reference or without a CIGAR"""
    generator = random.Random(seed)
    references = [("scaffold_%d_%d" % (seed, k), generator.randint(2000, 5000) if k == 0 else generator.randint(50, 5000)) for k in range(generator.randint(3, 6))]
    anchors = [(generator.randrange(len(references)), generator.randint(1, 40) * 10) for _ in range(12)]
    records = []
    for r in range(n_records):
        t, anchor = generator.choice(anchors)
        name, length = references[t]
        choice = generator.random()
        if choice < 0.5:
            pos = min(anchor, length) + generator.choice((0, 0, 10, 20, 25, 1))
        elif choice < 0.8:
            pos = generator.randint(1, length)
        else:
            pos = max(1, length - generator.randint(-5, 30))  # around the end of the contig, also behind it
        ops = []
        if generator.random() < 0.3:
            ops.append("%dS" % generator.randint(1, 9))
        for piece in range(generator.randint(1, 4)):
            if piece:
                ops.append("%d%s" % (generator.randint(1, 60), generator.choice("NNNDIP")))
            ops.append("%d%s" % (generator.choice((5, 10, 10, 20, 25, generator.randint(1, 70))), generator.choice("MMMMM=X")))
        if generator.random() < 0.3:
            ops.append("%dH" % generator.randint(1, 9))
        flag = generator.choice((0, 16, 99, 147, 83, 163, 256, 272, 2048, 1024, 512, 4, 77))
        rname, cigar = name, "".join(ops)
        special = generator.random()
        if special < 0.04:
            rname, flag = "*", generator.choice((73, 77, 4))  # (73: paired, the mate unmapped, bit 0x4 clear -- the ingest refuses any other record without a reference that claims to be mapped)
        elif special < 0.08:
            cigar = "*"
        records.append(("r%d" % r, flag, rname, pos if rname != "*" else 0, cigar, "*"))
    return references, records


def hot_case():
    """70 000 identical 64M records at one position and one record shifted by one base: a depth above 2^16, every mark on two addresses (three for the shifted record's)"""
    references = [("hot1", 3000), ("hot2", 500)]
    bases = "ACGT" * 16
    return references, [("h%05d" % k, 0, "hot1", 1001, "64M", bases) for k in range(70000)] + [("shifted", 16, "hot1", 1002, "64M", bases)]


def empty_case():
    """no record that counts"""
    return [("e1", 4000), ("e2", 90)], [("u1", 4, "e1", 10, "20M", "*"), ("u2", 77, "*", 0, "*", "*"), ("u3", 0, "e2", 5, "*", "*"), ("u4", 73, "*", 0, "10M", "*")]
