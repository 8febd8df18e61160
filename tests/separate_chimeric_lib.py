"""Shared by the tests of -c (tests/test_separate_chimeric.py) and tools/make_separate_golden.py: the inputs (tools/split_chimeric.py over a generated WithinBAM file), the live
reference (`arriba_ref -c C -x R`, where the oracle build is there), the committed goldens (tests/golden/separate_<dataset>/: its log and its two files)."""
import gzip
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import split_chimeric  # noqa: E402

import datasets  # noqa: E402

ARRIBA_REF = os.path.join(ROOT, "oracle", "_ref", "arriba_ref")
WORKFLOW = os.path.join(ROOT, "arriba_amd", "lib", "arriba_gpu_workflow")
DATASETS = ("toy3k", "shuffled2k", "itd6k")
NO_BLACKLIST = ["-f", "blacklist"]


def golden_directory(name):
    return os.path.join(ROOT, "tests", "golden", "separate_" + name)


def split_files(prefix, variant="clean", keep_multimappers=False, tag=None):
    """writes PREFIX.TAG.C.bam and PREFIX.TAG.R.bam; returns their paths"""
    tag = tag or (variant + ("_mm" if keep_multimappers else ""))
    chimeric, main, moved = split_chimeric.split(open(prefix + ".bam", "rb").read(), variant, keep_multimappers)
    paths = (prefix + "." + tag + ".C.bam", prefix + "." + tag + ".R.bam")
    for path, data in zip(paths, (chimeric, main)):
        with open(path, "wb") as out:
            out.write(data)
    assert moved > 0
    return paths


def strip_times(log):
    return re.sub(r"\[\d{4}-\d\d-\d\dT\d\d:\d\d:\d\d\] ", "", log)


def reference_available():
    return os.path.exists(ARRIBA_REF)


def run_reference(prefix, chimeric, main, outputs, extra=()):
    """`arriba_ref -c chimeric -x main`; returns its log (stdout + stderr, the time stamps taken out).  Run from the directory of the files, with relative names."""
    directory = os.path.dirname(prefix)
    relative = lambda path: os.path.relpath(path, directory)
    command = [ARRIBA_REF, "-c", relative(chimeric), "-x", relative(main), "-g", relative(prefix + ".gtf"), "-a", relative(prefix + ".fa"), "-o", relative(outputs[0]), "-O", relative(outputs[1])] + NO_BLACKLIST + list(extra)
    result = subprocess.run(command, cwd=directory, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert result.returncode == 0, result.stdout
    return strip_times(result.stdout), command


def totals_of(log):
    """([total of the first call, total of the second], [malformed count of the first, of the second]) from the lines "Reading chimeric alignments from ... (total=N)": the
    reference prints such a line in two halves, so the WARNING lines of a call stand between "(total=" and the number"""
    totals, malformed = [], []
    for warnings, total in re.findall(r"Reading chimeric alignments from '[^']*' \(total=((?:WARNING:[^\n]*\n)*)(\d+)\)", log):
        totals.append(int(total))
        count = re.search(r"WARNING: (\d+) SAM records were malformed and ignored", warnings)
        malformed.append(int(count.group(1)) if count else 0)
    return totals, malformed


def remaining_of(log):
    """every (remaining=N) of a log, in order"""
    return re.findall(r"\(remaining=(\d+)\)", log)


def read_golden(name, file_name):
    path = os.path.join(golden_directory(name), file_name)
    return gzip.open(path + ".gz", "rt").read() if os.path.exists(path + ".gz") else open(path).read()


def bgzf_deflated(stream):
    """the bytes as a BGZF file of deflated blocks with the end-of-file marker (SAMv1 section 4.1)"""
    import struct
    import zlib
    out = []
    for begin in range(0, len(stream), 0xFF00):
        payload = bytes(stream[begin:begin + 0xFF00])
        deflater = zlib.compressobj(6, zlib.DEFLATED, -15)
        deflated = deflater.compress(payload) + deflater.flush()
        out.append(b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", len(deflated) + 25) + deflated + struct.pack("<II", zlib.crc32(payload), len(payload)))
    out.append(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    return b"".join(out)


def workflow_command(prefix, chimeric, main, outputs, extra=()):
    return [WORKFLOW, "-c", chimeric, "-x", main, "-g", prefix + ".gtf", "-a", prefix + ".fa", "-o", outputs[0], "-O", outputs[1]] + NO_BLACKLIST + list(extra)
