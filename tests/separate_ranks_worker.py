"""TEST-ONLY worker: -c asked of a session that works over the ranks of a job (torch.distributed, gloo; the workflow library over the host stepping harness) -- the refusal of
arriba_workflow_sample_separate, and of a session opened with separate_chimeric_file set, each by its message.
usage: separate_ranks_worker.py fasta gtf out_directory chimeric bam"""
import ctypes
import json
import os
import sys

import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
fasta, gtf, out, chimeric, bam = sys.argv[1:6]
os.environ["ARRIBA_WORKFLOW_LIBRARY"] = os.path.join(ROOT, "tests", "emu", "libworkflow_on_harness.so")
from arriba_amd import _capi  # noqa: E402
_bind = _capi.bind_device_api
_harness = ctypes.CDLL(os.path.join(ROOT, "tests", "emu", "libemu.so"))
_capi.bind_device_api = lambda library, prefix: _bind(_harness, "emu_")
from arriba_amd.pipeline import ArribaError, WorkflowSession  # noqa: E402

dist.init_process_group("gloo")
rank = dist.get_rank()
result = {"rank": rank, "world": dist.get_world_size()}
for key, options in (("sample_separate", {}), ("option", {"separate_chimeric_file": chimeric})):
    try:
        session = WorkflowSession(fasta, gtf, **options)
        session.over_ranks()
        try:
            if key == "sample_separate":
                session.sample_separate(chimeric, bam, os.path.join(out, "never.tsv"))
            else:
                session.sample(bam, os.path.join(out, "never.tsv"))
            result[key] = "accepted"
        except ArribaError as error:
            result[key] = str(error)
        session.close()
    except Exception as error:  # noqa: BLE001 (the test reads the report)
        result[key] = repr(error)
json.dump(result, open(os.path.join(out, "rank%d.json" % rank), "w"))
dist.barrier()
dist.destroy_process_group()
