"""Per-launch LDS-conflict figures of the dominant kernel from the output of tools/pmc_lds.sh.

  python tools/lds_conflict_summary.py <outdir>/<name> [...]  > profiles/<round>/lds_conflict.json

Reads pmc_lds_counter_collection.csv of every directory given (wherever rocprofv3 put it below the directory) and prints, per
directory, the counters averaged over the full K-step launches of the kernel with the most dispatches whose name holds $KERNEL (default k_rollout), conflict cycles per LDS
instruction and conflict cycles as a share of SQ_LDS_IDX_ACTIVE."""
import csv
import glob
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_pmc_traffic import dominant, lds_conflict  # noqa: E402

out = {}
for d in sys.argv[1:]:
    rows = []
    for f in glob.glob(os.path.join(d, "**", "pmc_lds*counter_collection.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    k, vals = dominant(rows, os.environ.get("KERNEL", "k_rollout"))
    ent = {"kernel": k, "SQ_INSTS_LDS": vals.get("SQ_INSTS_LDS"), "SQ_ACTIVE_INST_LDS": vals.get("SQ_ACTIVE_INST_LDS")}
    ent.update(lds_conflict(vals))
    out[d] = ent
print(json.dumps(out, indent=1))
