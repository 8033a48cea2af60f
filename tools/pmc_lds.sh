#!/bin/bash
# usage (GPU box, from the repo root): tools/pmc_lds.sh <outdir> <name> <bench args...>
# The LDS-conflict PMC pass of one bench configuration: how the LDS ARRAY serves the kernel's reads (bank conflicts, address
# conflicts, array cycles), beside the instruction counters the other passes collect.  A `rocprofv3 --pmc` run of its own:
# counters only, no tracing of any kind in the same run.  Six SQ counters fit the eight SQ slots of one pass.
# tools/lds_conflict_summary.py turns pmc_lds_counter_collection.csv into lds_conflict.json (conflict cycles per LDS instruction and
# as a share of SQ_LDS_IDX_ACTIVE).
set -e
R=$(pwd)
OUT=$R/$1; name=$2; shift; shift
mkdir -p $OUT/$name
cd /tmp && export TMPDIR=/tmp
COMMON="--no-cpu-baseline --no-extras --no-spin"   # no clock warm-up launches under the profiler: they are the same kernel with fewer steps
CTR="SQ_LDS_BANK_CONFLICT SQ_LDS_ADDR_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_LDS SQ_ACTIVE_INST_LDS"
# SQ_LDS_UNALIGNED_STALL where the counter list of this ROCm has it for the device
if rocprofv3 -L 2>/dev/null | grep -q SQ_LDS_UNALIGNED_STALL; then CTR="$CTR SQ_LDS_UNALIGNED_STALL"; fi
rocprofv3 --pmc $CTR --output-format csv -d $OUT/$name -o pmc_lds -- python3 $R/bench.py $COMMON "$@" > $OUT/$name/pmc_lds.json 2> $OUT/$name/pmc_lds.err
echo done lds $name
