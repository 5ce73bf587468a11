#!/bin/bash
# tools/pmc_k.sh OUTDIR -- one rocprofv3 PMC pass per depth-lane count K over one bench frame (run
# on the GPU host, from anywhere; OUTDIR as tools/pmc.sh takes it, relative to the repository root)
OUT=$1
export TMPDIR=/tmp; cd "$(dirname "$0")/.." && mkdir -p "$OUT" || exit 1
for K in ${KS:-2 4 8}; do
  VR_DEPTH_LANES=$K timeout -k 10 240 rocprofv3 --pmc SQ_WAVES SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_SALU SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_WAIT_INST_ANY SQ_INSTS_VMEM_RD \
    -d "$OUT/k$K" -o pmc --output-format csv -- python bench.py --full --steps 1 --warmup 0 --no-cpu-baseline \
    > "$OUT/k$K.log" 2>&1 || exit 1
done
