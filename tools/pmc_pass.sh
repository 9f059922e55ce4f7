# GPU: PMC passes over the fused bench (separate --pmc passes; kernel-trace only). Writes OUT_DIR/pmc_*/
# usage: bash tools/pmc_pass.sh [OUT_DIR]
set -e
out=${1:-prof_out}
mkdir -p "$out"
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
i=0
for set in "SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_BUSY_CYCLES" \
           "SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_INSTS_VMEM SQ_INSTS_SMEM SQ_WAVES" \
           "SQC_ICACHE_MISSES SQC_ICACHE_HITS SQ_WAIT_INST_LDS SQ_INST_CYCLES_VMEM" \
           "SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_LDS SQ_ACTIVE_INST_MISC SQ_ACTIVE_INST_SCA"; do
  i=$((i+1))
  timeout -k 10 300 rocprofv3 --kernel-trace --pmc $set -d $out/pmc_$i -o run --output-format csv -- python3 bench.py --steps 5 --warmup 2 --full --no-cpu-baseline > $out/pmc_$i.log 2>&1
done
