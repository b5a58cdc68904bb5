#!/bin/bash
# PMC comparison of the plain search kernel and the kernel that also reduces (bench.py --reduce fused), one box.
set -o pipefail
R=${GRAFT_REPO_ROOT:-/root/repo}; O=$R/gpurun_out/pmc_fused; mkdir -p $O; cd /tmp; export TMPDIR=/tmp
for mode in separate fused; do
  for set in "SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_INSTS_VALU SQ_ACTIVE_INST_VALU" "SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_SALU" "GRBM_GUI_ACTIVE SQ_WAVES SQ_INSTS_VMEM_RD SQ_INSTS_SMEM"; do
    tag=$(echo $set | cut -d" " -f1)
    timeout -k 10 200 rocprofv3 --pmc $set --kernel-trace --output-format csv -d $O/${mode}_$tag -- python3 $R/bench.py --full --reduce $mode --steps 30 --settle-steps 100 --cpu-seconds 0 > $O/${mode}_$tag.log 2>&1 || { echo "$mode $tag failed"; tail -3 $O/${mode}_$tag.log; }
  done
done
python3 - <<'PY'
import csv, glob, collections, os
O=os.environ.get("GRAFT_REPO_ROOT","/root/repo")+"/gpurun_out/pmc_fused"
for mode in ("separate","fused"):
    acc=collections.defaultdict(lambda: collections.defaultdict(list))
    for f in glob.glob(f"{O}/{mode}_*/*/*_counter_collection.csv"):
        for r in csv.DictReader(open(f)):
            k=r["Kernel_Name"]
            if "lane8" not in k or "pruned" in k: continue
            k=k.split("(anonymous namespace)::")[-1].split("(")[0]
            acc[k][r["Counter_Name"]].append(float(r["Counter_Value"]))
    for k in acc:
        print(mode, k)
        for c in sorted(acc[k]):
            v=acc[k][c]; print(f"    {c:<22} n={len(v):<4} mean={sum(v)/len(v):.6g}")
PY
