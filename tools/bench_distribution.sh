#!/bin/bash
# The default bench and the 9 375-chain shard, N runs on the box this is started on (start it once per box to sample boxes):
#   tools/bench_distribution.sh N OUTFILE
N=${1:-8}; OUT=${2:-profiles/r06/bench_distribution.txt}
cd "$(dirname "$0")/.."
D=$(mktemp -d)
{
echo "# python bench.py --full --no-cpu-baseline, the same with --regions 75 --eps 125 and plain python bench.py --regions 75 --eps 125 --spinup-ms 0, $N runs:"
echo "# ms per pass, stages, this box's 8 B/lane copy bandwidth, the placement report of the headline run (staged ms of the allocations tried, mode),"
echo "# and what 8 GPUs would make of the fixed sweep on boxes like this one (headline pass / shard pass)"
for i in $(seq $N); do
  timeout -k 10 600 python bench.py --full --no-cpu-baseline > $D/h_$i.json 2>/dev/null && timeout -k 10 300 python bench.py --full --no-cpu-baseline --regions 75 --eps 125 > $D/s_$i.json 2>/dev/null && timeout -k 10 300 python bench.py --regions 75 --eps 125 --spinup-ms 0 > $D/n_$i.json 2>/dev/null || break
  python3 - $D $i <<'PY'
import json, sys
d, i = sys.argv[1], sys.argv[2]
try:
    h = json.loads(open(f"{d}/h_{i}.json").read().strip().splitlines()[-1])
    s = json.loads(open(f"{d}/s_{i}.json").read().strip().splitlines()[-1])
except Exception as e:
    print(f"run {i}: no result ({e})"); sys.exit(0)
hk, sk, pl = h["kernels"], s["kernels"], h["config"].get("placement") or {}
try:
    n = json.loads(open(f"{d}/n_{i}.json").read().strip().splitlines()[-1])["ms_per_step"]
except Exception:
    n = float("nan")
print("run %s  headline %6.2f ms (fwd %.2f pinv %.2f bwd %.2f)  copy %.2f TB/s  tries %s mode %s   shard %5.2f ms (fwd %.2f pinv %.2f bwd %.2f; %.2f without the spin-up)   ratio %.2f" % (
    i, h["ms_per_step"], hk["ekf_fwd_ms"], hk["eks_pinv_ms"], hk["eks_bwd_ms"], h["roofline"]["measured_copy"]["copy_8B_per_lane_GBs"] / 1e3,
    pl.get("tries"), pl.get("mode"), s["ms_per_step"], sk["ekf_fwd_ms"], sk["eks_pinv_ms"], sk["eks_bwd_ms"], n, h["ms_per_step"] / s["ms_per_step"]))
PY
done
} > $OUT 2>&1
rm -rf $D
cat $OUT
