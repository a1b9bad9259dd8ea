#!/bin/bash
# one gpurun call: launch-size table (default and MKHE_NTT32=0), the prefetch variant, then the headline / secondary bench lines
O=${1:-runs/ab}       # bash tools/quick_ab.sh [output directory, default runs/ab]
mkdir -p "$O"
( echo "== default"; python3 tools/ntt16_bench.py 1500 | grep -E "limbs" | cut -c1-150
  echo "== MKHE_NTT32=0"; MKHE_NTT32=0 python3 tools/ntt16_bench.py 1500 | grep -E "limbs" | cut -c1-150 ) > $O/sizes.txt 2>&1
REPS=1500 bash tools/run_variants.sh pf shipped > $O/variants.txt 2>&1
python3 bench.py --full > $O/bench_plain.json 2> $O/bench_plain.err
MKHE_NTT32=0 python3 bench.py --full --no-cpu > $O/bench_h16.json 2> $O/bench_h16.err
python3 bench.py --full --params PN14QP439 --no-cpu --no-extras --steps 50 --warmup 5 > $O/bench_pn14.json 2>/dev/null
python3 bench.py --full --params PN16QP1761 --parties 8 --steps 10 --warmup 2 --no-cpu > $O/bench_pn16.json 2>/dev/null
python3 bench.py --full --scheme bfv --no-cpu > $O/bench_bfv.json 2>/dev/null
python3 bench.py --full --scheme cnn --parties 4 --no-cpu --steps 20 --warmup 3 > $O/bench_cnn4.json 2>/dev/null
python3 bench.py --full --scheme cnn --parties 4 --batch 8 --no-cpu --steps 20 --warmup 3 > $O/bench_cnn4_b8.json 2>/dev/null
cat $O/sizes.txt $O/variants.txt
python3 - "$O" <<'PY'
import json, glob, sys
for f in sorted(glob.glob(sys.argv[1] + "/bench_*.json")):
    try:
        d = json.loads(open(f).read().strip().splitlines()[-1])
    except Exception as e:
        print(f, "ERR", e); continue
    r = d.get("roofline") or {}
    print(f.split("/")[-1], round(d["value"], 1), d["unit"], "ms/step", round(d["ms_per_step"], 4), "frac", r.get("frac"), (r.get("kernel") or "")[:28], "avg_us", r.get("avg_launch_us"))
PY
