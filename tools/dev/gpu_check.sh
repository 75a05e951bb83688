out=${PROFILE_OUT:-profile_out}; mkdir -p $out
timeout -k 10 600 python -m pytest tests -m gpu -x -q > $out/t.log 2>&1; tail -2 $out/t.log; python bench.py --full --steps 200 --warmup 20 2>/dev/null > $out/b.json && python bench.py --full --workload community_small_CC --steps 100 --warmup 10 2>/dev/null > $out/b_cs.json; python - <<EOF
import json
for f in ("$out/b.json","$out/b_cs.json"):
    try:
        j=json.loads(open(f).read().strip().splitlines()[-1]); print(f, j["value"], j["ms_per_step"], j["roofline"]["kernel"], j["roofline"]["avg_launch_us"], j.get("roofline_k_xa",{}).get("avg_launch_us"))
    except Exception as e: print(f, "ERR", e)
EOF
