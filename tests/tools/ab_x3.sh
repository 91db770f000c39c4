#!/bin/bash
# same-box A/B of the fp32 step: native fp32 MFMA kernels against the fp32x3 mode (six bf16 products per block)
STEPS=${STEPS:-30}
O=$(mktemp -d)                    # per-arm lines; the table below is the result
for tag in x3 f32 x3_noside x3b f32b; do
  case $tag in
    x3|x3b) extra="--precision fp32x3";;
    f32|f32b) extra="";;
    x3_noside) extra="--precision fp32x3 --no_side_stream";;
  esac
  python bench.py --full --steps $STEPS --warmup 10 --no_cpu_baseline $extra > $O/ab_$tag.json 2> $O/ab_$tag.err || tail -5 $O/ab_$tag.err
done
O=$O python - <<'EOF2'
import json, os
for f in ("x3", "f32", "x3_noside", "x3b", "f32b"):
    try:
        d = json.load(open(os.path.join(os.environ["O"], "ab_%s.json" % f)))
        print(f, d["value"], d["ms_per_step"], d["final_loss"])
        for fam in d.get("roofline_families", []):
            print("   ", fam["family"], fam["launches_per_step"], fam["avg_us"], fam["ms_per_step"], fam["achieved"])
    except Exception as e:
        print(f, "ERR", e)
EOF2
