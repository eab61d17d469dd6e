#!/bin/bash
# A/B of two EQTransformer plans on one box: bench lines + per-launch times.  usage: ab_eqt.sh FLAGS_A FLAGS_B
T=$(mktemp -d)
for v in A B; do
  if [ $v = A ]; then f="$1"; else f="$2"; fi
  VOLPICK_PLAN_FLAGS="$f" timeout -k 10 200 python bench.py --full --model eqtransformer --no-cpu-baseline --sustain-seconds 0 --no-api --detail-file $T/ab_$v.json > /dev/null 2> $T/ab_$v.err
done
python - "$1" "$2" "$T" <<'PY'
import json, sys
d = {}
T = sys.argv[3]
for v, f in zip("AB", sys.argv[1:3]):
    try:
        d[v] = json.load(open(f"{T}/ab_{v}.json"))
        print(v, f"flags={f!r}", round(d[v]["value"]), "windows/s", round(d[v]["ms_per_step"], 4), "ms/step  sum of launches", round(d[v]["forward"]["sum_kernel_ms"], 4))
    except Exception as e:
        print(v, "ERR", e, open(f"{T}/ab_{v}.err").read()[-400:])
if len(d) == 2:
    for ka, kb in zip(d["A"]["forward"]["kernels"], d["B"]["forward"]["kernels"]):
        print(f"  {ka['name'][:34]:34s} {ka['ms']*1e3:8.1f} {kb['ms']*1e3:8.1f} us")
PY
