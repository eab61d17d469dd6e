#!/bin/bash
# on-box A/B/C under sustained load (as ab_sustained.sh, any number of variants): bash tools/ab3_sustained.sh MODEL ROUNDS "FLAGS_A" "FLAGS_B" ...
M=${1:-phasenet}; R=${2:-2}; shift 2; T=$(mktemp -d)
for r in $(seq 1 $R); do for f in "$@"; do
VOLPICK_PLAN_FLAGS="$f" timeout -k 10 200 python bench.py --full --model $M --no-cpu-baseline --no-api --sustain-seconds 4 --detail-file $T/s_detail.json > $T/s.json 2> $T/s.err
python3 -c "
import json;d=json.loads(open('$T/s.json').read().strip().splitlines()[-1]);s=d['sustained']
print('round $r flags $f:', round(d['value']), 'windows/s (20-step regions)', round(d['ms_per_step']*1e3,1), 'us/step; sustained', round(s['value']), 'at', round(s['shader_clock_ghz'],3), 'GHz; kernel_ms', d['roofline']['kernel_ms'])" || tail -3 $T/s.err
done; done
