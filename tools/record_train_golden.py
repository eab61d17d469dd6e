#!/usr/bin/env python3
"""Record tests/golden/train_step_pinned.json (or the file named on the command line) on the library as built: the digests
tests/test_gpu_train_pinned.py compares against.  Record before a refactor of the training step, twice, and require equal
files: the step is deterministic, so the digests are a fair pin."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from tests.test_gpu_train_pinned import CASES, GOLDEN, run_case  # noqa: E402

out = Path(sys.argv[1]) if len(sys.argv) > 1 else GOLDEN
out.write_text(json.dumps({case: run_case(case) for case in CASES}, indent=1, sort_keys=True) + "\n")
print(f"{out}: {out.stat().st_size} bytes, launches {[json.loads(out.read_text())[c]['launch_count'] for c in CASES]}")
