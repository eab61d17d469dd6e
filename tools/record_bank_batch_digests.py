#!/usr/bin/env python3
"""Records the fixtures of tests/test_gpu_bank_batch_pinned.py on a GPU: the rows (tests/golden/bank_batch_rows.npz) and
the sha256 of what every batch generator writes for them (tests/golden/bank_batch_digests.json).

  python tools/record_bank_batch_digests.py [--check]

Run it with the library whose bits are to be pinned (VOLPICK_HIP_LIB selects one) *before* changing the generation code.
--check records nothing: it runs the cases against the committed rows and reports every digest that differs."""
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from tests import bank_batch_pinned as P  # noqa: E402
from volpick_amd import generate as G  # noqa: E402


def main():
    if "--check" in sys.argv[1:]:
        rows = {k: v.view(G.AUG_ROW) for k, v in np.load(P.ROWS_FILE).items()}
        want, got = json.loads(P.DIGEST_FILE.read_text()), P.run_all(rows)
        bad = sorted(k for k in want if got.get(k) != want[k])
        print(f"{len(want)} cases, {len(bad)} differ" + "".join(f"\n  {k}" for k in bad))
        return 1 if bad or set(got) != set(want) else 0
    rows = P.all_rows()
    digests = P.run_all(rows)  # asserts the conditions on the bank and the rows
    assert digests == P.run_all(rows), "the library does not reproduce its own bits"
    np.savez_compressed(P.ROWS_FILE, **{k: v.view(np.uint8) for k, v in rows.items()})
    P.DIGEST_FILE.write_text(json.dumps(digests, indent=1, sort_keys=True) + "\n")
    print(f"recorded {len(digests)} digests, {len(rows)} row sets")
    return 0


if __name__ == "__main__":
    sys.exit(main())
