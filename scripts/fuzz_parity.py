#!/usr/bin/env python3
"""Open-ended randomised GPU-vs-oracle parity sweep (the fixed-seed cases of tests/test_gpu_fuzz.py run the same
function under `pytest -m gpu`).
  python scripts/fuzz_parity.py [--stars] [cases] [seed]
--stars: the cases on disjoint stars with exact neighbour counts (tests/_stars.py), judged per star."""
import os
import sys
import tempfile

import numpy as np

os.environ.setdefault("MTP_BANK_ROUNDS", "2")   # (search effort of the LDS-bank numbering: a load-time / speed knob only)
os.environ.setdefault("MTP_BANK_SCALE", "1")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _fuzz import fuzz_case, fuzz_star_case  # noqa: E402

args = [a for a in sys.argv[1:] if a != "--stars"]
ncase = int(args[0]) if len(args) > 0 else 12
rng = np.random.default_rng(int(args[1]) if len(args) > 1 else 2026)
tmp = tempfile.mkdtemp()
if "--stars" in sys.argv[1:]:
    worst = 0.0
    for case in range(ncase):
        desc, w = fuzz_star_case(rng, tmp, "s%d" % case)       # (asserts the per-star tolerance itself)
        worst = max(worst, *w.values())
        print("case %2d %s  error / per-star tolerance %s" % (case, desc, " ".join("%s %.1e" % kv for kv in w.items())),
              flush=True)
    print("fuzz_parity --stars: worst error / per-star tolerance %.2e" % worst)
    sys.exit(0 if worst <= 1.0 else 1)
worst = 0.0
for case in range(ncase):
    desc, err = fuzz_case(rng, tmp, "p%d" % case)
    worst = max(worst, *err.values())
    print("case %2d %s  rel err F %.1e E %.1e V %.1e G %.1e" % (case, desc, err["F"], err["E"], err["V"], err["G"]),
          flush=True)
print("fuzz_parity: worst relative error %.2e" % worst)
sys.exit(0 if worst < 1e-9 else 1)
