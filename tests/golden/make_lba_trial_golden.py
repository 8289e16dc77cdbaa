"""Writes tests/golden/lba_trial_<case>.npz: the device results of the cases of lba_trial_cases.py, bytes and all.

Run on an MI355X from the repo root, with the library of the commit whose results are to be pinned -- the parent of the
Schur block rule, a755442, whose diagonal tiles still compute all sixteen blocks and whose class-0 solve still reads
k_lba_assemble's Hs (VIEO_LIB_PATH selects a build):  python tests/golden/make_lba_trial_golden.py [OUT_DIR]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.golden import lba_trial_cases as cases  # noqa: E402

if __name__ == "__main__":
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden")
    os.makedirs(out_dir, exist_ok=True)
    for name in cases.CASES:
        recs = cases.run_hip(name, cases.build(name))
        np.savez_compressed(os.path.join(out_dir, "lba_trial_%s.npz" % name), **cases.pack(recs))
        print(name, [(int(r["res"]["lm_trials"]), int(r["res"]["lm_iterations"]), int(r["res"]["status"])) for r in recs],
              flush=True)
