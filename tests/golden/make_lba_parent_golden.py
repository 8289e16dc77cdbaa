"""Writes tests/golden/lba_parent_<case>.npz: the device results of the cases of lba_xf_cases.py, bytes and all.

Run on an MI355X from the repo root, with the library of the commit whose results are to be pinned (the parent of the
key-frame transform table; VIEO_LIB_PATH selects a build):  python tests/golden/make_lba_parent_golden.py [OUT_DIR]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests.golden import lba_xf_cases as cases  # noqa: E402

if __name__ == "__main__":
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden")
    os.makedirs(out_dir, exist_ok=True)
    for name in cases.CASES:
        recs = cases.run_hip(name, cases.build(name))
        np.savez_compressed(os.path.join(out_dir, "lba_parent_%s.npz" % name), **cases.pack(recs))
        print(name, [(int(r["res"]["lm_trials"]), int(r["res"]["lm_iterations"]), int(r["res"]["status"])) for r in recs],
              flush=True)
