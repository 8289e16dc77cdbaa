#!/usr/bin/env python3
"""After tools/pmc_fast.sh: the counter databases pmc_fast_{a,b,c,d} in its output directory -> <tag>_pmc_fast.json beside
them, in the layout bench.py's valu_issue() reads (k_fast's counters per counter instance and launch, stamped with the
hash of orb_extractor.hip); tools/finish_fast_profile.py <that file> profiles/<tag>_pmc_fast.json then adds the derived
tables.
usage: python tools/collect_fast_profile.py <tag> <output directory of pmc_fast.sh> [images per launch = 512]"""
import glob
import hashlib
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read(db):
    out, k = {}, None
    txt = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rocpd_pmc.py"), db], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    for line in txt.split("\n"):
        if not line.startswith(" "):
            k = line.strip()
            out.setdefault(k, {})
        else:
            m = re.match(r"\s+(\S+)\s+avg (\S+)\s+\(n=(\d+)\)", line)
            if m:
                out[k][m.group(1)] = float(m.group(2))
    return out


def pick(d, sub):
    ks = [k for k in d if sub in k]
    return d[ks[0]] if ks else {}


def main():
    tag = sys.argv[1]
    out_dir = os.path.abspath(sys.argv[2])
    images = int(sys.argv[3]) if len(sys.argv) > 3 else 512
    fast, desc = {}, {}
    for name in "abcd":
        dbs = glob.glob(os.path.join(out_dir, "pmc_fast_" + name, "**", "*.db"), recursive=True)
        if dbs:
            d = read(dbs[0])
            fast.update(pick(d, "k_fast"))
            desc.update(pick(d, "k_describe_fused"))
    src = os.path.join("vieo_slam_amd", "csrc", "orb_extractor.hip")
    sha = hashlib.sha256(open(os.path.join(ROOT, src), "rb").read()).hexdigest()[:16]
    valu, cyc = fast.get("SQ_INSTS_VALU", 0) / 32.0, fast.get("GRBM_GUI_ACTIVE", 0)
    out = {"source": "tools/pmc_fast.sh: rocprofv3 --pmc in separate passes over a %d-image extraction; averages per (XCD, shader engine) "
                     "counter instance = 8 CUs = 32 SIMDs and per launch" % images,
           "kernel": "k_fast", "images_per_launch": images, "counters": fast, "valu_insts_per_simd": valu, "kernel_cycles": cyc,
           "valu_insts_per_cycle_per_simd": valu / cyc if cyc else None,
           "lane_fill": fast.get("SQ_THREAD_CYCLES_VALU", 0) / (64.0 * fast["SQ_ACTIVE_INST_VALU"]) if fast.get("SQ_ACTIVE_INST_VALU") else None,
           "issue_cycles_per_valu_inst": {"full_rate": 1.9, "half_rate": 3.4, "source": "tools/ubench/valu_rate.hip on gfx950 (profiles/r2_valu_rate.txt)"},
           "source_sha16": {src: sha}}
    if desc:
        out["k_describe_fused"] = {"counters": desc, "valu_insts_per_simd": desc.get("SQ_INSTS_VALU", 0) / 32.0, "kernel_cycles": desc.get("GRBM_GUI_ACTIVE", 0),
                                   "valu_insts_per_cycle_per_simd": (desc.get("SQ_INSTS_VALU", 0) / 32.0 / desc["GRBM_GUI_ACTIVE"]) if desc.get("GRBM_GUI_ACTIVE") else None,
                                   "lds_insts_per_simd": desc.get("SQ_INSTS_LDS", 0) / 32.0}
    dst = os.path.join(out_dir, tag + "_pmc_fast.json")
    json.dump(out, open(dst, "w"), indent=1)
    cells = images * 700.0 / 1024
    print("wrote", dst, "per cell: VALU %.0f SALU %.0f LDS %.0f" % (valu / cells, fast.get("SQ_INSTS_SALU", 0) / 32.0 / cells, fast.get("SQ_INSTS_LDS", 0) / 32.0 / cells))


if __name__ == "__main__":
    main()
