"""One sha256 per case and entry of the new-map-point path: two commits' libraries computed the same bytes iff their
lines are equal.  Cases: the eight CASES of tests/test_new_points.py and the ten parameter sets of
test_gpu_search_for_triangulation_parity (tests/test_tri_search.py).  Entries: vieo_search_for_triangulation,
vieo_triangulate_new_points on the rows that search left, vieo_create_new_map_points.  A hash covers the return code and
every output buffer of the call in full (rows, row counts, nmatches; status, x3d, x3d_f, accepted counts), capacity
2 * keys of pKF1 as the wrappers choose it.  Only names every commit with these entries has are used, so the file runs
unchanged against another build:
    python tools/new_points_digest.py
    VIEO_LIB_PATH=/path/to/another/libvieo_hot.so python tools/new_points_digest.py"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import test_new_points as tnp  # noqa: E402
from tests import test_tri_search as tts  # noqa: E402
from vieo_slam_amd import _lib, tri_search  # noqa: E402


def cases():
    """(name, kf1, st1, kf2s, st2s, only_stereo, check_orientation)"""
    for name, (seed, kw) in tnp.CASES.items():
        if name == "rig_stereo":
            kf1, st1, kf2s, st2s = tnp.make_rig_stereo_case(seed)[:4]
        else:
            kf1, st1, kf2s, st2s = tnp.make_case(seed, n_forced=50 if name != "small" else 5, **kw)[:4]
        yield name, kf1, st1, kf2s, st2s, False, True
    mark = [m for m in tts.test_gpu_search_for_triangulation_parity.pytestmark if m.name == "parametrize"][0]
    for seed, kw, (only_stereo, check) in mark.args[1]:
        kf1, kf2s, _ = tri_search.make_tri_scene(seed, **kw)
        if kw.get("rig"):  # the scene's keys as the parity test searches them; no depth, no groups
            mk = lambda k: tri_search.TriStereo(k, tnp.BF, depth=np.full(len(k.keys), -1, np.float32))
        else:
            mk = lambda k: tri_search.TriStereo(k, tnp.BF)
        yield "search%d" % seed, kf1, mk(kf1), kf2s, [mk(k) for k in kf2s], only_stereo, check


def digest(rc, *arrays):
    h = hashlib.sha256(b"%d" % rc)
    for a in arrays:
        h.update(str((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def main():
    L = _lib.lib()
    if not L.vieo_device_available():
        raise SystemExit("no gfx950 device: " + L.vieo_last_error().decode())
    for name, kf1, st1, kf2s, st2s, only_stereo, check in cases():
        recs = np.concatenate([k.rec for k in kf2s])
        srecs = np.concatenate([s.rec for s in st2s])
        a1, s1, a2, s2, n = kf1.rec.ctypes.data, st1.rec.ctypes.data, recs.ctypes.data, srecs.ctypes.data, len(kf2s)
        cap, stride, pairs, n_pairs, n_matches, status, x3d, x3d_f, n_new = tri_search.new_points_buffers(kf1, kf2s)
        rc = L.vieo_search_for_triangulation(a1, a2, n, int(only_stereo), int(check), cap, stride, pairs.ctypes.data,
                                             n_pairs.ctypes.data, n_matches.ctypes.data)
        print("%s vieo_search_for_triangulation (%d rows): %s" % (name, n_pairs.sum(), digest(rc, pairs, n_pairs, n_matches)))
        rc = L.vieo_triangulate_new_points(a1, s1, a2, s2, n, 0.0, cap, stride, pairs.ctypes.data, n_pairs.ctypes.data,
                                           status.ctypes.data, x3d.ctypes.data, x3d_f.ctypes.data, n_new.ctypes.data)
        print("%s vieo_triangulate_new_points (%d new): %s" % (name, n_new.sum(), digest(rc, status, x3d, x3d_f, n_new)))
        cap, stride, pairs, n_pairs, n_matches, status, x3d, x3d_f, n_new = tri_search.new_points_buffers(kf1, kf2s)
        rc = L.vieo_create_new_map_points(a1, s1, a2, s2, n, int(only_stereo), int(check), 0.0, cap, stride, pairs.ctypes.data,
                                          n_pairs.ctypes.data, n_matches.ctypes.data, status.ctypes.data, x3d.ctypes.data,
                                          x3d_f.ctypes.data, n_new.ctypes.data)
        print("%s vieo_create_new_map_points (%d new): %s"
              % (name, n_new.sum(), digest(rc, pairs, n_pairs, n_matches, status, x3d, x3d_f, n_new)))


if __name__ == "__main__":
    main()
