"""vieo_init_pair against the C header: sizeof / offsetof as gcc sees include/vieo_hot.h must be what the numpy dtype of
vieo_slam_amd/initialization.py says (no GPU: the header is plain C); the new symbols are declared and exported; and what the
entry refuses before it asks for a device."""
import os
import subprocess

import numpy as np

from vieo_slam_amd import _lib
from vieo_slam_amd import initialization as ini

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_pair_record_matches_the_header(tmp_path):
    name, dt = "vieo_init_pair", ini.INIT_PAIR_DTYPE
    lines = ['printf("%s %%zu\\n", sizeof(%s));' % (name, name)]
    lines += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f) for f in dt.names]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vieo_hot.h"\nint main(void) {\n%s\nreturn 0;\n}\n'
                   % "\n".join(lines))
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([exe]).decode().strip().splitlines())
    got = {k: int(v) for k, v in got.items()}
    assert got[name] == dt.itemsize == 64
    for f in dt.names:
        assert got["%s.%s" % (name, f)] == dt.fields[f][1], f
    header = open(os.path.join(ROOT, "include", "vieo_hot.h")).read()
    assert "static_assert(sizeof(vieo_init_pair) == 64" in header


def test_the_new_symbols_are_declared():
    new = {"vieo_search_for_initialization", "vieo_search_for_initialization_tap"}
    assert new <= set(_lib.declared_symbols())
    L = _lib.lib()
    assert all(hasattr(L, name) for name in new)


def _refused(pairs, bounds=(0, 752, 0, 480), nn=0.9):
    rc, out = ini.search_for_initialization_call(pairs, bounds, nn)
    msg = _lib.lib().vieo_last_error().decode()
    for m12, n, _ in out:  # nothing is written by a refused call
        assert n == -7 and (m12 == -7).all()
    return rc, msg


def test_arguments_are_refused_before_anything_is_written():
    F1, F2, prev, bounds = ini.make_search_pair(5, 20, 30)
    ok = (F1, F2, prev, 100)
    assert _refused([ok], bounds=(0, 0, 0, 480))[0] == _lib.VIEO_E_INVALID
    assert _refused([ok], bounds=(0, np.inf, 0, 480))[0] == _lib.VIEO_E_INVALID
    assert _refused([ok], nn=0.0)[0] == _lib.VIEO_E_INVALID
    assert _refused([ok], nn=float("nan"))[0] == _lib.VIEO_E_INVALID
    rc, msg = _refused([ok, (F1, F2, prev, -1)])
    assert rc == _lib.VIEO_E_INVALID and "pair 1" in msg
    bad = prev.copy()
    bad[7, 1] = np.nan
    rc, msg = _refused([ok, ok, (F1, F2, bad, 100)])
    assert rc == _lib.VIEO_E_INVALID and "pair 2" in msg and "prev_matched[7]" in msg
    k = F2.keys.copy()
    k["angle"][3] = 360.0
    rc, msg = _refused([(F1, ini.InitFrame(k, F2.desc), prev, 100)])
    assert rc == _lib.VIEO_E_INVALID and "key 3 of the second frame" in msg
    k = F1.keys.copy()
    k["octave"][4] = -1
    rc, msg = _refused([(ini.InitFrame(k, F1.desc), F2, prev, 100)])
    assert rc == _lib.VIEO_E_INVALID and "key 4 of the first frame" in msg
    big = ini.make_search_pair(6, 4, 8193)
    rc, msg = _refused([(big[0], big[1], big[2], 100)])
    assert rc == _lib.VIEO_E_CAPACITY and "8193" in msg
    assert _refused([ok] * 4097)[0] == _lib.VIEO_E_CAPACITY


def test_the_tap_is_empty_without_a_call():
    import threading
    got = []
    # (the tap is per thread: a fresh thread has made no call)
    t = threading.Thread(target=lambda: got.append(_lib.lib().vieo_search_for_initialization_tap(0, None, None, None, None, 0)))
    t.start(), t.join()
    assert got == [_lib.VIEO_E_EMPTY]
