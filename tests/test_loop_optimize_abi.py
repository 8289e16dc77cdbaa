"""The record layout of vieo_optimize_sim3 against the C header: sizeof / offsetof as gcc sees include/vieo_hot.h (which
also carries a static assertion on the size) must be what the numpy dtype of vieo_slam_amd/loop_closing.py says, and both
entries must be in the built library (no GPU: the header is plain C)."""
import os
import subprocess

from vieo_slam_amd import _lib
from vieo_slam_amd import loop_closing as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_visit_record_matches_the_header(tmp_path):
    name, dt = "vieo_sim3_opt_visit", lc.SIM3_OPT_VISIT_DTYPE
    lines = ['printf("%s %%zu\\n", sizeof(%s));' % (name, name)]
    lines += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f) for f in dt.names]
    lines.append('printf("max_trials %d\\n", VIEO_SIM3_OPT_MAX_TRIALS);')
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vieo_hot.h"\nint main(void) {\n%s\nreturn 0;\n}\n'
                   % "\n".join(lines))
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([exe]).decode().strip().splitlines())
    got = {k: int(v) for k, v in got.items()}
    assert got[name] == dt.itemsize == 152
    for f in dt.names:
        assert got["%s.%s" % (name, f)] == dt.fields[f][1], f
    assert got["max_trials"] == lc.SIM3_OPT_MAX_TRIALS
    header = open(os.path.join(ROOT, "include", "vieo_hot.h")).read()
    assert 'static_assert(sizeof(vieo_sim3_opt_visit) == 152' in header


def test_both_entries_are_declared_and_built():
    new = {"vieo_optimize_sim3", "vieo_optimize_sim3_trace"}
    assert new <= set(_lib.declared_symbols())
    L = _lib.lib()
    assert all(hasattr(L, name) for name in new)
