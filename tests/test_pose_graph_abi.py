"""The record layouts of the pose-graph entry against the C header: sizeof / offsetof as gcc sees include/vieo_hot.h must
be what the numpy dtypes of vieo_slam_amd/pose_graph.py say (no GPU: the header is plain C)."""
import os
import subprocess

from vieo_slam_amd import _lib
from vieo_slam_amd import pose_graph as pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pose_graph_records_match_the_header(tmp_path):
    dtypes = {"vieo_sim3": pg.SIM3_DTYPE, "vieo_pose_graph": pg.POSE_GRAPH_DTYPE, "vieo_pg_trial": pg.PG_TRIAL_DTYPE,
              "vieo_pose_graph_result": pg.POSE_GRAPH_RESULT_DTYPE}
    lines = []
    for name, dt in dtypes.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        lines += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f) for f in dt.names]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "vieo_hot.h"\nint main(void) {\n%s\nreturn 0;\n}\n' % "\n".join(lines)
    src = tmp_path / "sizes.c"
    src.write_text(prog)
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([exe]).decode().strip().splitlines())
    got = {k: int(v) for k, v in got.items()}
    assert [got[k] for k in dtypes] == [64, 104, 32, 88]
    for name, dt in dtypes.items():
        assert got[name] == dt.itemsize, name
        assert dt.itemsize % 8 == 0
        for f in dt.names:
            assert got["%s.%s" % (name, f)] == dt.fields[f][1], (name, f)


def test_pose_graph_symbols_are_declared():
    assert {"vieo_optimize_essential_graph", "vieo_pose_graph_linearize", "vieo_pose_graph_solve"} <= set(_lib.declared_symbols())
    assert (pg.EDGE_LOOP, pg.EDGE_PRIOR) == (0, 1)
