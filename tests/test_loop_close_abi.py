"""The record layouts of vieo_search_by_projection_scw / vieo_fuse_scw / vieo_compute_sim3 against the C header: sizeof / offsetof as gcc sees
include/vieo_hot.h must be what the numpy dtypes of vieo_slam_amd/loop_closing.py say (no GPU: the header is plain C), and
the new symbols are declared and exported."""
import os
import subprocess

from vieo_slam_amd import _lib
from vieo_slam_amd import loop_closing as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_new_records_match_the_header(tmp_path):
    dtypes = {"vieo_scw_visit": lc.SCW_VISIT_DTYPE, "vieo_fuse_scw_visit": lc.FUSE_SCW_VISIT_DTYPE,
              "vieo_loop_keyframe": lc.LOOP_KEYFRAME_DTYPE, "vieo_compute_sim3_visit": lc.COMPUTE_SIM3_VISIT_DTYPE,
              "vieo_compute_sim3_result": lc.COMPUTE_SIM3_RESULT_DTYPE}
    lines = []
    for name, dt in dtypes.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        lines += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f) for f in dt.names]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vieo_hot.h"\nint main(void) {\n%s\nreturn 0;\n}\n'
                   % "\n".join(lines))
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([exe]).decode().strip().splitlines())
    got = {k: int(v) for k, v in got.items()}
    assert [got[k] for k in dtypes] == [72, 88, 656, 32, 168]  # the key-frame record is unchanged
    for name, dt in dtypes.items():
        assert got[name] == dt.itemsize, name
        for f in dt.names:
            assert got["%s.%s" % (name, f)] == dt.fields[f][1], (name, f)


def test_the_new_symbols_are_declared():
    new = {"vieo_search_by_projection_scw", "vieo_search_by_projection_scw_tap", "vieo_fuse_scw", "vieo_fuse_scw_tap",
           "vieo_scw_gate_stats", "vieo_compute_sim3"}
    assert new <= set(_lib.declared_symbols())
    L = _lib.lib()
    assert all(hasattr(L, name) for name in new)
