"""The record layouts of the place-recognition entries against the C header: sizeof / offsetof as gcc sees
include/vieo_hot.h must be what the numpy dtypes of vieo_slam_amd/place_recognition.py say (no GPU: the header is plain C)."""
import os
import subprocess

from vieo_slam_amd import place_recognition as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_place_recognition_records_match_the_header(tmp_path):
    dtypes = {"vieo_voc_node": pr.VOC_NODE_DTYPE, "vieo_voc_info": pr.VOC_INFO_DTYPE, "vieo_bow_frame": pr.BOW_FRAME_DTYPE,
              "vieo_bow_vectors": pr.BOW_VECTORS_DTYPE}
    lines = []
    for name, dt in dtypes.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        lines += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f) for f in dt.names]
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "vieo_hot.h"\nint main(void) {\n%s\n'
            'printf("VIEO_BOW_MAX_KEYS %%zu\\n", (size_t)VIEO_BOW_MAX_KEYS);\nreturn 0;\n}\n' % "\n".join(lines))
    src = tmp_path / "sizes.c"
    src.write_text(prog)
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([exe]).decode().strip().splitlines())
    got = {k: int(v) for k, v in got.items()}
    assert [got[k] for k in dtypes] == [48, 16, 16, 48]
    for name, dt in dtypes.items():
        assert got[name] == dt.itemsize, name
        for f in dt.names:
            assert got["%s.%s" % (name, f)] == dt.fields[f][1], (name, f)
    assert got["VIEO_BOW_MAX_KEYS"] == pr.MAX_KEYS
