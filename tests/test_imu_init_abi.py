"""The record layouts of vieo_imu_init against the C header: sizeof / offsetof as gcc sees include/vieo_hot.h (which also
carries a static assertion on the sizes) must be what the numpy dtypes of vieo_slam_amd/imu_init.py say, the entry must be
declared and in the built library, and the constants of the cap must agree (no GPU: the header is plain C)."""
import os
import subprocess

import pytest

from vieo_slam_amd import _lib
from vieo_slam_amd import imu_init as ii

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDS = {"vieo_imu_init_seq": (ii.IMU_INIT_SEQ_DTYPE, 128), "vieo_imu_init_point": (ii.IMU_INIT_POINT_DTYPE, 20),
           "vieo_imu_init_result": (ii.IMU_INIT_RESULT_DTYPE, 376)}
CONSTANTS = {"VIEO_IMU_INIT_MAX_KF": ii.MAX_KF, "VIEO_IMU_INIT_MAX_SEQ": ii.MAX_SEQ, "VIEO_IMU_INIT_MAX_SWEEPS": ii.MAX_SWEEPS,
             "VIEO_IMU_INIT_OK": ii.OK, "VIEO_IMU_INIT_FEW_KF": ii.FEW_KF, "VIEO_IMU_INIT_FEW_EQUATIONS": ii.FEW_EQUATIONS,
             "VIEO_IMU_INIT_DEGENERATE_GRAVITY": ii.DEGENERATE_GRAVITY}


@pytest.fixture(scope="module")
def header_values(tmp_path_factory):
    lines = []
    for name, (dt, _) in RECORDS.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        lines += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (name, f, name, f) for f in dt.names]
    lines += ['printf("%s %%d\\n", %s);' % (c, c) for c in CONSTANTS]
    d = tmp_path_factory.mktemp("imu_init_abi")
    src = d / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vieo_hot.h"\nint main(void) {\n%s\nreturn 0;\n}\n'
                   % "\n".join(lines))
    exe = str(d / "sizes")
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([exe]).decode().strip().splitlines())
    return {k: int(v) for k, v in got.items()}


@pytest.mark.parametrize("name", sorted(RECORDS))
def test_the_records_match_the_header(header_values, name):
    dt, size = RECORDS[name]
    assert header_values[name] == dt.itemsize == size
    for f in dt.names:
        assert header_values["%s.%s" % (name, f)] == dt.fields[f][1], f


def test_the_constants_of_the_cap_and_the_statuses(header_values):
    for c, v in CONSTANTS.items():
        assert header_values[c] == v, c
    # the rows of a sequence at the cap fit into the LDS of one workgroup (160 KiB)
    assert 3 * (ii.MAX_KF - 2) * 7 * 8 == 85680 <= 160 * 1024
    header = open(os.path.join(ROOT, "include", "vieo_hot.h")).read()
    assert "static_assert(sizeof(vieo_imu_init_seq) == 128" in header
    assert "deliberate departure" in header  # DEGENERATE_GRAVITY: the guard TryInitVIO lacks


def test_the_entry_is_declared_and_built():
    assert "vieo_imu_init" in set(_lib.declared_symbols())
    assert hasattr(_lib.lib(), "vieo_imu_init")
