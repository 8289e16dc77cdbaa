"""ORBmatcher::SearchForInitialization behind the reference's signature (shim/ORBmatcher_init_hot.cc): the translation unit
is type-checked with `g++ -fsyntax-only` against the declaration-only stand-ins of tests/shim_compile/mock, as
tests/test_shim_compile.py checks the others, with tests/shim_compile/mock/init in front: its ORBmatcher.h declares the
class with the member, which the shared stand-ins lack.  A caller written the way Tracking::MonocularInitialization calls
it type-checks against the same declaration.  A syntax and ABI check, not parity evidence."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOCK = os.path.join(ROOT, "tests", "shim_compile", "mock")
INC = ["-I" + os.path.join(MOCK, "init"), "-I" + MOCK, "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "shim")]
REF = os.environ.get("VIEO_REFERENCE_ROOT", "/root/reference")


def _syntax_only(path):
    return subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror"] + INC + [path], capture_output=True, text=True)


def _declaration(text):
    m = re.search(r"int\s+SearchForInitialization\s*\([^;]*;", text)
    return re.sub(r"\s+", "", m.group(0)) if m else None


def test_the_initialisation_matcher_shim_type_checks():
    path = os.path.join(ROOT, "shim", "ORBmatcher_init_hot.cc")
    r = _syntax_only(path)
    assert r.returncode == 0, r.stderr[-3000:]
    m = open(path).read()
    assert "int ORBmatcher::SearchForInitialization(Frame& F1, Frame& F2, vector<cv::Point2f>& vbPrevMatched" in m
    assert "vieo_search_for_initialization(&P, 1," in m


def test_a_caller_as_in_monocular_initialization_type_checks(tmp_path):
    src = tmp_path / "use_init_search.cc"
    src.write_text("""#include "ORBmatcher.h"
namespace VIEO_SLAM {
int find_initial_correspondences(Frame& ini, Frame& cur, std::vector<cv::Point2f>& prev, std::vector<int>& matches) {
  ORBmatcher matcher(0.9, true);
  return matcher.SearchForInitialization(ini, cur, prev, matches, 100);
}
}  // namespace VIEO_SLAM
""")
    r = _syntax_only(str(src))
    assert r.returncode == 0, r.stderr[-3000:]


def test_the_stand_in_declares_the_member_as_the_reference_does():
    mock = _declaration(open(os.path.join(MOCK, "init", "ORBmatcher.h")).read())
    assert mock == "intSearchForInitialization(Frame&F1,Frame&F2,std::vector<cv::Point2f>&vbPrevMatched,std::vector<int>&vnMatches12,intwindowSize=10);"
    header = os.path.join(REF, "include", "ORBmatcher.h")
    if os.path.isfile(header):  # (where a checkout of the reference is at hand; nothing of it travels)
        assert _declaration(open(header).read()) == mock
