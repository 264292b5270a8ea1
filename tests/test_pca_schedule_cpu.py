"""The PCA solver's schedule (singlerust_amd/csrc/pca_schedule.hpp) without a GPU: the header compiles on its own with g++
under -Werror, and the filter degrees, sweep counts, rates, tolerances, plans and per-round options match known answers and a
literal copy of the expressions the host loop held inline (tests/cpp/pca_schedule_test.cpp), integers exactly, doubles to the
bit."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "singlerust_amd", "csrc")


def test_schedule_header_matches_known_answers_and_the_inline_expressions(tmp_path):
    exe = str(tmp_path / "pca_schedule_test")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
           os.path.join(ROOT, "tests", "cpp", "pca_schedule_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout


def test_schedule_header_is_plain_cpp():
    text = open(os.path.join(CSRC, "pca_schedule.hpp")).read()
    assert set(re.findall(r'#include\s+[<"]([^>"]+)[>"]', text)) <= {"algorithm", "cmath", "cstdint", "vector"}
    assert not re.search(r"__global__|__device__|\bhip[A-Z]", text)


def test_schedule_is_stated_once():
    """The schedule's constants and expressions appear in the header alone: the solver calls them."""
    pats = [r"32\.9", r"kPcaPerRoundSafe - 1", r"0\.93\b", r"std::acosh", r"\* 1e-4\)"]
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".inl", ".hpp")) or name == "pca_schedule.hpp":
            continue
        text = open(os.path.join(CSRC, name)).read()
        code = re.sub(r"//[^\n]*", "", text)
        for p in pats:
            assert not re.search(p, code), (name, p)
