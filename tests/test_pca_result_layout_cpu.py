"""The PCA result block's layout (singlerust_amd/csrc/pca_result.hpp) without a GPU: the header compiles on its own with g++
under -Werror, and every offset, the total size, the order and disjointness of the regions and locate(p) for every component
match a literal restatement of the documented layout (tests/cpp/pca_result_layout_test.cpp) — one round, plan A with deflation,
plan B, k <= 64, odd k, n_pc = 1."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "singlerust_amd", "csrc")


def test_layout_header_matches_the_documented_block(tmp_path):
    exe = str(tmp_path / "pca_result_layout_test")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
           os.path.join(ROOT, "tests", "cpp", "pca_result_layout_test.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout


def test_layout_header_is_plain_cpp():
    text = open(os.path.join(CSRC, "pca_result.hpp")).read()
    assert set(re.findall(r'#include\s+[<"]([^>"]+)[>"]', text)) <= {"cstddef", "utility", "vector"}


def test_layout_arithmetic_is_stated_once():
    """The block's strides and tail offsets appear in the header alone: no reader or writer re-derives them."""
    pats = [r"kl \+ 2 \* L", r"2 \* k \+ 2\b", r"2 \* \(size_t\)k \+ 2\b", r"\(size_t\)k \+ 1\) / 2", r"run_pca<"]
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".inl", ".hpp")) or name in ("pca_result.hpp",):
            continue
        text = open(os.path.join(CSRC, name)).read()
        for p in pats:
            if p == r"run_pca<" and name == "pca_solve.hip":
                continue
            assert not re.search(p, text), (name, p)
