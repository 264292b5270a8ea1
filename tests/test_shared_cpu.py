"""The pieces the translation units and the Python wrappers share, without a GPU: the one hash of csrc/hash.hpp, compiled
for the host, against the two Python references that were written independently of it (tests/umap_ref.py,
tests/harmony_ref.py), and the checked CSR triple of singlerust_amd/memory/processing/_common.py."""
import os
import subprocess

import numpy as np
import pytest

import harmony_ref
import umap_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIX_INPUTS = [0, 1, 0x9E3779B97F4A7C15, 2 ** 64 - 1, 123456789012345]          # those of tests/golden/make_umap_golden.py
HARMONY_CASES = [(0, 0, 0), (7, 1, 5), (2 ** 64 - 1, 3, 1000)]                  # (seed, a, i)
UNIT_INPUTS = [2 ** 64 - 1, 0x123456789ABCDEF0]


def test_hash_header_against_the_python_references(tmp_path):
    prog = ("#define __host__\n#define __device__\n#define __forceinline__ inline\n"
            '#include <cstdio>\n#include "hash.hpp"\nusing namespace srx;\nint main() {\n'
            + "".join('  printf("%%llu\\n", (unsigned long long)mix64(%dull));\n' % z for z in MIX_INPUTS)
            + '  printf("%llu\\n", (unsigned long long)splitmix64(0));\n'
            + "".join('  printf("%%llu\\n", (unsigned long long)mix64(%dull + kGold64 * (1ull + (%dull << 32) + %dull)));\n' % c
                      for c in HARMONY_CASES)
            + "".join('  printf("%%a\\n", unit53(%dull));\n' % z for z in UNIT_INPUTS)
            + "  return 0;\n}\n")
    src, exe = str(tmp_path / "h.cpp"), str(tmp_path / "h")
    open(src, "w").write(prog)
    subprocess.check_call(["g++", "-std=c++17", "-I", os.path.join(ROOT, "singlerust_amd", "csrc"), src, "-o", exe])
    out = subprocess.check_output([exe]).decode().split()
    got = [int(v) for v in out[:9]]
    kat = {int(z): int(v) for z, v in umap_ref.golden()["hash"]["mix"]}
    assert got[:5] == [umap_ref.mix_int(z) for z in MIX_INPUTS] == [kat[z] for z in MIX_INPUTS]
    assert got[5] == 0xE220A8397B1DCDAF                                             # splitmix64's first output for seed 0
    assert got[6:9] == [int(harmony_ref.hashes(seed, a, i + 1)[i]) for seed, a, i in HARMONY_CASES]
    assert [float.fromhex(v) for v in out[9:]] == [(z >> 11) * 2.0 ** -53 for z in UNIT_INPUTS]
    assert float.fromhex(out[9]) == 1.0 - 2.0 ** -53                                # the largest value stays below 1


def test_csr_triple():
    import scipy.sparse as sp

    from singlerust_amd.memory.processing._common import csr_triple
    W = umap_ref.ring(12)
    want = (W.indptr.astype(np.uint64), W.indices.astype(np.uint32), W.data)
    # a scipy matrix whose rows are stored in descending column order
    rev = np.concatenate([np.arange(W.indptr[i], W.indptr[i + 1])[::-1] for i in range(12)])
    U = sp.csr_matrix((W.data[rev], W.indices[rev], W.indptr), shape=W.shape)
    assert not U.has_sorted_indices
    for m in (W, U, W.tocoo()):
        got = csr_triple(m, "x_csr")
        assert [a.dtype for a in got] == [np.uint64, np.uint32, np.float64] and all(a.flags.c_contiguous for a in got)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert not U.has_sorted_indices                                                  # the caller's matrix is left as it was
    # a triple passes through: converted, not reordered or checked beyond its shape
    got = csr_triple([W.indptr, W.indices[rev], W.data[rev]], "x_csr")
    assert np.array_equal(got[1], W.indices[rev]) and np.array_equal(got[2], W.data[rev]) and got[0].dtype == np.uint64
    ready = csr_triple(want, "x_csr")
    assert all(a is b for a, b in zip(ready, want))                                  # nothing is copied that is already in form
    for bad in ((W.indptr, W.indices, W.data[:-1]), (W.indptr.reshape(1, -1), W.indices, W.data), ([], [], [])):
        with pytest.raises(ValueError, match=r"^who_csr: indptr \(n \+ 1\), indices and data \(nnz each\) expected$"):
            csr_triple(bad, "who_csr")
    with pytest.raises(ValueError, match=r"^who_csr: indptr\[n\] does not equal the number of stored entries$"):
        csr_triple((W.indptr[:-1], W.indices, W.data), "who_csr")
