"""CPU tests of the diffusion-map definition (tests/diffmap_ref.py) and of its C interface: the reference agrees with scanpy's own
call, scipy.sparse.linalg.eigsh(T, k, which="LM"), where the two orderings coincide and differs where they do not; the ring's
closed form; the conditions the GPU tests rely on; the layout of the two new structs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse.linalg as sla

import diffmap_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_T = {}


def operator(name):
    """(C, T as scipy CSR, D, all eigenvalues descending, the top 15 with their vectors) of a named graph, built once."""
    if name not in _T:
        Cm = ref.fixture(name)
        ip, ix, w = ref.csr_arrays(Cm)
        t, z, D = ref.transitions_D(ip, ix, w)
        T = ref.t_matrix(ip, ix, t)
        _T[name] = (Cm, T, D, z) + ref.eigen(T, 15)
    return _T[name]


def eigsh_lm(T, k, ncv=None, count=None):
    n = T.shape[0]

    def mv(x):
        if count is not None:
            count[0] += 1
        return T @ x
    v0 = np.random.default_rng(0).standard_normal(n)
    w = sla.eigsh(sla.LinearOperator((n, n), matvec=mv, dtype=np.float64), k=k, which="LM", ncv=ncv, v0=v0, tol=0, return_eigenvectors=False)
    return np.sort(w)[::-1]


@pytest.mark.parametrize("name", ["traj500", "blobs3"])
def test_reference_agrees_with_eigsh_where_the_orderings_coincide(name):
    Cm, T, D, z, w_all, lam, V = operator(name)
    assert abs(w_all[-1]) < lam[-1]                                   # |lambda_min| < lambda_15: 'LM' and 'LA' pick the same set
    got = eigsh_lm(T, 15)
    assert np.abs(got - lam).max() <= 1e-12
    R = T @ V - V * lam[None, :]
    assert np.sqrt((R * R).sum(axis=0)).max() <= 1e-13 and ref.sign_rule_holds(V)


def test_reference_differs_from_eigsh_on_the_odd_ring():
    Cm, T, D, z, w_all, lam, V = operator("ring257")
    got = eigsh_lm(T, 5)
    assert got.min() < -0.999 and lam[:5].min() > 0.998                # 'LM' takes the pairs next to -1


def test_ring_closed_form():
    Cm, T, D, z, w_all, lam, V = operator("ring257")
    assert Cm.nnz == 514 and np.abs(Cm.data - 1.0).max() <= 4 * ref.U       # every weight is 1 (to the rounding of the coordinates)
    assert np.abs(T.data - 0.5).max() <= 8 * ref.U
    want = np.sort(np.cos(2.0 * np.pi * np.arange(257) / 257.0))[::-1]
    assert np.abs(w_all - want).max() <= 1e-14
    assert abs(w_all[-1] + 0.99993) < 1e-5
    for m in (1, 3, 5):                                               # no degenerate pair is cut
        assert w_all[m - 1] - w_all[m] > 1e-4


def test_traj500_conditions():
    Cm, T, D, z, w_all, lam, V = operator("traj500")
    assert ref.components(Cm)[0] == 1 and Cm.nnz == 9058 and np.diff(Cm.indptr).max() == 29
    assert (abs(Cm - Cm.T)).nnz == 0 and (T != T.T).nnz == 0          # C and T: the same bits both ways
    assert abs(w_all[0] - 1.0) <= 1e-14 and abs(w_all[1] - 0.99925) < 1e-5 and abs(w_all[2] - 0.99786) < 1e-5
    assert abs(w_all[14] - 0.8906) < 1e-4
    assert abs(np.diff(-w_all[:16]).min() - 7.5e-4) < 1e-5 and ref.gaps(w_all, 15).min() >= 7.5e-4
    assert abs(w_all[-1] + 0.412) < 1e-3
    assert D <= 4 * ref.U
    count = [0]
    w6 = eigsh_lm(T, 6, ncv=14, count=count)
    assert np.abs(w6 - w_all[:6]).max() <= 1e-12 and count[0] > 3 * 14    # far more products than one basis holds: it restarts


def test_blobs3_conditions():
    Cm, T, D, z, w_all, lam, V = operator("blobs3")
    assert ref.components(Cm)[0] == 3
    assert np.abs(w_all[:3] - 1.0).max() <= 1e-14 and abs((w_all[2] - w_all[3]) - 0.133) < 1e-3
    assert abs(w_all[-1] + 0.486) < 1e-3


def test_small_graphs_and_rows():
    for n in (2, 5, 63, 64, 65, 257):
        Cm = ref.fixture("traj%d" % n)
        assert Cm.shape == (n, n) and np.diff(Cm.indptr).min() >= 1 and (abs(Cm - Cm.T)).nnz == 0
    ip, ix, w = ref.csr_arrays(ref.fixture("traj2"))
    t = ref.transitions(ip, ix, w)[0]
    assert np.abs(np.linalg.eigvalsh(ref.t_matrix(ip, ix, t).toarray()) - [-1.0, 1.0]).max() <= 4 * ref.U
    lens = set(np.diff(ref.fixture("traj257k7").indptr).tolist()) | set(np.diff(ref.fixture("traj257k8").indptr).tolist())
    assert {7, 8, 9, 17} <= lens                                      # the k-NN graphs whose T is compared entry by entry
    lens = np.diff(ref.fixture("rows8").indptr)
    assert lens.max() == 300 and {7, 8, 9, 17} <= set(lens.tolist())
    # the lane-group order is a reordering of the plain row sum
    Cm = ref.fixture("rows8")
    ip, ix, w = ref.csr_arrays(Cm)
    for G in (4, 8, 16):
        assert np.abs(ref.group_rowsum(ip, w, G) - np.asarray(Cm.sum(axis=1)).ravel()).max() <= 1e-12


def test_pseudotime_of_the_reference_follows_the_trajectory():
    Cm, T, D, z, w_all, lam, V = operator("traj500")
    p0, D0 = ref.dpt_D(lam, V, 0)
    p1, _ = ref.dpt_D(lam, V, 499)
    assert p0[0] == 0.0 and p0.max() == 1.0 and np.argmax(p0) > 400 and np.argmax(p1) < 100
    assert np.corrcoef(p0, np.arange(500))[0, 1] > 0.9
    assert lam[0] >= ref.CAP > lam[1] and D0 < 1e-9
    # cap = 1 changes the result only if lambda_0 came out below 1: then its weight is 1 / (1 - lambda_0), about 2^52
    assert np.array_equal(p0, ref.dpt(lam, V, 0, cap=1.0)) == bool(lam[0] >= 1.0)


def test_diffmap_struct_layouts_match_header():
    """sizeof() of the two new ctypes mirrors equals what the C compiler lays out (checked with gcc), field by field."""
    from singlerust_amd import _ffi
    fields = {"srx_diffmap_opts": _ffi.DiffmapOpts, "srx_diffmap_info": _ffi.DiffmapInfo}
    body = "".join('printf("%%zu\\n", sizeof(%s));' % s for s in fields)
    for s, m in fields.items():
        body += "".join('printf("%%zu\\n", offsetof(%s, %s));' % (s, f) for f, _ in m._fields_)
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "srx.h"\nint main(void){%s return 0;}' % body
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(prog)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        got = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).split()]
    want = [C.sizeof(m) for m in fields.values()]
    for m in fields.values():
        want += [getattr(m, f).offset for f, _ in m._fields_]
    assert got == want and C.sizeof(_ffi.DiffmapOpts) == 32 and C.sizeof(_ffi.DiffmapInfo) == 64
    assert _ffi.DIFFMAP_GROUP == int(subprocess.check_output(
        ["sh", "-c", "echo SRX_DIFFMAP_GROUP | gcc -E -P -include %s -" % os.path.join(ROOT, "include", "srx.h")]).split()[-1])
