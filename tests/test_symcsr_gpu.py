"""The check of a caller-supplied symmetric CSR (symcsr.hip) through all three entries that run it: srx_louvain_csr,
srx_umap_csr and srx_diffmap_csr.  One table of defects; every entry refuses each with SRX_E_ARG, a message that starts with
its own prefix and is otherwise the same for the three, and untouched outputs; the order of precedence with several defects
at once; a graph whose last workgroup of the check is partly filled; and the valid graphs afterwards on the same context."""
import ctypes as C

import numpy as np
import pytest

import umap_ref as ref

pytestmark = pytest.mark.gpu

ENTRIES = ("louvain", "umap", "diffmap")
N_COMPS = 3
LABEL_SENTINEL, F64_SENTINEL = 0xDEADBEEF, -7.5


def call(ctx, entry, indptr, indices, data, n=None):
    """(rc, message, outputs) of one entry on the raw arrays; the outputs start as sentinels."""
    from singlerust_amd import _ffi as F
    lib = F.lib()
    ip, ix, w = (np.ascontiguousarray(indptr, np.uint64), np.ascontiguousarray(indices, np.uint32),
                 np.ascontiguousarray(data, np.float64))
    n = len(ip) - 1 if n is None else n
    if entry == "louvain":
        outs = [np.full(n, LABEL_SENTINEL, np.uint32)]
        info = F.LouvainInfo()
        rc = lib.srx_louvain_csr(ctx.handle, F.ptr(ip), F.ptr(ix), F.ptr(w), n, None, F.ptr(outs[0]), C.byref(info))
    elif entry == "umap":
        outs = [np.full((n, 2), F64_SENTINEL)]
        info = F.UmapInfo()
        opts = F.UmapOpts(0.0, 0.0, 0.5, 1.0, 1.0, 1.0, 3, 10, 0, 2, 5, F.UMAP_INIT_RANDOM, 0)
        rc = lib.srx_umap_csr(ctx.handle, F.ptr(ip), F.ptr(ix), F.ptr(w), n, C.byref(opts), None, F.ptr(outs[0]), C.byref(info))
    else:
        outs = [np.full(N_COMPS, F64_SENTINEL), np.full((n, N_COMPS), F64_SENTINEL)]
        info = F.DiffmapInfo()
        opts = F.DiffmapOpts(0.0, 0, N_COMPS, 0, 0, 1)
        rc = lib.srx_diffmap_csr(ctx.handle, F.ptr(ip), F.ptr(ix), F.ptr(w), n, C.byref(opts), F.ptr(outs[0]), F.ptr(outs[1]),
                                 C.byref(info))
    msg = lib.srx_last_error(ctx.handle)
    return rc, (msg or b"").decode(), outs


def refused_alike(ctx, indptr, indices, data, word):
    """Every entry refuses the graph: E_ARG, its own prefix, the same remainder (which holds `word`), sentinels intact."""
    from singlerust_amd import _ffi as F
    rest = set()
    for entry in ENTRIES:
        rc, msg, outs = call(ctx, entry, indptr, indices, data)
        assert rc == F.E_ARG, (entry, rc, msg)
        assert msg.startswith(entry + ": "), (entry, msg)
        for o in outs:
            assert (o == (LABEL_SENTINEL if o.dtype == np.uint32 else F64_SENTINEL)).all(), (entry, msg)
        rest.add(msg[len(entry) + 2:])
    assert len(rest) == 1 and word in next(iter(rest)), (word, rest)
    return next(iter(rest))


def runs(ctx, W):
    """The valid graph goes through each entry."""
    from singlerust_amd import _ffi as F
    n = W.shape[0]
    for entry in ENTRIES:
        rc, msg, outs = call(ctx, entry, W.indptr, W.indices, W.data)
        assert rc == F.OK, (entry, msg)
        if entry == "louvain":
            assert outs[0].max() < n
        elif entry == "umap":
            assert np.isfinite(outs[0]).all() and (outs[0] != F64_SENTINEL).any()
        else:
            assert abs(outs[0][0] - 1.0) <= 1e-9 and np.isfinite(outs[1]).all()


def chorded_ring(n=67):
    """The ring plus the chords i to i + 5: four entries per row, several waves of the check, a partly filled last workgroup."""
    edges = [(i, (i + 1) % n, 0.2 + 0.8 * ((i * 3) % 11) / 10.0) for i in range(n)]
    edges += [(i, (i + 5) % n, 0.1 + 0.05 * (i % 7)) for i in range(n)]
    return ref.sym_csr(n, edges)


def test_every_defect_is_refused_alike(ctx):
    W = ref.ring(12)
    ip, ix, w = W.indptr.copy(), W.indices.copy(), W.data.copy()
    assert np.array_equal(np.diff(ip), [2] * 12) and list(ix[2:4]) == [0, 2]          # row 1 holds the columns 0 and 2
    bad = ix.copy(); bad[3] = 12                                                     # an index equal to n
    assert refused_alike(ctx, ip, bad, w, "index") == "a column index is not below n = 12"
    bad = ix.copy(); bad[2] = 1                                                      # row 1 names itself
    refused_alike(ctx, ip, bad, w, "diagonal")
    bad = ix.copy(); bad[[2, 3]] = bad[[3, 2]]                                       # two columns swapped
    refused_alike(ctx, ip, bad, w, "ascending")
    bad = ix.copy(); bad[3] = bad[2]                                                 # a duplicate is not strictly ascending
    refused_alike(ctx, ip, bad, w, "ascending")
    for v in (0.0, -1.0, np.nan, np.inf):
        bw = w.copy(); bw[2] = v
        refused_alike(ctx, ip, ix, bw, "weight")
    bw = w.copy(); bw[0] = np.nextafter(bw[0], 2.0)                                  # W_ij and W_ji differ in the last bit
    refused_alike(ctx, ip, ix, bw, "symmetric")
    # W_01 without W_10; the vertices 1 and 2 share an edge of their own, so that no row is empty (diffmap's own host check)
    refused_alike(ctx, [0, 1, 2, 3], [1, 2, 1], [1.0, 0.5, 0.5], "symmetric")
    bp = ip.copy(); bp[0] = 1
    assert refused_alike(ctx, bp, ix, w, "indptr") == "indptr[0] is not 0"
    bp = ip.copy(); bp[3] = 3                                                        # 0 2 4 3 8 ...: no row is empty
    assert refused_alike(ctx, bp, ix, w, "indptr") == "indptr decreases at row 2"
    runs(ctx, W)


def test_precedence_with_several_defects(ctx):
    """range, diagonal, order, weight, symmetry: each is reported only when those before it are absent."""
    W = ref.ring(12)
    ip = W.indptr
    defects = [("index", lambda ix, w: ix.__setitem__(3, 12)),                        # row 1
               ("diagonal", lambda ix, w: ix.__setitem__(8, 4)),                      # row 4: 3 5 -> 4 5
               ("ascending", lambda ix, w: ix.__setitem__(slice(14, 16), ix[14:16][::-1].copy())),      # row 7
               ("weight", lambda ix, w: w.__setitem__(20, -1.0)),                     # row 10
               ("symmetric", lambda ix, w: w.__setitem__(0, np.nextafter(w[0], 2.0)))]
    for first in range(len(defects)):
        ix, w = W.indices.copy(), W.data.copy()
        for _, apply in defects[first:]:
            apply(ix, w)
        refused_alike(ctx, ip, ix, w, defects[first][0])
    runs(ctx, W)


def test_defect_in_the_last_row_of_a_partly_filled_workgroup(ctx):
    n = 67
    W = chorded_ring(n)
    ip, ix, w = W.indptr, W.indices, W.data
    lo = int(ip[n - 1])
    assert (n + 3) // 4 == 17 and n % 4 == 3 and list(ix[lo:]) == [0, 4, 61, 65]
    bad = ix.copy(); bad[lo + 3] = n
    refused_alike(ctx, ip, bad, w, "index")
    bad = ix.copy(); bad[lo + 2] = n - 1
    refused_alike(ctx, ip, bad, w, "diagonal")
    bad = ix.copy(); bad[[lo, lo + 1]] = bad[[lo + 1, lo]]
    refused_alike(ctx, ip, bad, w, "ascending")
    bw = w.copy(); bw[lo + 1] = 0.0
    refused_alike(ctx, ip, ix, bw, "weight")
    bw = w.copy(); bw[lo + 3] = np.nextafter(bw[lo + 3], 2.0)
    refused_alike(ctx, ip, ix, bw, "symmetric")
    runs(ctx, W)
