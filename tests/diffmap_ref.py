"""Host restatement of the diffusion-map definition of include/srx.h (numpy / scipy), independent of the device code: the
transition operator with its row sums in the lane-group order, a dense numpy.linalg.eigh solve with the sign rule, DPT's
distance from a root, and the graphs the CPU and GPU tests share (all built here through tests/graph_ref.py)."""
import numpy as np
import scipy.sparse as sp

import graph_ref
import umap_ref

CAP = 0.9994
TOL = 1e-10
U = 2.0 ** -53


# ---- graphs -----------------------------------------------------------------------------------------------------------------
def knn_lists(x, k):
    """(indices, distances) n x k of the exact k nearest other points, ascending by (distance, index)."""
    x = np.asarray(x, dtype=np.float64)
    d2 = ((x[:, None, :] - x[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d2, np.inf)
    idx = np.argsort(d2, axis=1, kind="stable")[:, :k]
    return idx, np.sqrt(np.take_along_axis(d2, idx, axis=1))


def connectivities(x, k):
    """C of the points' k-NN lists by the definition of the neighbour graph (graph_ref)."""
    idx, dist = knn_lists(x, k)
    C = graph_ref.graph(idx, dist)[1]
    return C


def traj_points(n, rng):
    t = np.sort(rng.uniform(0.0, 1.0, n))
    return np.stack([t, np.sin(3.0 * t), t * t], axis=1) + 0.03 * rng.standard_normal((n, 3))


def blob_points(rng):
    return rng.standard_normal((450, 5)) + np.repeat([0.0, 4.0, 8.0], 150)[:, None]


_CACHE = {}


def points(name):
    """(points, k) of a graph that is built from k-NN lists: traj500, blobs3 (the same generator continued), ring257 (257
    points on a circle, k = 2: every weight is 1), traj<n> for the small trajectory graphs (traj2: one edge) and traj<n>k<k>
    for trajectory graphs of another k (traj257k7 and traj257k8 together hold rows of 7, 8, 9 and 17 entries)."""
    key = "pts_" + name
    if key not in _CACHE:
        if name in ("traj500", "blobs3"):
            rng = np.random.default_rng(7)
            _CACHE["pts_traj500"] = (traj_points(500, rng), 15)
            _CACHE["pts_blobs3"] = (blob_points(rng), 15)
        elif name == "ring257":
            a = 2.0 * np.pi * np.arange(257) / 257
            _CACHE[key] = (np.stack([np.cos(a), np.sin(a)], axis=1), 2)
        elif name.startswith("traj") and "k" in name:
            n, k = (int(v) for v in name[4:].split("k"))
            _CACHE[key] = (traj_points(n, np.random.default_rng(2000 + n + k)), k)
        elif name.startswith("traj"):
            n = int(name[4:])
            _CACHE[key] = (traj_points(n, np.random.default_rng(1000 + n)), min(15, n - 1))
        else:
            raise KeyError(name)
    return _CACHE[key]


def fixture(name):
    """The named graph as a scipy CSR with sorted indices (built once): the graphs of points(), and rows<G>, the hub-of-300
    graph of the UMAP tests with rows of G - 1, G, G + 1 and 2 G + 1 entries."""
    if name not in _CACHE:
        _CACHE[name] = umap_ref.star_rows(int(name[4:])) if name.startswith("rows") else connectivities(*points(name))
    return _CACHE[name]


def csr_arrays(W):
    W = W.tocsr()
    W.sort_indices()
    return W.indptr.astype(np.uint64), W.indices.astype(np.uint32), W.data.astype(np.float64)


def components(W):
    return sp.csgraph.connected_components(W, directed=False)


# ---- transitions ------------------------------------------------------------------------------------------------------------
def group_rowsum(indptr, vals, G):
    """Row sums in the order the header fixes: lane s of G adds the entries lo + s, lo + s + G, ... in that order, then the lanes'
    sums meet in a butterfly (offsets G / 2, .., 1)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    n = len(indptr) - 1
    lens = np.diff(indptr)
    L = max(int(-(-lens.max() // G) * G), G) if n else G
    M = np.zeros((n, L), dtype=vals.dtype)
    rows = np.repeat(np.arange(n), lens)
    pos = np.arange(len(vals)) - indptr[rows]
    M[rows, pos] = vals
    part = np.zeros((n, G), dtype=vals.dtype)
    for t in range(L // G):
        part = part + M[:, t * G:(t + 1) * G]
    off = G // 2
    while off:
        part = part + part[:, np.arange(G) ^ off]
        off //= 2
    return part[:, 0]


def transitions(indptr, indices, data, density_normalize=True, G=8, dtype=np.float64):
    """T's values in the CSR's order, every operation of the definition rounded once in `dtype`."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    c = np.asarray(data, dtype=np.float64).astype(dtype)
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    if density_normalize:
        q = group_rowsum(indptr, c, G)
        k = c / (q[rows] * q[indices])
    else:
        k = c
    z = group_rowsum(indptr, k, G)
    rz = np.sqrt(z)
    return k / (rz[rows] * rz[indices]), z


def transitions_D(indptr, indices, data, density_normalize=True, G=8):
    """(T f64, z, D): D = max |f64 - longdouble| of the reference itself."""
    t, z = transitions(indptr, indices, data, density_normalize, G)
    tl, _ = transitions(indptr, indices, data, density_normalize, G, dtype=np.longdouble)
    return t, z, float(np.abs(t.astype(np.longdouble) - tl).max()) if t.size else 0.0


def t_matrix(indptr, indices, tdata):
    n = len(indptr) - 1
    return sp.csr_matrix((tdata, np.asarray(indices, dtype=np.int64), np.asarray(indptr, dtype=np.int64)), shape=(n, n))


# ---- eigenpairs -------------------------------------------------------------------------------------------------------------
def fix_signs(V):
    """Each column's component of largest magnitude positive, the lowest index winning ties."""
    V = np.array(V, dtype=np.float64)
    for l in range(V.shape[1]):
        i = int(np.argmax(np.abs(V[:, l])))           # argmax returns the first maximum
        if V[i, l] < 0:
            V[:, l] = -V[:, l]
    return V


def used_comps(n, n_comps=15):
    return min(n_comps, n - 1)


def eigen(T, n_comps=15):
    """(all eigenvalues descending, the n_comps algebraically largest, their eigenvectors with the sign rule) by a dense solve."""
    w, v = np.linalg.eigh(T.toarray())
    w, v = w[::-1], v[:, ::-1]
    m = used_comps(T.shape[0], n_comps)
    return w, w[:m].copy(), fix_signs(v[:, :m])


def sign_rule_holds(V):
    for l in range(V.shape[1]):
        a = np.abs(V[:, l])
        if not V[int(np.argmax(a)), l] > 0:
            return False
    return True


def gaps(w_all, m):
    """delta_l for l < m: the distance of eigenvalue l to its nearest neighbour in the whole spectrum."""
    out = np.empty(m)
    for l in range(m):
        d = []
        if l > 0:
            d.append(w_all[l - 1] - w_all[l])
        if l + 1 < len(w_all):
            d.append(w_all[l] - w_all[l + 1])
        out[l] = min(d)
    return out


# ---- pseudotime -------------------------------------------------------------------------------------------------------------
def dpt(evals, evecs, root, cap=CAP, dtype=np.float64):
    lam = np.asarray(evals, dtype=np.float64).astype(dtype)
    V = np.asarray(evecs, dtype=np.float64).astype(dtype)
    one = dtype(1.0)
    w = np.where(lam < dtype(cap), lam / (one - np.where(lam < dtype(cap), lam, dtype(0.0))), one)
    s = np.zeros(V.shape[0], dtype=dtype)
    for l in range(V.shape[1]):
        t = w[l] * (V[root, l] - V[:, l])
        s = t * t if l == 0 else s + t * t
    d = np.sqrt(s)
    fin = d[np.isfinite(d)]
    mx = fin.max() if fin.size else dtype(0.0)
    return d / mx if mx > 0 else np.zeros_like(d)


def dpt_D(evals, evecs, root, cap=CAP):
    p = dpt(evals, evecs, root, cap)
    pl = dpt(evals, evecs, root, cap, dtype=np.longdouble)
    return p, float(np.abs(p.astype(np.longdouble) - pl).max())
