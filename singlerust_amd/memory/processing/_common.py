"""What the wrappers of this package share: the checked CSR triple of a caller-supplied graph, the graph handle of an adata,
the dict of a flat info struct and the owning wrapper of a device handle."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ... import _ffi as F

_SCALARS = (C.c_int32, C.c_uint32, C.c_int64, C.c_uint64, C.c_double)


def csr_triple(matrix, who: str):
    """(indptr uint64, indices uint32, data f64), contiguous, of a scipy sparse matrix (columns sorted here) or of an
    (indptr, indices, data) triple (passed through); ``who`` names the caller in the two ``ValueError`` texts."""
    if isinstance(matrix, (tuple, list)):
        indptr, indices, data = matrix
    else:
        m = matrix.tocsr()
        if not m.has_sorted_indices:
            m = m.sorted_indices()
        indptr, indices, data = m.indptr, m.indices, m.data
    indptr = np.ascontiguousarray(indptr, dtype=np.uint64)
    indices = np.ascontiguousarray(indices, dtype=np.uint32)
    data = np.ascontiguousarray(data, dtype=np.float64)
    if indptr.ndim != 1 or indptr.size < 1 or indices.shape != data.shape or indices.ndim != 1:
        raise ValueError("%s: indptr (n + 1), indices and data (nnz each) expected" % who)
    if int(indptr[-1]) != indices.size:
        raise ValueError("%s: indptr[n] does not equal the number of stored entries" % who)
    return indptr, indices, data


def graph_of(adata, who: str):
    """The ``Graph`` that ``neighbors(adata, connectivities=True)`` left with the adata."""
    g = getattr(adata, "_graph", None)
    if g is None or not g.handle:
        raise F.SrxError(F.E_ARG, "%s: the adata holds no graph; run neighbors(adata, connectivities=True) first" % who)
    return g


def flat_info(struct) -> dict:
    """A ctypes info struct of scalar fields as a dict, without its padding: ctypes hands an integer field out as ``int``
    and a double as ``float``, so nothing is converted.  A struct with an array field is not flat and is refused."""
    assert all(t in _SCALARS for _, t in struct._fields_), type(struct).__name__
    return {name: getattr(struct, name) for name, _ in struct._fields_ if name != "reserved_"}


class OwnedHandle:
    """Owning wrapper of a device handle: ``_free`` names the C function that releases it."""

    _free = None

    def __init__(self, ctx, handle):
        self.ctx = ctx
        self._h = handle

    @property
    def handle(self):
        return self._h

    def free(self) -> None:
        if self._h:
            # a handle must not outlive its context: once the context is closed the device memory has gone with it and only
            # the handle is dropped
            if getattr(self.ctx, "_h", None):
                getattr(F.lib(), self._free)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
