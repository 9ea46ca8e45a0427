"""Normalised min-sum with a layered (serial) schedule on the GPU.

The flooding schedule of the other decoders lets every check read the same posteriors and then updates every variable.  Here the checks are cut
into layers whose members share no column, and a layer reads the posteriors the layers before it left, so one iteration carries information across
the whole graph and the iteration usually needs fewer of them.  Inside a layer every posterior is touched by one check at most, so the order of
the checks of a layer cannot matter and the result is a pure function of the inputs and the layers.

The semantics are specified at ``qldpc_layered_decoder_create`` in ``include/qldpc_hip.h``; ``tests/layered_model.py`` is the numpy model the
library is tested against.  The outputs are those of the flooding min-sum decoder, so OSD-0 and OSD-CS take them unchanged.
"""
import numpy as np

from .. import _lib
from .relay import _csr


def check_layers(H):
    """Greedy colouring of the rows of H (dense, scipy sparse or ``(indptr, indices, n)``) -> ``row_layer`` int32[m]: rows in ascending index, a row
    gets the smallest layer >= 0 that no earlier row sharing a column with it holds; a row without entries gets layer 0.  Host code (what
    ``qldpc_check_layers`` computes on a graph handle)."""
    indptr, indices, n = _csr(H)
    m = indptr.size - 1
    used = [0] * n                       # per column: bit c set iff a row of layer c has an entry there
    row_layer = np.zeros(m, np.int32)
    for i in range(m):
        cols = indices[indptr[i]:indptr[i + 1]].tolist()
        taken = 0
        for j in cols:
            taken |= used[j]
        c = (~taken & (taken + 1)).bit_length() - 1           # the lowest clear bit
        row_layer[i] = c
        for j in cols:
            used[j] |= 1 << c
    return row_layer


def validate_layers(H, row_layer):
    """ValueError unless ``row_layer`` is m integers >= 0 and no two rows of one layer share a column (the message names both rows) -> int32[m]."""
    indptr, indices, n = _csr(H)
    m = indptr.size - 1
    row_layer = _lib.check_row_layer(row_layer, m)
    seen = {}
    for i in np.argsort(row_layer, kind="stable").tolist():
        lay = int(row_layer[i])
        for j in indices[indptr[i]:indptr[i + 1]].tolist():
            other = seen.get((lay, j))
            if other is not None:
                raise ValueError(f"rows {other} and {i} are both in layer {lay} and share column {j}")
            seen[(lay, j)] = i
    return row_layer


def layer_count(H, row_layer):
    """Number of layers that run: distinct layer numbers over the rows with at least one entry."""
    indptr = _csr(H)[0]
    return int(np.unique(np.asarray(row_layer)[np.diff(indptr) > 0]).size)


class LayeredMinSumDecoder:
    """Layered-schedule min-sum decoder of one parity-check matrix and prior.  ``decode(syndromes)`` returns
    ``(err int8[B, n], conv uint8[B], llr f64[B, n], final_iter int32[B])``, one shot in, one shot out.  ``layers``: a ``row_layer`` (int per
    row; two rows of one layer share no column), None = ``check_layers(H)``.  ``.layers`` is the row_layer in use, ``.info`` what the kernel runs."""

    def __init__(self, H, prior, maxIter=50, alpha_mode="dynamical", alpha=1.0, clip_llr=20.0, layers=None, device=0, flags=0):
        indptr, indices, n = _csr(H)
        maxIter, clip_llr = _lib.check_layered_args(maxIter, clip_llr)
        self.prior = _lib.f64(prior).reshape(-1)
        if self.prior.size != n:
            raise ValueError(f"prior has {self.prior.size} entries, H has {n} columns")
        _lib.alpha_args(alpha_mode, alpha)
        csr = (indptr, indices, n)
        self.layers = check_layers(csr) if layers is None else validate_layers(csr, layers)
        self.graph = _lib.Graph(indptr, indices, n, device=device)
        self._dec = _lib.LayeredDecoder(self.graph, self.prior, max_iter=maxIter, alpha_mode=alpha_mode, alpha=alpha, clip_llr=clip_llr, layers=self.layers,
                                        flags=flags)
        self.info = self._dec.info()

    def decode(self, syndromes):
        syndromes = np.asarray(syndromes, dtype=np.int8)
        single = syndromes.ndim == 1
        out = self._dec.decode(syndromes.reshape(-1, self.graph.m))
        return tuple(o[0] for o in out) if single else out


def layered_minsum_decode(H, syndromes, prior, **kw):
    """One-shot form of ``LayeredMinSumDecoder(H, prior, **kw).decode(syndromes)``."""
    return LayeredMinSumDecoder(H, prior, **kw).decode(syndromes)
