"""OSD-CS: ordered-statistics decoding with a combination sweep (Roffe, White, Burton, Campbell, "Decoding across the quantum low-density
parity-check code landscape", 2020) on the GPU.

The post-processor keeps searching after OSD-0 has found a solution, for a lighter one.  Per shot, with H (m x n), the syndrome s, the BP
posteriors ``llr`` with their hard decision ``hard``, and per-column weights ``w`` (finite; the same for every shot):

* weights are quantised as Relay-BP's: ``q_j = floor(w_j * 2**20 + 0.5)`` (the product clamped to +-2**40), and the cost of x is
  ``W(x) = sum of q_j over x_j = 1``, an exact int64;
* the columns are ordered by ascending ``|llr|`` (NaN as +inf, ties by ascending index); the pivots S are the columns independent of the ones
  before them, and T holds the other ``n - rank`` columns in the same order;
* a candidate is a correction c with ``H c = s + H hard``, fixed by its non-pivot part ``t``: candidate 0 is ``t = {}`` (OSD-0), then
  ``t = {T[i]}`` for EVERY non-pivot column, then the pairs ``{T[a], T[b]}``, ``a < b < order``, in lexicographic order;
* the candidate of least ``W(hard ^ c)`` is returned, the earlier one on ties (OSD-0 wins every tie);
* a syndrome whose ``s + H hard`` is outside the column space gets exactly OSD-0's answer.

``flips`` (int32[B, 2]) names the winner's non-pivot columns, padded with -1; (-1, -1) means the OSD-0 answer was kept.  The C ABI is
``qldpc_osdcs_batch`` in ``include/qldpc_hip.h``; ``tests/osd_cs_model.py`` is the numpy model the kernel is tested against.
"""
import numpy as np

from .. import _lib
from .relay import _csr


class OsdCsDecoder:
    """OSD-CS post-processor of one parity-check matrix and weight vector.  ``decode(syndromes, llr, hard)`` returns
    ``(solution int8[B, n], flips int32[B, 2])`` (one shot in, one shot out)."""

    def __init__(self, H, weights, order=7, device=0):
        indptr, indices, n = _csr(H)
        self.weights = _lib.f64(weights).reshape(-1)
        if self.weights.size != n:
            raise ValueError(f"weights has {self.weights.size} entries, H has {n} columns")
        if not np.isfinite(self.weights).all():
            raise ValueError("weights must be finite")
        self.order = int(order)
        if not 0 <= self.order <= _lib.OSDCS_MAX_ORDER:
            raise ValueError(f"order must be in 0..{_lib.OSDCS_MAX_ORDER}, got {order}")
        self.graph = _lib.Graph(indptr, indices, n, device=device)

    def decode(self, syndromes, llr, hard):
        syndromes = np.asarray(syndromes, dtype=np.int8)
        single = syndromes.ndim == 1
        n = self.graph.n
        sol, flips = _lib.osdcs_batch(self.graph, syndromes.reshape(-1, self.graph.m), np.asarray(llr, np.float64).reshape(-1, n),
                                      np.asarray(hard, np.int8).reshape(-1, n), self.weights, self.order)
        return (sol[0], flips[0]) if single else (sol, flips)


def osd_cs_decode(H, syndromes, llr, hard, weights, order=7, device=0):
    """One-shot form of ``OsdCsDecoder(H, weights, order, device).decode(syndromes, llr, hard)``."""
    return OsdCsDecoder(H, weights, order=order, device=device).decode(syndromes, llr, hard)
