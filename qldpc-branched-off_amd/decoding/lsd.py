"""BP+LSD: localized statistics decoding (Hillmann, Berent, Quintavalle, Eisert, Wille, Roffe, "Localized statistics decoding: a parallel decoding
algorithm for quantum low-density parity-check codes", 2024) on the GPU, as a post-processor of the OSD hand-over.

Where OSD eliminates the whole matrix, LSD grows clusters around the unsatisfied checks of ``s + H hard`` and solves each on its own small system.
Per shot, with H (m x n), the syndrome s, the BP posteriors ``llr`` and their hard decision ``hard``; the key of a column is
``(|llr_j| with NaN as +inf, j)``, the order of OSD-0:

* the seeds are the rows where ``b = s + H hard`` is one; each is a cluster of its own.  A cluster is the connected component of the cluster rows R
  and the added columns A, and it is valid once b restricted to it lies in the span of its columns;
* every round, each invalid cluster picks its ``bits_per_step`` smallest keys among the columns that touch it and are not in A; the picks of a round
  join A in ascending key order and their rows join R (clusters that meet merge);
* when every cluster is valid, the correction is the one on the pivots of A (the columns independent of the ones before them) and the solution is
  ``hard ^ c``;
* a shot whose clusters would hold more than ``max_rows`` rows (flag 1), or with an invalid cluster that no column outside A touches (flag 2: the
  residual is outside the reachable column space), gets exactly OSD-0's answer.

``info`` (int32[B, 4]) holds the flag, the rounds, ``|R|`` and ``|A|`` of a shot (the last three 0 when the flag is not 0).  With
``bits_per_step=1`` a flag-0 answer has been OSD-0's on every recorded circuit-level case; larger steps take fewer rounds and may differ.  The C ABI is
``qldpc_lsd_batch`` in ``include/qldpc_hip.h``; ``tests/lsd_model.py`` is the model the kernel is tested against.

``decode(..., return_stats=True)`` adds the statistics of the clusters a shot ends with (uint64[B, 8], ``_lib.LSD_STATS`` names the words: the number
of clusters, the 1-, squared 2- and infinity norm of their column counts and of their weights, the largest row count), the soft output of BP+LSD
(Lee et al., "Efficient post-selection for general quantum LDPC codes", 2025).  ``weights`` is uint16[n]; ``_lib.quantise_weights(prior)`` is the
default table.  A shot with flag 1 or 2 has eight words 2^64 - 1: no statement (``qldpc_lsd_stats_batch``; ``tests/lsd_stats_model.py``).
"""
import numpy as np

from .. import _lib
from .relay import _csr


class LsdDecoder:
    """BP+LSD post-processor of one parity-check matrix.  ``decode(syndromes, llr, hard)`` returns ``(solution int8[B, n], info int32[B, 4])``
    (one shot in, one shot out); with ``return_stats=True`` a third array, the cluster statistics uint64[B, 8] under ``weights`` (uint16[n] or None)."""

    def __init__(self, H, bits_per_step=1, max_rows=512, device=0):
        indptr, indices, n = _csr(H)
        p = _lib.lsd_params({"bits_per_step": bits_per_step, "max_rows": max_rows})
        self.bits_per_step, self.max_rows = p["bits_per_step"], p["max_rows"]
        self.graph = _lib.Graph(indptr, indices, n, device=device)

    def decode(self, syndromes, llr, hard, weights=None, return_stats=False):
        syndromes = np.asarray(syndromes, dtype=np.int8)
        single = syndromes.ndim == 1
        n = self.graph.n
        if weights is not None and not return_stats:
            raise ValueError("weights are for return_stats=True")
        if return_stats:
            out = _lib.lsd_stats_batch(self.graph, syndromes.reshape(-1, self.graph.m), np.asarray(llr, np.float64).reshape(-1, n),
                                       np.asarray(hard, np.int8).reshape(-1, n), self.bits_per_step, self.max_rows, weights)
            return tuple(a[0] for a in out) if single else out
        sol, info = _lib.lsd_batch(self.graph, syndromes.reshape(-1, self.graph.m), np.asarray(llr, np.float64).reshape(-1, n),
                                   np.asarray(hard, np.int8).reshape(-1, n), self.bits_per_step, self.max_rows)
        return (sol[0], info[0]) if single else (sol, info)


def lsd_decode(H, syndromes, llr, hard, bits_per_step=1, max_rows=512, device=0):
    """One-shot form of ``LsdDecoder(H, bits_per_step, max_rows, device).decode(syndromes, llr, hard)``."""
    return LsdDecoder(H, bits_per_step=bits_per_step, max_rows=max_rows, device=device).decode(syndromes, llr, hard)
