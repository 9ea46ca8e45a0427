"""Sliding-window decoding of a space-time decoding matrix on the GPU.

The rows of a circuit-level decoding matrix come in layers of ``layer_rows`` rows (one layer per syndrome cycle) and every column has its rows
in one layer or in two consecutive ones.  The decoder works through the layers ``window`` at a time: it decodes the window's graph (the covered
rows, the columns that start inside them) with min-sum, sends a window that did not converge to OSD-0, commits the columns of the first
``commit`` layers, XORs what they explain out of the running syndrome and moves on by ``commit`` layers; the last window commits everything it
holds.  A window's graph does not grow with the number of cycles, so an experiment of any length runs on the kernels a ``window``-cycle
matrix takes.  With ``window`` >= the number of layers there is one window and the result is min-sum + OSD-0 on the whole matrix, bit for bit.

The semantics are specified at ``qldpc_window_decoder_create`` in ``include/qldpc_hip.h``; ``tests/window_model.py`` is the numpy model the
library is tested against.
"""
import numpy as np

from .. import _lib
from .relay import _csr


def column_layers(H, layer_rows):
    """(tau, span) per column of H: ``tau[j]`` = the first layer (``row // layer_rows``) column j has a row in and ``span[j]`` = last layer -
    first layer; a column without rows has ``tau = span = 0``.  A matrix is windowable when ``span.max() <= 1``."""
    indptr, indices, n = _csr(H)
    m = indptr.size - 1
    layer_rows = _lib.check_window_args(layer_rows, 1, 1, m)[0]
    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(indptr))
    first, last = np.full(n, m, np.int64), np.full(n, -1, np.int64)
    np.minimum.at(first, indices, rows)
    np.maximum.at(last, indices, rows)
    empty = last < 0
    tau = np.where(empty, 0, first // layer_rows)
    return tau, np.where(empty, 0, last // layer_rows - tau)


class SlidingWindowDecoder:
    """Sliding-window min-sum + OSD-0 decoder of one parity-check matrix and prior.  ``decode(syndromes)`` returns ``(err, info)``: ``err``
    int8[B, n] and ``info`` = dict of per-shot arrays ``conv`` (windows in which min-sum converged), ``iters`` (iterations summed over the
    windows), ``osd`` (windows sent to OSD-0), ``unsat`` (1 where ``H err != s``) and the scalar ``windows``.  One shot in, one shot out."""

    def __init__(self, H, prior, layer_rows, window, commit, max_iter=50, alpha_mode="dynamical", alpha=1.0, device=0):
        indptr, indices, n = _csr(H)
        m = indptr.size - 1
        self.layer_rows, self.window, self.commit = _lib.check_window_args(layer_rows, window, commit, m)
        self.prior = _lib.f64(prior).reshape(-1)
        if self.prior.size != n:
            raise ValueError(f"prior has {self.prior.size} entries, H has {n} columns")
        if not np.isfinite(self.prior).all():
            raise ValueError("sliding-window decoding needs a finite prior")
        _lib.alpha_args(alpha_mode, alpha)
        span = column_layers((indptr, indices, n), self.layer_rows)[1]
        if span.size and span.max() > 1:
            raise ValueError(f"column {int(np.flatnonzero(span > 1)[0])} has rows in more than two consecutive layers of {self.layer_rows} rows")
        self.graph = _lib.Graph(indptr, indices, n, device=device)
        self._dec = _lib.WindowDecoder(self.graph, self.layer_rows, self.window, self.commit, self.prior, max_iter=max_iter, alpha_mode=alpha_mode,
                                       alpha=alpha)

    def info(self):
        return self._dec.info()

    def decode(self, syndromes):
        syndromes = np.asarray(syndromes, dtype=np.int8)
        single = syndromes.ndim == 1
        err, conv, iters, osd, unsat = self._dec.decode(syndromes.reshape(-1, self.graph.m))
        info = dict(conv=conv, iters=iters, osd=osd, unsat=unsat, windows=self._dec.info()["windows"])
        if single:
            return err[0], {k: (v[0] if isinstance(v, np.ndarray) else v) for k, v in info.items()}
        return err, info
