"""Min-sum with a prior that differs per shot, on the GPU: the front door for soft measurement information, heralded erasures or leakage, and any
re-weighting scheme.

Every other decoder here takes one prior for the whole batch.  ``ShotPriorMinSumDecoder.decode_batch(syndromes, priors)`` takes ``priors`` of shape
``[n]`` (shared) or ``[B, n]`` (one per shot): a shot whose qubit was heralded as erased passes a prior near 0 for its columns, a soft readout passes
the LLR it measured.  The decode is constant-alpha normalised min-sum, one round of guided decimation with nothing frozen; the law is stated at
``qldpc_shotprior_decode_batch`` in ``include/qldpc_hip.h`` and ``tests/correlated_model.py`` is the numpy model the kernel equals bit for bit.  The
outputs are the flooding decoder's (``err``, ``llr``, ``conv``, ``iters``), so OSD-0, OSD-CS and LSD take them unchanged.

``links`` / ``src_err`` are the reweighting step of two-pass correlated decoding (``simulation/correlated.py``): a link lowers the prior of its
column in the shots in which its source column is set in ``src_err``.
"""
import numpy as np

from .. import _lib
from .relay import _csr


class ShotPriorMinSumDecoder:
    """Constant-alpha min-sum decoder of one parity-check matrix whose prior comes with the call.  ``decode_batch(syndromes, priors)`` returns
    ``(err int8[B, n], llr f64[B, n], conv uint8[B], iters int32[B])``."""

    def __init__(self, H, alpha=1.0, clip_llr=20.0, max_iter=50, device=0):
        self.alpha, self.clip_llr, self.max_iter = _lib.shotprior_params(alpha, clip_llr, max_iter)
        indptr, indices, n = _csr(H)
        self.graph = _lib.Graph(indptr, indices, n, device=device)

    def decode_batch(self, syndromes, priors, links=None, src_err=None):
        """priors: f64[n] for every shot or f64[B, n] per shot, finite, any sign.  links (ptr, src, llr) with src_err int8[B, n_src]: see the module text."""
        syndromes = np.asarray(syndromes, dtype=np.int8)
        single = syndromes.ndim == 1
        priors = _lib.f64(priors)
        if not np.all(np.isfinite(priors)):
            raise ValueError("per-shot-prior min-sum needs finite priors")
        out = _lib.shotprior_decode_batch(self.graph, syndromes.reshape(-1, self.graph.m), priors, self.alpha, self.clip_llr, self.max_iter, links=links,
                                          src_err=src_err)
        return tuple(o[0] for o in out) if single else out
