"""Normalised min-sum (flooding schedule) in single precision on the GPU.

An opt-in fast mode: the algorithm of the f64 flooding decoder with damping 1, every floating-point operation one correctly rounded f32 operation
(priors, alphas and the clip are rounded to f32 first; subnormals are kept).  The f32 posteriors fit LDS where the f64 ones do not and several
workgroups share a CU.  Rounding is amplified by the iteration, so some shots -- mostly the hard decisions of shots that do not converge -- differ
from the f64 decoder's: the mode is validated statistically (logical error rates, ``tools/kbench_f32.py``) and f64 stays the default everywhere.

The semantics are specified at ``qldpc_minsum32_decoder_create`` in ``include/qldpc_hip.h``; ``tests/minsum32_model.py`` is the numpy model the
library is tested against bit for bit.  The outputs are those of the f64 decoder (``llr`` as f64, the f32 values widened), so OSD-0 and OSD-CS take
them unchanged.
"""
import numpy as np

from .. import _lib
from .relay import _csr


class SingleMinSumDecoder:
    """Single-precision min-sum decoder of one parity-check matrix (dense, scipy sparse or ``(indptr, indices, n)``) and prior.
    ``decode(syndromes)`` returns ``(err int8[B, n], conv uint8[B], llr f64[B, n], final_iter int32[B])``, one shot in, one shot out.
    ``.info`` is what the kernel runs: LDS bytes, threads per workgroup, resident workgroups per CU, clean-input form."""

    def __init__(self, H, prior, max_iter=50, alpha_mode="dynamical", alpha=1.0, clip_llr=20.0, device=0, flags=0):
        indptr, indices, n = _csr(H)
        max_iter, clip_llr = _lib.check_minsum32_args(max_iter, clip_llr)
        self.prior = _lib.f64(prior).reshape(-1)
        if self.prior.size != n:
            raise ValueError(f"prior has {self.prior.size} entries, H has {n} columns")
        _lib.alpha_args(alpha_mode, alpha)
        self.graph = _lib.Graph(indptr, indices, n, device=device)
        self._dec = _lib.Minsum32Decoder(self.graph, self.prior, max_iter=max_iter, alpha_mode=alpha_mode, alpha=alpha, clip_llr=clip_llr, flags=flags)
        self.info = self._dec.info()

    def decode(self, syndromes):
        syndromes = np.asarray(syndromes, dtype=np.int8)
        single = syndromes.ndim == 1
        out = self._dec.decode(syndromes.reshape(-1, self.graph.m))
        return tuple(o[0] for o in out) if single else out

    def close(self):
        self._dec.close()


def minsum32_decode(H, syndromes, prior, **kw):
    """One-shot form of ``SingleMinSumDecoder(H, prior, **kw).decode(syndromes)``."""
    dec = SingleMinSumDecoder(H, prior, **kw)
    try:
        return dec.decode(syndromes)
    finally:
        dec.close()
