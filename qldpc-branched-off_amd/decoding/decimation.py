"""BP with guided decimation (Yao, Laird, Gokduman, Pfister et al., "Belief propagation decoding of quantum LDPC codes with guided decimation",
2024) on the GPU.

Constant-alpha normalised min-sum in rounds of ``t_round`` iterations.  After a round that has not converged, the ``per_round`` most reliable
undecided columns (largest ``|V_j|``, ties to the lowest column) are frozen to their hard decision: their prior becomes ``+-fix_llr``, and the next
round starts from the marginals the last one left.  Freezing breaks the symmetric trapping sets that stall BP on degenerate quantum codes; it
needs no elimination and no random numbers.  The algorithm is specified at ``qldpc_decim_decode_batch`` in ``include/qldpc_hip.h``;
``tests/decimation_model.py`` is the numpy model the kernel is tested against.  The outputs include the flooding decoder's (``err``, ``llr``,
``conv``, ``iters``), so OSD-0 and OSD-CS take them unchanged.  The defaults are ``_lib.DECIM_DEFAULTS``.
"""
import numpy as np

from .. import _lib
from .relay import _csr


class DecimationDecoder:
    """Guided-decimation decoder of one parity-check matrix and prior.  ``decode(syndromes)`` returns
    ``(err int8[B, n], llr f64[B, n], conv uint8[B], iters int32[B], rounds int32[B], fixed int32[B])``."""

    def __init__(self, H, prior, device=0, **params):
        self.params = _lib.decim_params(params)
        self.prior = _lib.f64(prior).reshape(-1)
        if not np.all(np.isfinite(self.prior)):
            raise ValueError("guided decimation needs a finite prior")
        indptr, indices, n = _csr(H)
        if self.prior.size != n:
            raise ValueError(f"prior has {self.prior.size} entries, H has {n} columns")
        self.graph = _lib.Graph(indptr, indices, n, device=device)

    def decode(self, syndromes):
        syndromes = np.asarray(syndromes, dtype=np.int8)
        single = syndromes.ndim == 1
        out = _lib.decim_decode_batch(self.graph, syndromes.reshape(-1, self.graph.m), self.prior, **self.params)
        return tuple(o[0] for o in out) if single else out


def decimation_decode(H, syndromes, prior, **params):
    """One-shot form of ``DecimationDecoder(H, prior, **params).decode(syndromes)``."""
    return DecimationDecoder(H, prior, **params).decode(syndromes)
