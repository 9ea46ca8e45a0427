"""Relay-BP (Mueller et al., "Improved belief propagation is sufficient for real-time decoding of quantum memory", 2025) on the GPU.

Normalised min-sum with a per-variable memory term, run in legs: leg 0 uses one memory strength ``gamma0``; every later leg draws new,
disordered strengths in ``[gamma_min, gamma_max]`` (Philox, a pure function of ``(seed, shot, tag, leg, column)``), starts from the previous
leg's marginals and counts a solution when it converges.  The lightest solution is returned; no OSD stage.  The algorithm and its
parameters are specified at ``qldpc_relay_decode_batch`` in ``include/qldpc_hip.h``; the defaults are ``_lib.RELAY_DEFAULTS``.
"""
import numpy as np

from .. import _lib


def _csr(H):
    """H dense, scipy sparse, or (indptr, indices, n) -> (indptr, indices, n)."""
    if isinstance(H, tuple) and len(H) == 3:
        indptr, indices, n = H
        return _lib.i32(indptr), _lib.i32(indices), int(n)
    indptr, indices, shape = _lib.canonical_csr(H)
    return indptr, indices, int(shape[1])


class RelayBPDecoder:
    """Relay-BP decoder of one parity-check matrix and prior.  ``decode`` returns
    ``(err int8[B, n], conv uint8[B], legs int32[B], iters int32[B], solutions int32[B])``."""

    def __init__(self, H, prior, tag=0, device=0, **params):
        self.params = _lib.relay_params(params)
        self.prior = _lib.f64(prior).reshape(-1)
        _lib.relay_check_inputs(self.prior, tag)
        self.tag = int(tag)
        indptr, indices, n = _csr(H)
        if self.prior.size != n:
            raise ValueError(f"prior has {self.prior.size} entries, H has {n} columns")
        self.graph = _lib.Graph(indptr, indices, n, device=device)

    def decode(self, syndromes, seed=0, shot_begin=0):
        syndromes = np.asarray(syndromes, dtype=np.int8)
        single = syndromes.ndim == 1
        out = _lib.relay_decode_batch(self.graph, syndromes.reshape(-1, self.graph.m), self.prior, seed, shot_begin, self.tag, **self.params)
        return tuple(o[0] for o in out) if single else out


def relay_bp_decode(H, syndromes, prior, seed=0, shot_begin=0, tag=0, **params):
    """One-shot form of ``RelayBPDecoder(H, prior, tag, **params).decode(syndromes, seed, shot_begin)``."""
    return RelayBPDecoder(H, prior, tag=tag, **params).decode(syndromes, seed=seed, shot_begin=shot_begin)
