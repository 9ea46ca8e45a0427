"""The soft-readout channel and its decoder tables (``CircuitPlan.use_soft_readout``, ``CircuitPlan.use_soft_aware``, ``_lib.soft_priors``).  Host code,
numpy and ``math`` only.

A circuit plan with soft readout (``CircuitPlan.use_soft_readout``) gives every MeasX / MeasZ location a readout on top of the plan's ordinary faults:
with probability ``flip_mass[lv] / S`` it lands on the wrong side at confidence level ``lv`` (and flips the measurement), with ``keep_mass[lv] / S`` on
the right side at level ``lv``.  The sampler reports the level only (the level record).  Given the level, the flip probability of that measurement is
``q[lv]`` -- small at a confident level, near 1/2 at an unconfident one -- and a decoder that reads the levels weighs every measurement by it.

The law (``include/qldpc_hip.h`` at ``qldpc_circuit_plan_use_soft_readout`` and ``qldpc_soft_priors``): the 2K masses, flipped bins first, become
integer cuts of the 32-bit word the sampler draws, and ``q`` and ``qbar`` are taken from the integers, so the decoder's belief is exactly the
sampler's law.  A measurement is its slot-0 projection of the sector's class (MeasX in sector Z, MeasZ in sector X); it finds its column the way
``simulation.erasure`` finds one (``_view_columns``, ``_key``).  Column ``j`` with measurements ``k_0 < ... < k_{c-1}`` has a run of ``K**c`` lut
entries, entry ``sum_r lv_r * K**r`` being ``prior_llrs((1 - t) / 2)`` with ``t = (1 - 2 p_j)`` multiplied by ``(1 - 2 q[lv_r])`` for r = 0, 1, ...
in that order (independent flips compose by multiplying their ``1 - 2q``).  A column without measurements keeps ``prior_llrs(p_j)`` verbatim.
"""
import math

import numpy as np

from .correlated import _key, _view_columns
from .engine import prior_llrs

MAX_LEVELS = 16
MAX_RUN = 65536
_TWO32 = 1 << 32


def _tail(x):
    """P(N(0, 1) > x) through erfc"""
    return 0.5 * math.erfc(x / math.sqrt(2.0))


class SoftReadout:
    """A readout channel with K = len(flip_mass) confidence levels.  ``cut`` (Python ints, 2K of them, the last 2**32), ``q`` f64[K] (the flip
    probability given the level) and ``qbar`` (the marginal flip rate) follow the law of include/qldpc_hip.h.  ValueError for K outside 1..16,
    masses of different lengths, a negative or non-finite mass, a sum of 0, and a level whose two integer masses are both 0."""

    def __init__(self, flip_mass, keep_mass):
        f, k = np.atleast_1d(np.asarray(flip_mass, np.float64)), np.atleast_1d(np.asarray(keep_mass, np.float64))
        if f.ndim != 1 or k.ndim != 1 or f.size != k.size:
            raise ValueError(f"SoftReadout: flip_mass and keep_mass must be two 1-D arrays of one length, got shapes {f.shape} and {k.shape}")
        K = int(f.size)
        if not 1 <= K <= MAX_LEVELS:
            raise ValueError(f"SoftReadout: {K} levels, outside 1..{MAX_LEVELS}")
        for name, w in (("flip_mass", f), ("keep_mass", k)):
            for i, v in enumerate(w):
                if not (math.isfinite(v) and v >= 0.0):
                    raise ValueError(f"SoftReadout: {name}[{i}] = {v} is negative or not finite")
        run, S = 0.0, []
        for v in list(f) + list(k):
            run += float(v)
            S.append(run)
        if not (S[-1] > 0.0 and math.isfinite(S[-1])):
            raise ValueError(f"SoftReadout: the masses sum to {S[-1]}: a readout channel needs a positive finite sum")
        cut = [int(math.floor(math.ldexp(s / S[-1], 32))) for s in S[:-1]] + [_TWO32]
        width = [c - (cut[b - 1] if b else 0) for b, c in enumerate(cut)]
        q = np.zeros(K, np.float64)
        for lv in range(K):
            if width[lv] + width[K + lv] == 0:
                raise ValueError(f"SoftReadout: level {lv} has no mass (flip_mass[{lv}] and keep_mass[{lv}] both come to 0 of 2**32)")
            q[lv] = width[lv] / (width[lv] + width[K + lv])
        self.flip_mass, self.keep_mass, self.levels, self.cut, self.q, self.qbar = f, k, K, cut, q, cut[K - 1] / _TWO32

    @classmethod
    def gaussian(cls, sigma, levels=8, edges=None):
        """A signal y ~ N(+1, sigma**2): flipped iff y < 0, the level is the bin of |y| between ``edges`` (``levels`` ascending values starting
        at 0; the last bin is open).  Default edges 2 * lv / levels: level 0 is the least confident."""
        K = int(levels)
        if not 1 <= K <= MAX_LEVELS:
            raise ValueError(f"SoftReadout.gaussian: {levels} levels, outside 1..{MAX_LEVELS}")
        if not (isinstance(sigma, (int, float, np.integer, np.floating)) and math.isfinite(sigma) and sigma > 0):
            raise ValueError(f"SoftReadout.gaussian: sigma = {sigma!r} must be a positive finite number")
        e = [2.0 * lv / K for lv in range(K)] if edges is None else [float(v) for v in edges]
        if len(e) != K or e[0] != 0.0 or any(not math.isfinite(v) for v in e) or any(b <= a for a, b in zip(e, e[1:])):
            raise ValueError(f"SoftReadout.gaussian: edges must be {K} finite ascending values starting at 0, got {e}")
        e.append(math.inf)
        flip = [_tail((e[lv] + 1.0) / sigma) - _tail((e[lv + 1] + 1.0) / sigma) for lv in range(K)]       # -e[lv + 1] < y <= -e[lv]
        keep = [_tail((e[lv] - 1.0) / sigma) - _tail((e[lv + 1] - 1.0) / sigma) for lv in range(K)]       #  e[lv] <= y < e[lv + 1]
        return cls(flip, keep)

    @classmethod
    def hard(cls, q):
        """One level: a classical flip with probability q that tells the decoder nothing (the control)."""
        if not (isinstance(q, (int, float, np.integer, np.floating)) and 0.0 <= q <= 1.0):
            raise ValueError(f"SoftReadout.hard: q = {q!r} must be in [0, 1]")
        return cls([float(q)], [1.0 - float(q)])

    def __repr__(self):
        return f"SoftReadout(levels={self.levels}, qbar={self.qbar:.6g})"


class SoftTables:
    """One sector's tables: meas_col int32[n_meas] (-1: no column of this sector), meas_w int32[n_meas] (levels**rank inside the column),
    lut_ptr int32[n + 1], lut f64[lut_ptr[n]], ``levels`` (K).  ``unmatched``: projections no column holds."""

    def __init__(self, meas_col, meas_w, lut_ptr, lut, levels, unmatched=0):
        self.meas_col = np.ascontiguousarray(meas_col, np.int32)
        self.meas_w = np.ascontiguousarray(meas_w, np.int32)
        self.lut_ptr = np.ascontiguousarray(lut_ptr, np.int32)
        self.lut = np.ascontiguousarray(lut, np.float64)
        self.levels, self.unmatched = int(levels), int(unmatched)
        if self.meas_col.ndim != 1 or self.meas_col.shape != self.meas_w.shape or self.lut_ptr.ndim != 1 or self.lut_ptr.size < 2 or self.lut.ndim != 1:
            raise ValueError("SoftTables: meas_col and meas_w must be int32[n_meas], lut_ptr int32[n + 1] and lut one array")

    n_meas = property(lambda self: int(self.meas_col.size))
    n = property(lambda self: int(self.lut_ptr.size - 1))

    def measurements(self, j):
        """the measurements of column j, ascending"""
        return np.flatnonzero(self.meas_col == j).tolist()


def tables_from_columns(meas_col, n, channel_probs, readout, unmatched=0):
    """meas_col: for every measurement the column of the sector it lands on (-1: none); channel_probs f64[n] (p_j) -> SoftTables.
    ValueError for a column whose run would pass 65536 entries."""
    K, q = readout.levels, readout.q
    meas_col = np.asarray(meas_col, np.int64)
    p = np.asarray(channel_probs, np.float64)
    c = np.zeros(n, np.int64)
    meas_w = np.ones(meas_col.size, np.int64)
    for k, j in enumerate(meas_col):
        if j < 0:
            continue
        meas_w[k] = K ** int(c[j])
        c[j] += 1
        if K ** int(c[j]) > MAX_RUN:
            raise ValueError(f"soft tables: column {j} has {int(c[j])} measurements: a run of {K}**{int(c[j])} entries is above {MAX_RUN}")
    lut_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(K ** c, out=lut_ptr[1:])
    lut = np.zeros(int(lut_ptr[-1]), np.float64)
    lut[lut_ptr[:-1]] = prior_llrs(p)                              # a run of length 1: the plain prior verbatim
    for j in np.flatnonzero(c):
        I = np.arange(K ** int(c[j]))
        t = np.full(I.size, 1.0 - 2.0 * p[j])
        for r in range(int(c[j])):
            t = t * (1.0 - 2.0 * q[(I // K ** r) % K])
        lut[lut_ptr[j]:lut_ptr[j + 1]] = prior_llrs((1.0 - t) / 2.0)
    return SoftTables(meas_col, meas_w, lut_ptr, lut, K, unmatched)


def _sector_measurements(base_ops, sig, is_x):
    """The key of every MeasX / MeasZ location in ascending location order, as erasure._sector_projections enumerates them: the slot-0 projection
    (entry 2 * location of qldpc_circuit_fault_signatures) where the location is of the sector's class, None where it is of the other class or the
    projection is empty."""
    from ..noise.constants import GATE_TO_OPCODE as OP
    ptr, idx, lm = sig
    mine = OP["MeasZ"] if is_x else OP["MeasX"]
    out = []
    for i, op in enumerate(np.asarray(base_ops)):
        if op == OP["MeasX"] or op == OP["MeasZ"]:
            out.append(_key(sorted(int(v) for v in idx[ptr[2 * i]:ptr[2 * i + 1]]), int(lm[2 * i])) if op == mine else None)
    return out


def _sector_view(matrices, s, k):
    from .. import _lib
    ip, ix, shape = _lib.canonical_csr(matrices[f"Hdec{s}"])
    n = int(shape[1])
    if f"H{s}_logical" in matrices:
        mask = _lib.logical_column_masks(matrices[f"H{s}_logical"], n)
    else:
        flr = int(matrices[f"first_logical_row{s}"])
        mask = _lib.logical_column_masks(np.asarray(matrices[f"H{s}_full"])[flr:flr + k], n)
    return _view_columns(ip, ix, n, mask), n


def soft_tables_from_circuit(compiled, Lx, Lz, matrices, readout, signatures=None):
    """(SoftTables of sector Z, SoftTables of sector X) of a circuit-level plan whose decoding matrices are ``matrices`` (the dict of
    build_decoding_matrices / precomputed_matrices): p_j is its ``channel_probs``.  signatures: ((ptr, idx, logmask) of sector Z, the same of
    sector X); None computes them on the device (_lib.circuit_fault_signatures), the only step here that is not host code."""
    from .. import _lib
    if signatures is None:
        signatures = (_lib.circuit_fault_signatures(compiled, Lx, Lz, False), _lib.circuit_fault_signatures(compiled, Lx, Lz, True))
    k = np.asarray(Lx).shape[0]
    base_ops = compiled.base_ops if hasattr(compiled, "base_ops") else compiled["base_ops"]
    out = []
    for is_x, s in enumerate(("Z", "X")):
        cols, n = _sector_view(matrices, s, k)
        meas_col, unmatched = [], 0
        for key in _sector_measurements(base_ops, signatures[is_x], bool(is_x)):
            j = cols.get(key) if key is not None else None
            unmatched += key is not None and j is None
            meas_col.append(-1 if j is None else j)
        out.append(tables_from_columns(meas_col, n, np.asarray(matrices[f"channel_probs{s}"], np.float64), readout, unmatched))
    return tuple(out)


def marginal_priors(matrices, tables, readout):
    """(prior of sector Z, prior of sector X), f64[n] each: the matched prior of a decoder that does not read the levels.  p_j becomes p_j (+) qbar
    once per contributing measurement -- t = (1 - 2 p_j) times (1 - 2 qbar) per measurement, (1 - t) / 2 -- and a column without measurements
    keeps ``prior_llrs(p_j)`` verbatim."""
    out = []
    for s, t in zip(("Z", "X"), tables):
        p = np.asarray(matrices[f"channel_probs{s}"], np.float64)
        c = np.bincount(t.meas_col[t.meas_col >= 0], minlength=t.n)
        prior = prior_llrs(p)
        tt = 1.0 - 2.0 * p
        for r in range(int(c.max()) if c.size else 0):
            tt = np.where(c > r, tt * (1.0 - 2.0 * readout.qbar), tt)
        prior[c > 0] = prior_llrs((1.0 - tt[c > 0]) / 2.0)
        out.append(prior)
    return tuple(out)
