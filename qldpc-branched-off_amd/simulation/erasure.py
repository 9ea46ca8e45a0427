"""Decoder tables for heralded erasures (``CircuitPlan.use_erasure_aware``, ``_lib.erasure_priors``).  Host code, numpy only.

A circuit plan with erasure noise (``CircuitPlan.use_erasure_noise``) erases gate locations and reports which ones (the herald record); an erased
location is fully depolarised.  Given the herald, each column of a sector's decoding matrix that the location can flip is no longer a rare event:

  * a measurement, preparation or idle location flips its slot-0 projection with probability 1/2: one entry with ``h = INF`` (255);
  * a CNOT with projections ``a`` (control), ``b`` (target) and ``a ^ b`` (both) flips each non-empty one with probability 1/4 (the sixteen
    two-qubit Paulis project uniformly onto {none, a, b, a ^ b}): one entry with ``h = 1`` each, ``1 - 2q = 2**-1``;
  * where two of the three land on one column (``a == b``, or one of them is empty) that column flips with probability 1/2: a single ``INF`` entry.

Empty projections are dropped; a projection that no column of the decoding matrix holds is counted in ``.unmatched``.  The faults are enumerated as
``noise.builder._sector`` enumerates them, and a projection finds its column the way ``simulation.correlated`` finds it (``_view_columns``, ``_key``).

The per-shot prior of column ``j`` is 0.0 when one of its erased contributions is ``INF`` and else ``lut[lut_ptr[j] + H]``, ``H`` the number of its
erased ``h = 1`` contributions: ``lut[lut_ptr[j]]`` is the plan's own prior verbatim, entry ``H >= 1`` is ``prior_llrs((1 - (1 - 2 p_j) * 0.5**H) / 2)``
(independent flips compose by multiplying their ``1 - 2q``).  The law is stated in ``include/qldpc_hip.h`` at ``qldpc_erasure_priors``.
"""
import numpy as np

from .correlated import _key, _view_columns
from .engine import prior_llrs

H_INF = 255
GATES = ("CNOT", "PrepX", "PrepZ", "MeasX", "MeasZ", "IDLE")


def erasure_rates(rates):
    """rates: a number (every location class) or a dict keyed by the gate names ``GATES`` (a class left out: 0) -> f64[7] indexed by op code
    (noise/constants.py; entry 0 is unused).  ValueError for an unknown name or a rate outside [0, 1)."""
    from ..noise.constants import GATE_TO_OPCODE as OP
    out = np.zeros(7, np.float64)
    if isinstance(rates, dict):
        unknown = [g for g in rates if g not in GATES]
        if unknown:
            raise ValueError(f"unknown erasure location class(es): {sorted(map(str, unknown))} (expected {', '.join(GATES)})")
        for g, r in rates.items():
            out[OP[g]] = float(r)
    elif isinstance(rates, (bool, np.bool_)) or not isinstance(rates, (int, float, np.integer, np.floating)):
        raise ValueError(f"erasure rates must be a number or a dict keyed by gate name, got {rates!r}")
    else:
        out[1:] = float(rates)
    if not np.all((out >= 0) & (out < 1)):
        raise ValueError("erasure rates must be in [0, 1)")
    return out


class ErasureTables:
    """One sector's tables: loc_ptr int32[n_locs + 1], loc_col int32[entries] (ascending inside a location's run), loc_h uint8[entries] (1 or
    H_INF), lut_ptr int32[n + 1], lut f64[lut_ptr[n]].  ``unmatched``: projections no column holds."""

    def __init__(self, loc_ptr, loc_col, loc_h, lut_ptr, lut, unmatched=0):
        self.loc_ptr = np.ascontiguousarray(loc_ptr, np.int32)
        self.loc_col = np.ascontiguousarray(loc_col, np.int32)
        self.loc_h = np.ascontiguousarray(loc_h, np.uint8)
        self.lut_ptr = np.ascontiguousarray(lut_ptr, np.int32)
        self.lut = np.ascontiguousarray(lut, np.float64)
        self.unmatched = int(unmatched)
        if self.loc_ptr.ndim != 1 or self.loc_ptr.size < 1 or self.lut_ptr.ndim != 1 or self.lut_ptr.size < 2:
            raise ValueError("ErasureTables: loc_ptr must be int32[n_locs + 1] and lut_ptr int32[n + 1]")
        if self.loc_col.shape != self.loc_h.shape or self.loc_col.ndim != 1 or self.lut.ndim != 1:
            raise ValueError("ErasureTables: loc_col and loc_h hold one entry per contribution, lut is one array")

    n_locs = property(lambda self: int(self.loc_ptr.size - 1))
    n = property(lambda self: int(self.lut_ptr.size - 1))

    def contributions(self, l):
        """[(column, h)] of location l"""
        a, b = int(self.loc_ptr[l]), int(self.loc_ptr[l + 1])
        return [(int(c), int(h)) for c, h in zip(self.loc_col[a:b], self.loc_h[a:b])]


def location_projections(keys, cnot):
    """The (key, h) list of one erased location in one sector.  keys: its projections as _key(...) values, None for an empty one -- [slot 0] of a
    measurement, preparation or idle location, [a, b, a ^ b] of a CNOT.  A CNOT's projection that stands alone has h = 1; everything else is INF."""
    count = {}
    for k in keys:
        if k is not None:
            count[k] = count.get(k, 0) + 1
    return [(k, 1 if cnot and c == 1 else H_INF) for k, c in count.items()]


def tables_from_projections(per_location, cols, n, channel_probs, prior):
    """per_location: for every location the (key, h) list of location_projections; cols: _view_columns of the sector; channel_probs f64[n] (p_j);
    prior f64[n]: the plan's prior, which becomes lut[lut_ptr[j]] verbatim -> ErasureTables."""
    loc_ptr, loc_col, loc_h, unmatched = [0], [], [], 0
    c = np.zeros(n, np.int64)
    for entries in per_location:
        run = []
        for key, h in entries:
            j = cols.get(key)
            if j is None:
                unmatched += 1
                continue
            run.append((j, h))
        for j, h in sorted(run):
            loc_col.append(j)
            loc_h.append(h)
            c[j] += h == 1
        loc_ptr.append(len(loc_col))
    lut_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(c + 1, out=lut_ptr[1:])
    lut = np.zeros(int(lut_ptr[-1]), np.float64)
    p = np.asarray(channel_probs, np.float64)
    col = np.repeat(np.arange(n), c + 1)
    H = np.arange(lut.size) - lut_ptr[col]
    lut[:] = prior_llrs((1 - (1 - 2 * p[col]) * 0.5 ** H) / 2)
    lut[lut_ptr[:-1]] = np.asarray(prior, np.float64)
    return ErasureTables(loc_ptr, loc_col, loc_h, lut_ptr, lut, unmatched)


def _sector_projections(base_ops, sig, is_x):
    """The erased-location projections of one sector, enumerated as builder._sector enumerates its faults.  sig: (ptr, idx, logmask) of
    qldpc_circuit_fault_signatures, entry 2 * location + slot."""
    from ..noise.constants import GATE_TO_OPCODE as OP
    ptr, idx, lm = sig
    meas, prep = (OP["MeasZ"], OP["PrepZ"]) if is_x else (OP["MeasX"], OP["PrepX"])

    def s(e):
        return frozenset(int(v) for v in idx[ptr[e]:ptr[e + 1]]), int(lm[e])

    def key(x):
        return _key(sorted(x[0]), x[1])

    out = []
    for i, op in enumerate(np.asarray(base_ops)):
        if op == meas or op == prep or op == OP["IDLE"]:
            out.append(location_projections([key(s(2 * i))], False))
        elif op == OP["CNOT"]:
            a, b = s(2 * i), s(2 * i + 1)
            out.append(location_projections([key(a), key(b), key((a[0] ^ b[0], a[1] ^ b[1]))], True))
        else:
            out.append([])
    return out


def erasure_tables_from_circuit(compiled, Lx, Lz, matrices, signatures=None):
    """(ErasureTables of sector Z, ErasureTables of sector X) of a circuit-level plan whose decoding matrices are ``matrices`` (the dict of
    build_decoding_matrices / precomputed_matrices): p_j is its ``channel_probs``, the base entry ``prior_llrs`` of it (what run_simulation gives the
    plan).  signatures: ((ptr, idx, logmask) of sector Z, the same of sector X); None computes them on the device (_lib.circuit_fault_signatures),
    the only step here that is not host code."""
    from .. import _lib
    if signatures is None:
        signatures = (_lib.circuit_fault_signatures(compiled, Lx, Lz, False), _lib.circuit_fault_signatures(compiled, Lx, Lz, True))
    k = np.asarray(Lx).shape[0]
    base_ops = compiled.base_ops if hasattr(compiled, "base_ops") else compiled["base_ops"]
    out = []
    for is_x, s in enumerate(("Z", "X")):
        ip, ix, shape = _lib.canonical_csr(matrices[f"Hdec{s}"])
        n = int(shape[1])
        if f"H{s}_logical" in matrices:
            mask = _lib.logical_column_masks(matrices[f"H{s}_logical"], n)
        else:
            flr = int(matrices[f"first_logical_row{s}"])
            mask = _lib.logical_column_masks(np.asarray(matrices[f"H{s}_full"])[flr:flr + k], n)
        probs = np.asarray(matrices[f"channel_probs{s}"], np.float64)
        out.append(tables_from_projections(_sector_projections(base_ops, signatures[is_x], bool(is_x)), _view_columns(ip, ix, n, mask), n, probs,
                                           prior_llrs(probs)))
    return tuple(out)
