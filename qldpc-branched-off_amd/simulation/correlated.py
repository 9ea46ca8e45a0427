"""Link tables for two-pass correlated decoding (``CircuitPlan.use_correlated``, ``qldpc_circuit_plan_use_correlated``).  Host code, numpy only.

The two sectors of a plan are decoded one after the other, and the noise is not independent across them: a Y on an idle location, most of the
fifteen two-qubit Paulis on a CNOT, or a detector-error-model mechanism with detectors in both sectors flips both at once.  A LINK says: when
sector 0's correction uses column ``i``, column ``j`` of sector 1 is as likely as ``llr`` says.  The decoder lowers the prior of ``j`` to the
smallest such ``llr`` over the links whose source is in the correction (``include/qldpc_hip.h``: ``qldpc_shotprior_decode_batch``).

How a link is formed.  A mechanism (DEM) or a Pauli fault (circuit) maps to column ``i`` of sector 0 and column ``j`` of sector 1 when its
projection onto the sector -- (detectors, logical mask) -- equals that column's.  An empty projection has no column.  A projection that no column of
the view holds is skipped and counted in ``.unmatched``.  ``J[i, j]`` is the plain sum, in enumeration order, of the masses of everything that maps
to ``(i, j)``; ``P0[i]`` is the mass of everything mapping to ``i``; ``link_llr = prior_llrs(min(J / P0, 1))``: the probability of ``j`` given ``i``.

Two modes.  ``"raise"`` (the default): ``base`` is None, the decoder's own sector-1 prior stays underneath, so a column never becomes less likely than
the decoder thought.  ``"condition"``: ``base_j = prior_llrs(max(U_j, floor))`` with ``U_j`` the mass of what reaches column ``j`` without touching
sector 0 -- the conditional prior under "sector 0's correction is the truth".
"""
import numpy as np

from .engine import prior_llrs

MODES = ("raise", "condition")


class CorrelationLinks:
    """ptr int32[n1 + 1], src int32[links] (sector-0 columns, ascending inside a column's run), llr f64[links]; base f64[n1] or None (the plan's own
    sector-1 prior).  ``unmatched``: projections no column holds; ``n_src``: columns of sector 0."""

    def __init__(self, ptr, src, llr, base=None, unmatched=0, n_src=None):
        self.ptr = np.ascontiguousarray(ptr, np.int32)
        self.src = np.ascontiguousarray(src, np.int32)
        self.llr = np.ascontiguousarray(llr, np.float64)
        self.base = None if base is None else np.ascontiguousarray(base, np.float64)
        self.unmatched, self.n_src = int(unmatched), n_src
        if self.ptr.ndim != 1 or self.ptr.size < 1 or self.src.shape != self.llr.shape or self.src.ndim != 1 or int(self.ptr[-1]) != self.src.size:
            raise ValueError("CorrelationLinks: ptr must be int32[n + 1] ending at the number of links, src and llr one entry per link")
        if self.base is not None and self.base.shape != (self.ptr.size - 1,):
            raise ValueError("CorrelationLinks: base needs one entry per column")

    n_links = property(lambda self: int(self.src.size))
    n = property(lambda self: int(self.ptr.size - 1))

    def pairs(self):
        """[(sector-0 column, sector-1 column, llr)] in table order."""
        col = np.repeat(np.arange(self.n), np.diff(self.ptr))
        return [(int(i), int(j), float(v)) for i, j, v in zip(self.src, col, self.llr)]


def check_mode(mode, floor):
    if mode not in MODES:
        raise ValueError(f"Unsupported correlated mode: {mode!r} (expected 'raise' or 'condition')")
    if floor is not None and not (np.isfinite(floor) and 0 < floor < 1):
        raise ValueError("floor must be a probability in (0, 1)")


def _view_columns(indptr, indices, n, logmask):
    """{(detectors as bytes of int64, logical mask): column}; of equal columns the first stands for all."""
    indptr, indices = np.asarray(indptr, np.int64), np.asarray(indices, np.int64)
    rows = np.repeat(np.arange(indptr.size - 1, dtype=np.int64), np.diff(indptr))
    order = np.argsort(indices, kind="stable")
    colptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(indices, minlength=n), out=colptr[1:])
    rows = rows[order]
    out = {}
    for j in range(n):
        out.setdefault((rows[colptr[j]:colptr[j + 1]].tobytes(), int(logmask[j])), j)
    return out


def _key(dets, mask):
    dets = np.sort(np.asarray(dets, np.int64))
    return (dets.tobytes(), int(mask)) if dets.size or int(mask) else None


def links_from_events(events, cols0, cols1, n0, n1, P0, mode="raise", floor=None):
    """The rule of the module text on a list of (key0, key1, mass) in enumeration order; a key is _key(detectors, mask), None for an empty projection.
    cols0 / cols1: _view_columns of the two sectors.  P0: f64[n0], or None = the mass of everything mapping to each sector-0 column."""
    J, unmatched = {}, 0
    U, M0 = np.zeros(n1), np.zeros(n0)
    for k0, k1, mass in events:
        i = cols0.get(k0) if k0 is not None else None
        j = cols1.get(k1) if k1 is not None else None
        unmatched += (k0 is not None and i is None) + (k1 is not None and j is None)
        if i is not None:
            M0[i] = M0[i] + mass
        if j is None:
            continue
        if k0 is None:
            U[j] = U[j] + mass
        elif i is not None:
            J[(j, i)] = J.get((j, i), 0.0) + mass
    P0 = M0 if P0 is None else np.asarray(P0, np.float64)
    keys = sorted(J)                                               # by sector-1 column, then source ascending
    src = np.array([i for _, i in keys], np.int32)
    col = np.array([j for j, _ in keys], np.int64)
    mass = np.array([J[k] for k in keys], np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.minimum(mass / P0[src], 1.0) if len(keys) else np.zeros(0)
    ptr = np.zeros(n1 + 1, np.int32)
    np.cumsum(np.bincount(col, minlength=n1), out=ptr[1:])
    base = prior_llrs(np.maximum(U, floor)) if mode == "condition" else None
    return CorrelationLinks(ptr, src, prior_llrs(ratio), base, unmatched, n0)


def links_from_dem(dem, mode="raise", floor=None):
    """CorrelationLinks of a two-sector DetectorErrorModel: the masses are the mechanisms' probabilities, in mechanism order, and the columns those of
    ``dem.decoder_view(s)``.  floor (mode "condition"): default the smallest positive probability of the model."""
    check_mode(mode, floor)
    if dem.n_sectors != 2:
        raise ValueError("correlated decoding needs a detector error model with two sectors")
    views = [dem.decoder_view(s) for s in range(2)]
    cols = [_view_columns(v.indptr, v.indices, v.shape[1], v.logmask) for v in views]
    if floor is None:
        pos = dem.prob[dem.prob > 0]
        floor = float(pos.min()) if pos.size else 0.5
    events = []
    for l in np.flatnonzero(dem.prob > 0):
        (d0, m0), (d1, m1) = dem.mechanism(l, 0), dem.mechanism(l, 1)
        events.append((_key(d0, m0), _key(d1, m1), float(dem.prob[l])))
    return links_from_events(events, cols[0], cols[1], views[0].shape[1], views[1].shape[1], None, mode, floor)


def circuit_events(base_ops, sig_z, sig_x, error_rate):
    """The (key of the Z part, key of the X part, mass) list of a circuit's Pauli faults, location by location: what links_from_circuit enumerates.
    sig_*: (ptr, idx, logmask) of qldpc_circuit_fault_signatures, entry 2 * location + slot.  IDLE: Z, X and Y of slot 0, p / 3 each; CNOT: the
    fifteen products of a Z part and an X part in {none, slot 0, slot 1, both}, p / 15 each (composite signatures by XOR, as builder._sector
    forms them); a measurement or preparation flips its own sector only, with mass p."""
    from ..noise.constants import GATE_TO_OPCODE as OP

    def sigs(tab, l):
        ptr, idx, lm = tab
        a = (frozenset(int(v) for v in idx[ptr[2 * l]:ptr[2 * l + 1]]), int(lm[2 * l]))
        b = (frozenset(int(v) for v in idx[ptr[2 * l + 1]:ptr[2 * l + 2]]), int(lm[2 * l + 1]))
        return a, b, (a[0] ^ b[0], a[1] ^ b[1])

    def key(s):
        return _key(sorted(s[0]), s[1])

    events = []
    for l, op in enumerate(np.asarray(base_ops)):
        if op in (OP["MeasX"], OP["PrepX"]):
            events.append((key(sigs(sig_z, l)[0]), None, error_rate))
        elif op in (OP["MeasZ"], OP["PrepZ"]):
            events.append((None, key(sigs(sig_x, l)[0]), error_rate))
        elif op == OP["IDLE"]:
            z, x = key(sigs(sig_z, l)[0]), key(sigs(sig_x, l)[0])
            events += [(z, None, error_rate / 3), (None, x, error_rate / 3), (z, x, error_rate / 3)]
        elif op == OP["CNOT"]:
            zs, xs = [None] + [key(s) for s in sigs(sig_z, l)], [None] + [key(s) for s in sigs(sig_x, l)]
            events += [(z, x, error_rate / 15) for z in zs for x in xs if z is not None or x is not None]
    return events


def links_from_circuit(compiled, Lx, Lz, matrices, error_rate, mode="raise", floor=None, signatures=None):
    """CorrelationLinks of a circuit-level plan: the faults are those the circuit sampler draws (circuit_events), the columns those of the decoding
    matrices ``matrices`` (the dict of build_decoding_matrices / precomputed_matrices), and P0 is its ``channel_probsZ``.  floor (mode "condition"):
    default error_rate / 15.  signatures: ((ptr, idx, logmask) of sector Z, the same of sector X); None computes them on the device
    (_lib.circuit_fault_signatures), the only step here that is not host code."""
    check_mode(mode, floor)
    from .. import _lib
    if signatures is None:
        signatures = (_lib.circuit_fault_signatures(compiled, Lx, Lz, False), _lib.circuit_fault_signatures(compiled, Lx, Lz, True))
    k = np.asarray(Lx).shape[0]
    cols, ns = [], []
    for s in ("Z", "X"):
        ip, ix, shape = _lib.canonical_csr(matrices[f"Hdec{s}"])
        n = int(shape[1])
        if f"H{s}_logical" in matrices:
            mask = _lib.logical_column_masks(matrices[f"H{s}_logical"], n)
        else:
            flr = int(matrices[f"first_logical_row{s}"])
            mask = _lib.logical_column_masks(np.asarray(matrices[f"H{s}_full"])[flr:flr + k], n)
        cols.append(_view_columns(ip, ix, n, mask))
        ns.append(n)
    events = circuit_events(compiled.base_ops if hasattr(compiled, "base_ops") else compiled["base_ops"], signatures[0], signatures[1], float(error_rate))
    return links_from_events(events, cols[0], cols[1], ns[0], ns[1], np.asarray(matrices["channel_probsZ"], np.float64), mode,
                             float(error_rate) / 15 if floor is None else floor)
