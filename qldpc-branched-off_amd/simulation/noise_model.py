"""Per-class, biased Pauli noise for circuit plans (``CircuitPlan.use_noise_model``) and the decoder priors that match it.  Host code, numpy only.

A circuit plan's own sampler fires every fault location at one rate ``p`` and draws a faulty IDLE's Pauli uniformly from X, Y, Z and a faulty CNOT's
uniformly from the fifteen two-qubit Paulis.  A ``NoiseModel`` gives each of the six location classes (CNOT, PrepX, PrepZ, MeasX, MeasZ, IDLE) a rate
of its own and, optionally, the three IDLE Paulis and the fifteen CNOT Paulis weights of their own.  The sampling law is stated in
``include/qldpc_hip.h`` at ``qldpc_circuit_plan_use_noise_model``: a weight table becomes K - 1 integer cuts of the 32-bit random word (``cuts``).

The decoding matrices do not depend on the rates: a column is a (detectors, logicals) signature, and the same faults exist under every model.  What
changes is each column's probability.  ``channel_probs`` enumerates the faults exactly as ``noise.builder._sector`` does, finds each fault's column the
way ``simulation.erasure`` and ``simulation.correlated`` find it (``_view_columns``, ``_key``) and sums the masses per column in enumeration order:

  * a measurement or preparation fault has mass ``rate[class]``;
  * a projection of an IDLE or CNOT has mass ``rate * wsum / wtotal``, evaluated left to right, with ``wsum`` the sum (in table index order) of the
    weights of the Paulis that have this projection and ``wtotal`` the sum of all weights; a table that is None counts 1.0 per Pauli.

With every rate ``p`` and no weights these are the builder's ``p``, ``p * 2 / 3`` and ``p * 4 / 15`` -- the same expressions -- so ``uniform(p)``
reproduces ``channel_probsZ`` / ``channel_probsX`` of matrices built at ``p`` bit for bit.

``prior_llrs`` floors the probabilities at 1e-12 first.  A class at rate 0 (or a Pauli at weight 0) can leave a column with zero mass; the column
stays in the matrix with a large finite prior (about 27.6) instead of being removed or given an infinite one.  That is a design choice, not a
measurement: the plan's buffers, the OSD stage and every recorded layout keep the shape of the matrices, and a finite prior keeps every kernel's
"clean input" form.
"""
import ctypes as C

import numpy as np

from .correlated import _key, _view_columns
from .engine import prior_llrs as _prior_llrs
from .erasure import GATES

PRIOR_FLOOR = 1e-12
# component masks of the Paulis in table order (csrc/sampler_common.h: bit 0 = X on slot 0, bit 1 = X on slot 1, bit 2 = Z on slot 0, bit 3 = Z on slot 1)
IDLE_COMP = (1, 5, 4)                                                    # X, Y, Z
CNOT_COMP = (1, 5, 4, 2, 10, 8, 3, 15, 12, 11, 7, 13, 14, 9, 6)          # the order of noise/kernels.py:283-343


def model_rates(rates):
    """rates: a number (every location class) or a dict keyed by the gate names ``GATES`` (a class left out: 0) -> f64[7] indexed by op code
    (noise/constants.py; entry 0 is unused).  ValueError for an unknown name or a rate outside [0, 1).  The conventions of erasure.erasure_rates."""
    from ..noise.constants import GATE_TO_OPCODE as OP
    out = np.zeros(7, np.float64)
    if isinstance(rates, dict):
        unknown = [g for g in rates if g not in GATES]
        if unknown:
            raise ValueError(f"unknown noise-model location class(es): {sorted(map(str, unknown))} (expected {', '.join(GATES)})")
        for g, r in rates.items():
            out[OP[g]] = float(r)
    elif isinstance(rates, (bool, np.bool_)) or not isinstance(rates, (int, float, np.integer, np.floating)):
        raise ValueError(f"noise-model rates must be a number or a dict keyed by gate name, got {rates!r}")
    else:
        out[1:] = float(rates)
    if not np.all((out >= 0) & (out < 1)):
        raise ValueError("noise-model rates must be in [0, 1)")
    return out


def _weights(w, K, name):
    if w is None:
        return None
    w = np.array(w, np.float64).ravel()
    if w.size != K:
        raise ValueError(f"{name} needs {K} weights, got {w.size}")
    if not np.all(np.isfinite(w) & (w >= 0)):
        raise ValueError(f"{name} must be finite and >= 0")
    if not w.sum() > 0:
        raise ValueError(f"{name} sum to 0: at least one weight must be positive")
    return w


def weight_cuts(w):
    """uint64[K - 1]: cut[i] = floor(ldexp(S_i / S_{K-1}, 32)) with S_i the running f64 sum w_0 + ... + w_i in index order.  A faulty location whose
    random word is r takes Pauli #{i : r >= cut[i]}; a cut may be 2**32."""
    S, run = [], 0.0
    for v in np.asarray(w, np.float64):
        run = run + float(v)
        S.append(run)
    return np.array([int(np.floor(np.ldexp(s / S[-1], 32))) for s in S[:-1]], np.uint64)


class NoiseModel:
    """rates: a number or {gate name: rate} (model_rates); idle_weights: None (uniform: the plan's own r % 3) or the weights of X, Y, Z on a faulty
    IDLE; cnot_weights: None (r % 15) or the weights of the fifteen Paulis of a faulty CNOT in the order of noise/kernels.py:283-343 (``CNOT_COMP``)."""

    def __init__(self, rates, idle_weights=None, cnot_weights=None):
        self.rates = model_rates(rates)
        self.idle_weights = _weights(idle_weights, 3, "idle_weights")
        self.cnot_weights = _weights(cnot_weights, 15, "cnot_weights")

    @classmethod
    def uniform(cls, p):
        """Every class at rate p, uniform Paulis: the plan's own noise at p (bit for bit when p is the plan's)."""
        return cls(p)

    @classmethod
    def si1000(cls, p):
        """The SI1000 (superconducting-inspired) ratios mapped onto this circuit's six classes: CNOT p, preparations 2p, measurements 5p, IDLE p / 10,
        uniform Paulis.  (SI1000 distinguishes further cases -- idling during measurement, single-qubit gates -- that this circuit does not have.)"""
        p = float(p)
        return cls({"CNOT": p, "PrepX": 2 * p, "PrepZ": 2 * p, "MeasX": 5 * p, "MeasZ": 5 * p, "IDLE": p / 10})

    @classmethod
    def biased(cls, p, eta):
        """Every class at rate p, idle Paulis X : Y : Z = 1 : 1 : 2 eta (eta = 0.5 is unbiased, large eta is Z-biased), CNOT Paulis uniform."""
        eta = float(eta)
        if not (np.isfinite(eta) and eta >= 0):
            raise ValueError(f"eta must be finite and >= 0, got {eta!r}")
        return cls(p, idle_weights=(1.0, 1.0, 2.0 * eta))

    def rates_by_op(self):
        """f64[7] by op code (entry 0 unused)"""
        return self.rates.copy()

    def cuts(self):
        """(idle cuts uint64[2] or None, CNOT cuts uint64[14] or None): weight_cuts of each table"""
        return (None if self.idle_weights is None else weight_cuts(self.idle_weights), None if self.cnot_weights is None else weight_cuts(self.cnot_weights))

    def as_struct(self):
        """(NoiseModelStruct, keep-alive): what qldpc_circuit_plan_use_noise_model takes"""
        from .._lib import NoiseModelStruct
        s = NoiseModelStruct()
        keep = [None if w is None else np.ascontiguousarray(w, np.float64) for w in (self.idle_weights, self.cnot_weights)]
        for i in range(7):
            s.rate[i] = float(self.rates[i])
        s.idle_w = keep[0].ctypes.data_as(C.POINTER(C.c_double)) if keep[0] is not None else None
        s.cnot_w = keep[1].ctypes.data_as(C.POINTER(C.c_double)) if keep[1] is not None else None
        return s, keep

    def __repr__(self):
        body = ", ".join(f"{g}={self.rates[i + 1]:g}" for i, g in enumerate(GATES))
        for name, w in (("idle_weights", self.idle_weights), ("cnot_weights", self.cnot_weights)):
            if w is not None:
                body += f", {name}={w.tolist()}"
        return f"NoiseModel({body})"

    # ------------------------------------------------------------------------------------ the matched priors
    def _projection_masses(self, op, is_x):
        """The masses of the projections of one location of op code `op` onto a sector, in builder._sector's order: [slot 0] of a measurement,
        preparation (of this sector) or IDLE, [control, target, both] of a CNOT, [] of anything else."""
        from ..noise.constants import GATE_TO_OPCODE as OP
        meas, prep = (OP["MeasZ"], OP["PrepZ"]) if is_x else (OP["MeasX"], OP["PrepX"])
        rate = float(self.rates[op]) if 1 <= op <= 6 else 0.0
        shift = 0 if is_x else 2                                         # sector X sees the X components (bits 0, 1), sector Z the Z components (bits 2, 3)
        if op == meas or op == prep:
            return [rate]
        if op == OP["IDLE"]:
            comps, w = IDLE_COMP, self.idle_weights
            wanted = (1,)
        elif op == OP["CNOT"]:
            comps, w = CNOT_COMP, self.cnot_weights
            wanted = (1, 2, 3)                                           # slot 0 alone, slot 1 alone, both
        else:
            return []
        w = [1.0] * len(comps) if w is None else [float(v) for v in w]
        wtotal = 0.0
        for v in w:
            wtotal = wtotal + v
        out = []
        for proj in wanted:
            wsum = 0.0
            for c, v in zip(comps, w):
                if (c >> shift) & 3 == proj:
                    wsum = wsum + v
            out.append(rate * wsum / wtotal)
        return out

    def channel_probs(self, compiled, Lx, Lz, M, signatures=None):
        """(probsZ f64[n_z], probsX f64[n_x]) aligned with the columns of the decoding matrices ``M`` (the dict of build_decoding_matrices /
        precomputed_matrices): the rule of the module text.  signatures: ((ptr, idx, logmask) of sector Z, the same of sector X); None computes
        them on the device (_lib.circuit_fault_signatures), the only step here that is not host code.  A fault whose projection no column holds
        is skipped (there is none for matrices built from this circuit)."""
        return self._channel_probs(compiled, Lx, Lz, M, signatures)[:2]

    def _channel_probs(self, compiled, Lx, Lz, M, signatures=None):
        """channel_probs plus, third, the number of skipped faults per sector (the tests and the probe check that it is 0)"""
        from .. import _lib
        if signatures is None:
            signatures = (_lib.circuit_fault_signatures(compiled, Lx, Lz, False), _lib.circuit_fault_signatures(compiled, Lx, Lz, True))
        k = np.asarray(Lx).shape[0]
        base_ops = np.asarray(compiled.base_ops if hasattr(compiled, "base_ops") else compiled["base_ops"])
        out, unmatched = [], []
        for is_x, s in enumerate(("Z", "X")):
            ip, ix, shape = _lib.canonical_csr(M[f"Hdec{s}"])
            n = int(shape[1])
            if f"H{s}_logical" in M:
                mask = _lib.logical_column_masks(M[f"H{s}_logical"], n)
            else:
                flr = int(M[f"first_logical_row{s}"])
                mask = _lib.logical_column_masks(np.asarray(M[f"H{s}_full"])[flr:flr + k], n)
            cols = _view_columns(ip, ix, n, mask)
            ptr, idx, lm = signatures[is_x]
            empty = (np.zeros(0, np.int64).tobytes(), 0)                 # the builder keeps a column for faults that flip nothing, if there are any

            def sig(e):
                return frozenset(int(v) for v in idx[ptr[e]:ptr[e + 1]]), int(lm[e])

            probs, miss = np.zeros(n, np.float64), 0
            for i, op in enumerate(base_ops):
                masses = self._projection_masses(int(op), bool(is_x))
                if not masses:
                    continue
                a = sig(2 * i)
                faults = [a]
                if len(masses) == 3:
                    b = sig(2 * i + 1)
                    faults = [a, b, (a[0] ^ b[0], a[1] ^ b[1])]
                for f, mass in zip(faults, masses):
                    key = _key(sorted(f[0]), f[1])
                    j = cols.get(empty if key is None else key)
                    if j is None:
                        miss += key is not None
                        continue
                    probs[j] = probs[j] + mass
            out.append(probs)
            unmatched.append(miss)
        return out[0], out[1], tuple(unmatched)

    def prior_llrs(self, compiled, Lx, Lz, M, signatures=None, floor=PRIOR_FLOOR):
        """(prior LLRs of sector Z, of sector X): engine.prior_llrs(maximum(channel_probs, floor)).  A column of zero mass keeps a large finite
        prior (the module text says why)."""
        pz, px = self.channel_probs(compiled, Lx, Lz, M, signatures)
        return _prior_llrs(np.maximum(pz, floor)), _prior_llrs(np.maximum(px, floor))
