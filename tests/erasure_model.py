"""Numpy model of heralded-erasure noise and the erasure-aware prior as include/qldpc_hip.h specifies them (qldpc_circuit_plan_use_erasure_noise,
qldpc_erasure_priors), built on the Philox of tests/relay_model.py and the signature tables of tests/fixed_weight_model.py: the tests pin the GPU
kernels, and the host module qldpc_amd/simulation/erasure.py, to it bit for bit.  Written from the law, not from the package: it shares no code with either."""
import numpy as np

from fixed_weight_model import CNOT_COMP, IDLE_COMP, OP_CNOT, OP_IDLE, OP_MEAS_X, OP_MEAS_Z, OP_PREP_X, OP_PREP_Z, _dense
from relay_model import philox4x32_10

FAULT_DOMAIN, PAULI_DOMAIN, ERASE_DOMAIN, ERASED_PAULI_DOMAIN = 1, 2, 5, 6
H_INF = 255
_M32 = np.uint64(0xFFFFFFFF)
GATE_OP = {"CNOT": OP_CNOT, "PrepX": OP_PREP_X, "PrepZ": OP_PREP_Z, "MeasX": OP_MEAS_X, "MeasZ": OP_MEAS_Z, "IDLE": OP_IDLE}
ERASED_IDLE = np.array([0, 1, 5, 4], np.int64)


def threshold(p):
    """bernoulli_threshold of csrc/mc_common.h"""
    return 0 if p <= 0 else (0xFFFFFFFF if p >= 1 else int(np.floor(p * 4294967296.0)))


def rates_by_op(rates):
    """a number (every class) or {gate name: rate} -> f64[7] by op code"""
    out = np.zeros(7)
    if isinstance(rates, dict):
        for g, r in rates.items():
            out[GATE_OP[g]] = r
    else:
        out[1:] = rates
    return out


def _fires(thr_of_loc, domain, seed, trial_begin, count):
    """bool[count, n_locs]: word l & 3 of Philox(g, l >> 2, domain) < thr_of_loc[l]"""
    n = thr_of_loc.size
    g = (np.uint64(trial_begin) + np.arange(count, dtype=np.uint64)).reshape(-1, 1)
    blk = np.arange((n + 3) // 4, dtype=np.uint64).reshape(1, -1)
    o = philox4x32_10(g & _M32, g >> np.uint64(32), blk, domain, int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    o = np.stack(o, axis=2).reshape(count, -1)[:, :n].astype(np.uint64)
    return o < thr_of_loc.astype(np.uint64).reshape(1, -1)


def _word0(b, l, domain, seed, trial_begin):
    """word 0 of Philox(g = trial_begin + b, l, domain) for paired index arrays"""
    g = np.uint64(trial_begin) + b.astype(np.uint64)
    return philox4x32_10(g & _M32, g >> np.uint64(32), l.astype(np.uint64), domain, int(seed) & 0xFFFFFFFF, int(seed) >> 32)[0].astype(np.int64)


def erased_components(ty, r0):
    comp = np.where(ty == OP_CNOT, r0 & 15, 0)
    comp = np.where(ty == OP_IDLE, ERASED_IDLE[r0 & 3], comp)
    comp = np.where((ty == OP_MEAS_X) | (ty == OP_PREP_X), np.where(r0 & 1, 4, 0), comp)
    return np.where((ty == OP_MEAS_Z) | (ty == OP_PREP_Z), np.where(r0 & 1, 1, 0), comp)


def fault_components(ty, r0):
    comp = np.where(ty == OP_IDLE, IDLE_COMP[r0 % 3], CNOT_COMP[r0 % 15])
    comp = np.where((ty == OP_MEAS_X) | (ty == OP_PREP_X), 4, comp)
    return np.where((ty == OP_MEAS_Z) | (ty == OP_PREP_Z), 1, comp)


def pack_heralds(erased):
    """bool[count, n_locs] -> uint32[count, ceil(n_locs / 32)], bit l & 31 of word l >> 5"""
    count, n = erased.shape
    nw = (n + 31) // 32
    pad = np.zeros((count, nw * 32), np.uint64)
    pad[:, :n] = erased
    return (pad.reshape(count, nw, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def unpack_heralds(words, n_locs):
    words = np.asarray(words, np.uint32)
    bits = (words[:, :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return bits.reshape(words.shape[0], -1)[:, :n_locs].astype(bool)


class SamplerModel:
    """sig_z / sig_x: (ptr, idx, logmask) of _lib.circuit_fault_signatures (entry 2 * location + slot); loc_type: the op code of every location."""

    def __init__(self, sig_z, sig_x, loc_type, n_det, k):
        self.loc_type = np.asarray(loc_type, np.int64)
        self.N, self.k = self.loc_type.size, k
        self.tabs = [_dense(*sig_z, n_det[0], k), _dense(*sig_x, n_det[1], k)]

    def _xor_in(self, out, b, l, comp):
        """XOR the signatures of the components `comp` of the (trial b, location l) pairs into out = [synd_z, true_z, synd_x, true_x]"""
        for s, (slot0, slot1) in enumerate(((4, 8), (1, 2))):                # sector Z takes the Z components, sector X the X components
            D, Lg = self.tabs[s]
            for bit, slot in ((slot0, 0), (slot1, 1)):
                on = (comp & bit) != 0
                np.bitwise_xor.at(out[2 * s], b[on], D[2 * l[on] + slot])
                np.bitwise_xor.at(out[2 * s + 1], b[on], Lg[2 * l[on] + slot])

    def sample(self, p, rates, seed, trial_begin, count):
        """-> (sparse_z, true_z, sparse_x, true_x int8, erased bool[count, n_locs]): the ordinary faults at p plus the erasures at rates (by op code)"""
        out = [np.zeros((count, self.tabs[s][t].shape[1]), np.uint8) for s in range(2) for t in range(2)]
        faulty = _fires(np.full(self.N, threshold(p)), FAULT_DOMAIN, seed, trial_begin, count)
        b, l = np.nonzero(faulty)
        self._xor_in(out, b, l, fault_components(self.loc_type[l], _word0(b, l, PAULI_DOMAIN, seed, trial_begin)))
        ethr = np.array([threshold(r) for r in rates_by_op(rates)], np.uint64)
        erased = _fires(ethr[self.loc_type], ERASE_DOMAIN, seed, trial_begin, count)
        b, l = np.nonzero(erased)
        self._xor_in(out, b, l, erased_components(self.loc_type[l], _word0(b, l, ERASED_PAULI_DOMAIN, seed, trial_begin)))
        return tuple(x.astype(np.int8) for x in out) + (erased,)


# ---------------------------------------------------------------------------------------- the decoder tables and the prior rule
def columns_of(H, logmask):
    """{(frozenset of detectors, logical mask): column} of a dense 0 / 1 decoding matrix; of equal columns the first stands for all"""
    out = {}
    for j in range(H.shape[1]):
        out.setdefault((frozenset(np.flatnonzero(H[:, j]).tolist()), int(logmask[j])), j)
    return out


def location_entries(op, is_x, a, b):
    """[(projection, h)] of one erased location in one sector; a / b: (frozenset of detectors, mask) of slot 0 / slot 1; empty projections dropped"""
    def empty(s):
        return not s[0] and not s[1]
    single = (OP_MEAS_Z, OP_PREP_Z, OP_IDLE) if is_x else (OP_MEAS_X, OP_PREP_X, OP_IDLE)
    if op in single:
        return [] if empty(a) else [(a, H_INF)]
    if op != OP_CNOT:
        return []
    ab = (a[0] ^ b[0], a[1] ^ b[1])
    seen = [s for s in (a, b, ab) if not empty(s)]
    return [(s, H_INF if seen.count(s) == 2 else 1) for s in dict.fromkeys(seen)]


def prior_llrs(p):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.clip(np.nan_to_num(np.log((1 - p) / p)), -50, 50)


def build_tables(loc_type, sig, is_x, cols, n, channel_probs, prior):
    """-> dict(loc_ptr, loc_col, loc_h, lut_ptr, lut, unmatched) of one sector, by the law of include/qldpc_hip.h"""
    ptr, idx, lm = sig

    def s(e):
        return frozenset(int(v) for v in idx[ptr[e]:ptr[e + 1]]), int(lm[e])

    loc_ptr, loc_col, loc_h, unmatched = [0], [], [], 0
    c = np.zeros(n, np.int64)
    for i, op in enumerate(np.asarray(loc_type)):
        run = []
        for proj, h in location_entries(int(op), is_x, s(2 * i), s(2 * i + 1)):
            if proj in cols:
                run.append((cols[proj], h))
            else:
                unmatched += 1
        for j, h in sorted(run):
            loc_col.append(j)
            loc_h.append(h)
            c[j] += h == 1
        loc_ptr.append(len(loc_col))
    lut_ptr = np.concatenate([[0], np.cumsum(c + 1)])
    lut = np.zeros(lut_ptr[-1])
    for j in range(n):
        lut[lut_ptr[j]] = prior[j]
        H = np.arange(1, c[j] + 1)
        lut[lut_ptr[j] + 1:lut_ptr[j + 1]] = prior_llrs((1 - (1 - 2 * channel_probs[j]) * 0.5 ** H) / 2)
    return dict(loc_ptr=np.array(loc_ptr, np.int32), loc_col=np.array(loc_col, np.int32), loc_h=np.array(loc_h, np.uint8),
                lut_ptr=lut_ptr.astype(np.int32), lut=lut, unmatched=unmatched)


def as_tuple(t):
    """tables as a dict (build_tables), an object with the five attributes or the 5-tuple itself -> the 5-tuple of arrays"""
    if isinstance(t, (tuple, list)):
        return tuple(np.asarray(x) for x in t)
    get =(lambda k: t[k]) if isinstance(t, dict) else (lambda k: getattr(t, k))
    return tuple(np.asarray(get(k)) for k in ("loc_ptr", "loc_col", "loc_h", "lut_ptr", "lut"))


def priors(erased, tables):
    """bool[B, n_locs] heralds and one sector's tables -> f64[B, n]: 0.0 under an erased INF contribution, else lut[lut_ptr[j] + H]"""
    loc_ptr, loc_col, loc_h, lut_ptr, lut = as_tuple(tables)
    n = lut_ptr.size - 1
    out = np.zeros((erased.shape[0], n))
    for b in range(erased.shape[0]):
        H, inf = np.zeros(n, np.int64), np.zeros(n, bool)
        for l in np.flatnonzero(erased[b]):
            col, h = loc_col[loc_ptr[l]:loc_ptr[l + 1]], loc_h[loc_ptr[l]:loc_ptr[l + 1]]
            inf[col[h == H_INF]] = True
            np.add.at(H, col[h != H_INF], h[h != H_INF].astype(np.int64))
        out[b] = np.where(inf, 0.0, lut[lut_ptr[:-1] + H])
    return out
