"""Numpy model of soft-readout noise and the soft-aware prior as include/qldpc_hip.h specifies them (qldpc_circuit_plan_use_soft_readout,
qldpc_soft_priors), built on the Philox of tests/relay_model.py alone: the tests pin the GPU kernels, and the host module
qldpc_amd/simulation/soft.py, to it bit for bit.  Written from the law, not from the package: it shares no code with either."""
import math

import numpy as np

from relay_model import philox4x32_10

FAULT_DOMAIN, PAULI_DOMAIN, READOUT_DOMAIN = 1, 2, 7
OP_CNOT, OP_PREP_X, OP_PREP_Z, OP_MEAS_X, OP_MEAS_Z, OP_IDLE = 1, 2, 3, 4, 5, 6
CNOT_COMP = np.array([1, 5, 4, 2, 10, 8, 3, 15, 12, 11, 7, 13, 14, 9, 6], np.int64)      # bit 0 / 1: X on slot 0 / 1, bit 2 / 3: Z on slot 0 / 1
IDLE_COMP = np.array([1, 5, 4], np.int64)
_M32 = np.uint64(0xFFFFFFFF)
TWO32 = 1 << 32


# ---------------------------------------------------------------------------------------- the channel
def cuts(flip_mass, keep_mass):
    """the 2K cuts (Python ints): floor(ldexp(S_b / S_last, 32)) of the running f64 sum, flipped bins first; the last is 2^32"""
    run, S = 0.0, []
    for w in list(flip_mass) + list(keep_mass):
        run = run + float(w)
        S.append(run)
    return [int(math.floor(math.ldexp(s / S[-1], 32))) for s in S[:-1]] + [TWO32]


def level_flip_probs(cut):
    """q[lv] from the integers; ZeroDivisionError for a level without mass"""
    K = len(cut) // 2
    w = [c - (cut[b - 1] if b else 0) for b, c in enumerate(cut)]
    return np.array([w[lv] / (w[lv] + w[K + lv]) for lv in range(K)])


def gaussian_masses(sigma, K, edges=None):
    """y ~ N(1, sigma^2), flipped iff y < 0, level = bin of |y|; an independent evaluation through the normal CDF Phi(x) = erfc(-x / sqrt 2) / 2"""
    e = [2.0 * lv / K for lv in range(K)] if edges is None else list(edges)
    e = e + [math.inf]

    def Phi(y):
        return 0.5 * math.erfc(-(y - 1.0) / (sigma * math.sqrt(2.0)))
    flip = [Phi(-e[lv]) - Phi(-e[lv + 1]) for lv in range(K)]
    keep = [Phi(e[lv + 1]) - Phi(e[lv]) for lv in range(K)]
    return flip, keep


# ---------------------------------------------------------------------------------------- the sampler
def threshold(p):
    """bernoulli_threshold of csrc/mc_common.h"""
    return 0 if p <= 0 else (0xFFFFFFFF if p >= 1 else int(np.floor(p * 4294967296.0)))


def _words(n, domain, seed, trial_begin, count):
    """uint64[count, n]: word l & 3 of Philox(g, l >> 2, domain)"""
    g = (np.uint64(trial_begin) + np.arange(count, dtype=np.uint64)).reshape(-1, 1)
    blk = np.arange((n + 3) // 4, dtype=np.uint64).reshape(1, -1)
    o = philox4x32_10(g & _M32, g >> np.uint64(32), blk, domain, int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    return np.stack(o, axis=2).reshape(count, -1)[:, :n].astype(np.uint64)


def _word0(b, l, domain, seed, trial_begin):
    g = np.uint64(trial_begin) + b.astype(np.uint64)
    return philox4x32_10(g & _M32, g >> np.uint64(32), l.astype(np.uint64), domain, int(seed) & 0xFFFFFFFF, int(seed) >> 32)[0].astype(np.int64)


def _dense(ptr, idx, logmask, n_det, k):
    """signature table -> (entries x n_det, entries x k) 0 / 1 matrices"""
    ptr, idx = np.asarray(ptr, np.int64), np.asarray(idx, np.int64)
    n = ptr.size - 1
    D = np.zeros((n, n_det), np.uint8)
    D[np.repeat(np.arange(n), np.diff(ptr)), idx] = 1
    lm = np.asarray(logmask, np.uint64).reshape(-1, 1)
    return D, ((lm >> np.arange(k, dtype=np.uint64).reshape(1, -1)) & np.uint64(1)).astype(np.uint8)


class SamplerModel:
    """sig_z / sig_x: (ptr, idx, logmask) of _lib.circuit_fault_signatures (entry 2 * location + slot); loc_type: the op code of every location."""

    def __init__(self, sig_z, sig_x, loc_type, n_det, k):
        self.loc_type = np.asarray(loc_type, np.int64)
        self.N, self.k = self.loc_type.size, k
        self.tabs = [_dense(*sig_z, n_det[0], k), _dense(*sig_x, n_det[1], k)]
        self.meas = np.flatnonzero((self.loc_type == OP_MEAS_X) | (self.loc_type == OP_MEAS_Z))          # ascending: entry k of the level record

    def _xor_in(self, out, b, l, comp):
        for s, (slot0, slot1) in enumerate(((4, 8), (1, 2))):                # sector Z takes the Z components, sector X the X components
            D, Lg = self.tabs[s]
            for bit, slot in ((slot0, 0), (slot1, 1)):
                on = (comp & bit) != 0
                np.bitwise_xor.at(out[2 * s], b[on], D[2 * l[on] + slot])
                np.bitwise_xor.at(out[2 * s + 1], b[on], Lg[2 * l[on] + slot])

    def sample(self, p, cut, seed, trial_begin, count):
        """-> (sparse_z, true_z, sparse_x, true_x int8, levels uint8[count, n_meas], flipped bool[count, n_meas]); cut None: the plain sampler"""
        out = [np.zeros((count, self.tabs[s][t].shape[1]), np.uint8) for s in range(2) for t in range(2)]
        ty = self.loc_type
        b, l = np.nonzero(_words(self.N, FAULT_DOMAIN, seed, trial_begin, count) < np.uint64(threshold(p)))
        r0 = _word0(b, l, PAULI_DOMAIN, seed, trial_begin)
        comp = np.where(ty[l] == OP_IDLE, IDLE_COMP[r0 % 3], CNOT_COMP[r0 % 15])
        comp = np.where((ty[l] == OP_MEAS_X) | (ty[l] == OP_PREP_X), 4, comp)
        comp = np.where((ty[l] == OP_MEAS_Z) | (ty[l] == OP_PREP_Z), 1, comp)
        self._xor_in(out, b, l, comp)
        levels = np.zeros((count, self.meas.size), np.uint8)
        flipped = np.zeros((count, self.meas.size), bool)
        if cut is not None:
            K = len(cut) // 2
            u = _words(self.N, READOUT_DOMAIN, seed, trial_begin, count)[:, self.meas]
            bins = sum((u >= np.uint64(c)).astype(np.int64) for c in cut[:2 * K - 1])       # 64-bit compares: a cut may be 2^32
            flipped = bins < K
            levels = np.where(flipped, bins, bins - K).astype(np.uint8)
            b, k = np.nonzero(flipped)
            l = self.meas[k]
            self._xor_in(out, b, l, np.where(ty[l] == OP_MEAS_X, 4, 1))
        return tuple(x.astype(np.int8) for x in out) + (levels, flipped)


# ---------------------------------------------------------------------------------------- the decoder tables and the prior rule
def columns_of(H, logmask):
    """{(frozenset of detectors, logical mask): column} of a dense 0 / 1 decoding matrix; of equal columns the first stands for all"""
    out = {}
    for j in range(H.shape[1]):
        out.setdefault((frozenset(np.flatnonzero(H[:, j]).tolist()), int(logmask[j])), j)
    return out


def prior_llrs(p):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.clip(np.nan_to_num(np.log((1 - p) / p)), -50, 50)


def build_tables(loc_type, sig, is_x, cols, n, channel_probs, cut):
    """-> dict(meas_col, meas_w, lut_ptr, lut, levels, unmatched) of one sector, by the law of include/qldpc_hip.h"""
    ptr, idx, lm = sig
    K, q = len(cut) // 2, level_flip_probs(cut)
    mine = OP_MEAS_Z if is_x else OP_MEAS_X
    meas_col, meas_w, unmatched = [], [], 0
    members = [[] for _ in range(n)]
    for i, op in enumerate(np.asarray(loc_type)):
        if op not in (OP_MEAS_X, OP_MEAS_Z):
            continue
        proj = (frozenset(int(v) for v in idx[ptr[2 * i]:ptr[2 * i + 1]]), int(lm[2 * i]))
        j = -1
        if op == mine and (proj[0] or proj[1]):
            j = cols.get(proj, -1)
            unmatched += j < 0
        meas_w.append(K ** len(members[j]) if j >= 0 else 1)
        if j >= 0:
            members[j].append(len(meas_col))
        meas_col.append(j)
    lut_ptr = np.concatenate([[0], np.cumsum([K ** len(m) for m in members])])
    lut = np.zeros(lut_ptr[-1])
    for j in range(n):
        c = len(members[j])
        if c == 0:
            lut[lut_ptr[j]] = prior_llrs(np.float64(channel_probs[j]))
            continue
        for I in range(K ** c):
            t = 1.0 - 2.0 * channel_probs[j]
            for r in range(c):
                t = t * (1.0 - 2.0 * q[(I // K ** r) % K])
            lut[lut_ptr[j] + I] = prior_llrs(np.float64((1.0 - t) / 2.0))
    return dict(meas_col=np.array(meas_col, np.int32), meas_w=np.array(meas_w, np.int32), lut_ptr=lut_ptr.astype(np.int32), lut=lut, levels=K,
                unmatched=unmatched)


def as_tuple(t):
    """tables as a dict (build_tables), an object with the attributes or the 5-tuple itself -> (meas_col, meas_w, lut_ptr, lut, levels)"""
    if isinstance(t, (tuple, list)):
        return tuple(np.asarray(x) for x in t[:4]) + (int(t[4]),)
    get = (lambda k: t[k]) if isinstance(t, dict) else (lambda k: getattr(t, k))
    return tuple(np.asarray(get(k)) for k in ("meas_col", "meas_w", "lut_ptr", "lut")) + (int(get("levels")),)


def priors(levels, tables):
    """uint8[B, n_meas] levels and one sector's tables -> f64[B, n]: lut[lut_ptr[j] + I_j], I_j = sum of level * weight over column j's measurements"""
    meas_col, meas_w, lut_ptr, lut, _ = as_tuple(tables)
    n = lut_ptr.size - 1
    on = meas_col >= 0
    out = np.zeros((levels.shape[0], n))
    for b in range(levels.shape[0]):
        I = np.zeros(n, np.int64)
        np.add.at(I, meas_col[on], levels[b, on].astype(np.int64) * meas_w[on])
        out[b] = lut[lut_ptr[:-1] + I]
    return out


def marginal_priors(channel_probs, meas_col, qbar):
    """the matched prior of a decoder that does not read the levels: p (+) qbar once per measurement of the column; verbatim without one"""
    p = np.asarray(channel_probs, np.float64)
    out = prior_llrs(p)
    c = np.bincount(meas_col[meas_col >= 0], minlength=p.size)
    for j in np.flatnonzero(c):
        t = 1.0 - 2.0 * p[j]
        for _ in range(c[j]):
            t = t * (1.0 - 2.0 * qbar)
        out[j] = prior_llrs(np.float64((1.0 - t) / 2.0))
    return out
