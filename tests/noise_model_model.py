"""Numpy model of the per-class, biased Pauli noise of a circuit plan as include/qldpc_hip.h specifies it (qldpc_circuit_plan_use_noise_model), built on
the Philox draws, the threshold and the signature XOR of tests/erasure_model.py: the tests pin the GPU kernel, and the host module
qldpc_amd/simulation/noise_model.py, to it bit for bit.  Written from the law, not from the package: it shares no code with either."""
import math

import numpy as np

import erasure_model as EM
from erasure_model import FAULT_DOMAIN, PAULI_DOMAIN, _fires, _word0, rates_by_op, threshold
from fixed_weight_model import CNOT_COMP, IDLE_COMP, OP_CNOT, OP_IDLE, OP_MEAS_X, OP_MEAS_Z, OP_PREP_X, OP_PREP_Z


def thresholds(rates):
    """a number or {gate name: rate} -> uint64[7]: bernoulli_threshold of every class ([0] stays 0)"""
    return np.array([threshold(r) for r in rates_by_op(rates)], np.uint64)


def cuts(w):
    """K weights -> K - 1 Python ints: cut[i] = floor(ldexp(S_i / S_{K-1}, 32)), S the running f64 sum in index order"""
    S, run = [], 0.0
    for v in w:
        run = run + float(v)
        S.append(run)
    return [int(math.floor(math.ldexp(s / S[-1], 32))) for s in S[:-1]]


def choose(r, cut):
    """#{i : r >= cut[i]} for an int64 array of 32-bit words r (the compare in more than 32 bits: a cut may be 2**32)"""
    r = np.asarray(r, np.int64)
    return sum((r >= int(c)).astype(np.int64) for c in cut)


def pauli_index(ty, r0, idle_w, cnot_w):
    """the index into the component table of a faulty IDLE / CNOT (0 for the other classes): r % K without weights, the cut count with them"""
    r0 = np.asarray(r0, np.int64)
    idle = r0 % 3 if idle_w is None else choose(r0, cuts(idle_w))
    cnot = r0 % 15 if cnot_w is None else choose(r0, cuts(cnot_w))
    return np.where(ty == OP_IDLE, idle, np.where(ty == OP_CNOT, cnot, 0))


def components(ty, idx):
    comp = np.where(ty == OP_IDLE, IDLE_COMP[np.minimum(idx, 2)], CNOT_COMP[idx])
    comp = np.where((ty == OP_MEAS_X) | (ty == OP_PREP_X), 4, comp)
    return np.where((ty == OP_MEAS_Z) | (ty == OP_PREP_Z), 1, comp)


class SamplerModel(EM.SamplerModel):
    """erasure_model.SamplerModel's tables and signature XOR with the noise model's draws"""

    def draw(self, rates, idle_w, cnot_w, seed, trial_begin, count):
        """-> (b, l, idx): the faulty (trial, location) pairs and the Pauli index each drew"""
        thr = thresholds(rates)
        faulty = _fires(thr[self.loc_type], FAULT_DOMAIN, seed, trial_begin, count)
        b, l = np.nonzero(faulty)
        return b, l, pauli_index(self.loc_type[l], _word0(b, l, PAULI_DOMAIN, seed, trial_begin), idle_w, cnot_w)

    def sample_model(self, rates, idle_w, cnot_w, seed, trial_begin, count):
        """-> (sparse_z, true_z, sparse_x, true_x int8), and the draws (b, l, idx) they came from"""
        out = [np.zeros((count, self.tabs[s][t].shape[1]), np.uint8) for s in range(2) for t in range(2)]
        b, l, idx = self.draw(rates, idle_w, cnot_w, seed, trial_begin, count)
        self._xor_in(out, b, l, components(self.loc_type[l], idx))
        return tuple(x.astype(np.int8) for x in out), (b, l, idx)
