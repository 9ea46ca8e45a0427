"""Numpy model of the fixed-weight sampler as include/qldpc_hip.h specifies it (qldpc_circuit_plan_use_fixed_weight), built on the Philox of
tests/relay_model.py: the tests pin the GPU kernel to it bit for bit."""
import numpy as np

from relay_model import philox4x32_10

DOMAIN, PAULI_DOMAIN = 4, 2
_M32 = np.uint64(0xFFFFFFFF)
# component masks of csrc/sampler_common.h: bit0 = X on slot 0, bit1 = X on slot 1, bit2 = Z on slot 0, bit3 = Z on slot 1
CNOT_COMP = np.array([1, 5, 4, 2, 10, 8, 3, 15, 12, 11, 7, 13, 14, 9, 6], np.int64)
IDLE_COMP = np.array([1, 5, 4], np.int64)
OP_CNOT, OP_PREP_X, OP_PREP_Z, OP_MEAS_X, OP_MEAS_Z, OP_IDLE = 1, 2, 3, 4, 5, 6


def floyd_sets(N, w, seed, trial_begin, count):
    """int64[count, w]: the faulty set of trials trial_begin .. trial_begin + count - 1 in the order Floyd's algorithm adds its members.  Step i:
    j = N - w + i, t = (o_i * (j + 1)) >> 32 with o_i = word i & 3 of Philox(counter (lo g, hi g, i >> 2, 4), key seed); j if t is taken, else t."""
    N, w = int(N), int(w)
    assert 0 <= w <= N
    out = np.zeros((count, w), np.int64)
    if w == 0:
        return out
    g = (np.uint64(trial_begin) + np.arange(count, dtype=np.uint64)).reshape(-1, 1)
    blk = np.arange((w + 3) // 4, dtype=np.uint64).reshape(1, -1)
    o = philox4x32_10(g & _M32, g >> np.uint64(32), blk, DOMAIN, int(seed) & 0xFFFFFFFF, int(seed) >> 32)
    o = np.stack(o, axis=2).reshape(count, -1)[:, :w].astype(np.uint64)
    j = (N - w + np.arange(w)).astype(np.uint64)
    t = ((o * (j + np.uint64(1)).reshape(1, -1)) >> np.uint64(32)).astype(np.int64)
    for b in range(count):
        taken = set()
        row = t[b].tolist()
        for i in range(w):
            x = row[i]
            if x in taken:
                x = N - w + i
            assert x not in taken
            taken.add(x)
            out[b, i] = x
    return out


def floyd_set(N, w, seed, g):
    """The faulty set of trial g as a list, in the order of its steps."""
    return floyd_sets(N, w, seed, g, 1)[0].tolist()


def _dense(ptr, idx, logmask, n_det, k):
    """signature table -> (entries x n_det, entries x k) 0 / 1 matrices"""
    ptr, idx = np.asarray(ptr, np.int64), np.asarray(idx, np.int64)
    n = ptr.size - 1
    D = np.zeros((n, n_det), np.uint8)
    D[np.repeat(np.arange(n), np.diff(ptr)), idx] = 1
    lm = np.asarray(logmask, np.uint64).reshape(-1, 1)
    Lg = ((lm >> np.arange(max(k, 1), dtype=np.uint64).reshape(1, -1)) & np.uint64(1)).astype(np.uint8)[:, :k]
    return D, Lg


def _xor_rows(M, entries, on):
    """XOR over axis 1 of the rows M[entries] where `on` -> int8[count, columns]"""
    out = np.zeros((entries.shape[0], M.shape[1]), np.uint8)
    for b in range(entries.shape[0]):
        out[b] = np.bitwise_xor.reduce(M[entries[b][on[b]]], axis=0)
    return out.astype(np.int8)


class CircuitModel:
    """The circuit side: signatures (ptr, idx, logmask) of sector Z and X from _lib.circuit_fault_signatures (entry 2 * location + slot), the op type of
    every location, the detectors per sector and k.  sample() is what plan.sample returns under use_fixed_weight(w)."""

    def __init__(self, sig_z, sig_x, loc_type, n_det, k):
        self.loc_type = np.asarray(loc_type, np.int64)
        self.N = self.loc_type.size
        self.tabs = [_dense(*sig_z, n_det[0], k), _dense(*sig_x, n_det[1], k)]

    def components(self, members, seed, trial_begin):
        """the Pauli component mask of every member: fixed for measurements and preparations, else word 0 of Philox(g, l, domain 2) mod 3 / mod 15"""
        count = members.shape[0]
        g = (np.uint64(trial_begin) + np.arange(count, dtype=np.uint64)).reshape(-1, 1)
        r0 = philox4x32_10(g & _M32, g >> np.uint64(32), members.astype(np.uint64), PAULI_DOMAIN, int(seed) & 0xFFFFFFFF, int(seed) >> 32)[0].astype(np.int64)
        ty = self.loc_type[members]
        comp = np.where(ty == OP_IDLE, IDLE_COMP[r0 % 3], CNOT_COMP[r0 % 15])
        comp = np.where((ty == OP_MEAS_X) | (ty == OP_PREP_X), 4, comp)
        return np.where((ty == OP_MEAS_Z) | (ty == OP_PREP_Z), 1, comp)

    def sample(self, w, seed, trial_begin, count):
        members = floyd_sets(self.N, w, seed, trial_begin, count)
        comp = self.components(members, seed, trial_begin) if w else np.zeros((count, 0), np.int64)
        out = []
        for (D, Lg), b0, b1 in ((self.tabs[0], 4, 8), (self.tabs[1], 1, 2)):
            entries = np.concatenate([2 * members, 2 * members + 1], axis=1)
            on = np.concatenate([(comp & b0) != 0, (comp & b1) != 0], axis=1)
            out += [_xor_rows(D, entries, on), _xor_rows(Lg, entries, on)]
        return tuple(out)                                           # (sparse_z, true_z, sparse_x, true_x)


def sample_circuit(sig_z, sig_x, loc_type, n_det, k, w, seed, trial_begin, count):
    return CircuitModel(sig_z, sig_x, loc_type, n_det, k).sample(w, seed, trial_begin, count)


def sample_dem(dem, w, seed, trial_begin, count):
    """[(syndromes int8[count, n_det], true int8[count, k]) per sector] of a uniform qldpc_amd.simulation.dem.DetectorErrorModel at exactly w mechanisms."""
    members = floyd_sets(dem.n_mech, w, seed, trial_begin, count)
    on = np.ones(members.shape, bool)
    out = []
    for S in dem.sectors:
        D, Lg = _dense(S.det_ptr, S.det_idx, S.logmask, S.n_det, S.k)
        out.append((_xor_rows(D, members, on), _xor_rows(Lg, members, on)))
    return out


def uniform_tiny_dem(DetectorErrorModel, prob=0.1, n_sectors=2):
    """The column structure of dem_model.tiny_dem (37 mechanisms, two sectors with 37 and 5 detectors, k = (64, 3)) with one probability for all."""
    import dem_model as DM
    tiny = DM.tiny_dem(DetectorErrorModel)
    dem = DetectorErrorModel(np.full(tiny.n_mech, float(prob)), [tuple(S) for S in tiny.sectors])
    return dem if n_sectors == 2 else dem.sector(0)
