"""Numpy model of min-sum with a per-shot prior and of the reweighting step of correlated two-sector decoding, as include/qldpc_hip.h specifies them
(qldpc_shotprior_decode_batch): the tests pin the GPU kernel (csrc/shot_prior.hip) to it bit for bit.

reweight is the per-shot prior, decode is one round of decimation_model with nothing frozen.  The byte counts below are a SECOND COPY of the host code
(leg_lds_prefix of bp_leg.h, shotprior_lds_bytes and shotprior_mode of shot_prior.hip), kept on purpose as an independent statement of the rule: the GPU
module sizes its families by searching these functions, never by a literal, and observes the accept / refuse line directly.  toy_dem is the smallest
model in which the links decide the verdict.  Plain module (no pytest hooks).
"""
import numpy as np

import decimation_model as DM

LDS_BYTES = 160 * 1024
LEG_ROW_DEG = 56


def reweight(prior, src_err, ptr, src, llr):
    """P[b][j] = min(prior[b][j], min of llr[l] over ptr[j] <= l < ptr[j + 1] with src_err[b][src[l]] == 1).  prior: [n] or [B, n] -> P f64[B, n]."""
    src_err = np.asarray(src_err)
    B, n = src_err.shape[0], len(ptr) - 1
    P = np.array(np.broadcast_to(np.asarray(prior, np.float64), (B, n)))
    for j in range(n):
        for l in range(int(ptr[j]), int(ptr[j + 1])):
            fired = src_err[:, int(src[l])] == 1
            P[fired, j] = np.minimum(P[fired, j], float(llr[l]))
    return P


def decode(indptr, indices, n, syndromes, P, alpha, clip_llr, max_iter):
    """Every shot with its own prior P[B, n] -> (err int8[B, n], llr f64[B, n], conv uint8[B], iters int32[B])."""
    tab = DM.Tables(indptr, indices, n)
    synd = (np.asarray(syndromes, np.int8).reshape(-1, tab.m) & 1).astype(bool)
    P = np.array(np.broadcast_to(np.asarray(P, np.float64), (synd.shape[0], n)))
    V = P.copy()
    with np.errstate(invalid="ignore"):
        conv, itc = DM.run_round(tab, synd, V, P, alpha, clip_llr, max_iter)
    return (V < 0.0).astype(np.int8), V, conv.astype(np.uint8), itc.astype(np.int32)


# ---------------------------------------------------------------------------------------- the storage rule, restated
def _up(x, a):
    return (x + a - 1) // a * a


def leg_lds_prefix(m, n, vg):
    """V[n] f64 (not in the global-memory form) | 16 bytes per check | 8 bytes per check"""
    off_p = 0 if vg else _up(8 * n, 16)
    return _up(off_p + 16 * m + 8 * m, 16)


def shotprior_lds_bytes(m, n, vg, p_lds):
    """the prefix | P[n] f64 when it lives in LDS | 16 bytes of flags"""
    return leg_lds_prefix(m, n, vg) + (_up(8 * n, 16) if p_lds else 0) + 16


def shotprior_mode(m, n, max_row_deg):
    """0: refused; where V / P live with link tables: 1 LDS / LDS, 2 LDS / global memory, 3 global / global."""
    if not (n < 65535 and max_row_deg < 256) or m <= 0 or n <= 0 or max_row_deg > LEG_ROW_DEG:      # graph.hip: the slot tables exist
        return 0
    if shotprior_lds_bytes(m, n, False, True) <= LDS_BYTES:
        return 1
    if shotprior_lds_bytes(m, n, False, False) <= LDS_BYTES:
        return 2
    return 3 if shotprior_lds_bytes(m, n, True, False) <= LDS_BYTES else 0


# ---------------------------------------------------------------------------------------- the toy model
TOY_MECHANISMS = ("A", "C", "D", "B", "E", "F")
TOY_COLUMNS = (("A", "C", "D"), ("A", "B", "E", "F"))         # the derived decoder views: columns in order of first appearance


def toy_dem():
    """Two sectors of two detectors.  Sector 0: A = {a0} p 0.01, C = {a0, a1} 0.02, D = {a1} 0.02.  Sector 1 (k = 1): A = {d0} flipping the observable,
    B = {d0} 0.03, E = {d0, d1} 0.02, F = {d1} 0.02.  A is the only mechanism in both sectors, and alone in sector 1 it loses to B."""
    from qldpc_amd.simulation.dem import DetectorErrorModel
    prob = [0.01, 0.02, 0.02, 0.03, 0.02, 0.02]
    columns = [[([0], 0), ([0], 1)],        # A
               [([0, 1], 0), ([], 0)],      # C
               [([1], 0), ([], 0)],         # D
               [([], 0), ([0], 0)],         # B
               [([], 0), ([0, 1], 0)],      # E
               [([], 0), ([1], 0)]]         # F
    return DetectorErrorModel.from_columns(prob, columns, (2, 2), (1, 1))


# ---------------------------------------------------------------------------------------- the links of a circuit, restated
def circuit_links(loc_type, sig_z, sig_x, cols_z, cols_x, n_x, probs_z, p, mode="raise", floor=None):
    """The rule of qldpc_amd/simulation/correlated.py's module text on a circuit, written a second time: -> (ptr int32[n_x + 1], src int32[links],
    llr f64[links], base f64[n_x] or None, unmatched).  loc_type: the op code of every location; sig_*: (ptr, idx, logmask), entry 2 * location +
    slot; cols_*: {(frozenset of detectors, logical mask): column} of the two decoding matrices (of equal columns the first).  The Pauli faults in
    location order -- a measurement or preparation: its own sector, mass p; an IDLE: Z, X, Y of slot 0, p / 3 each; a CNOT: every product of a Z
    part and an X part in (none, slot 0, slot 1, both) but the identity, p / 15 each -- map to the column that equals their projection; J[i, j] and
    U[j] are running f64 sums in that order; llr = prior_llrs(min(J / probs_z[i], 1)), sorted by X column, then Z column."""
    def parts(sig, l):
        ptr, idx, lm = sig
        a = (frozenset(int(v) for v in idx[ptr[2 * l]:ptr[2 * l + 1]]), int(lm[2 * l]))
        b = (frozenset(int(v) for v in idx[ptr[2 * l + 1]:ptr[2 * l + 2]]), int(lm[2 * l + 1]))
        return [None] + [s if (s[0] or s[1]) else None for s in (a, b, (a[0] ^ b[0], a[1] ^ b[1]))]

    def llrs(q):
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.clip(np.nan_to_num(np.log((1 - q) / q)), -50, 50)

    J, U, unmatched = {}, np.zeros(n_x), 0
    for l, op in enumerate(np.asarray(loc_type).tolist()):
        z, x = parts(sig_z, l), parts(sig_x, l)
        if op in (4, 2):                                                   # MeasX, PrepX
            faults = [(z[1], None, p)]
        elif op in (5, 3):                                                 # MeasZ, PrepZ
            faults = [(None, x[1], p)]
        elif op == 6:
            faults = [(z[1], None, p / 3), (None, x[1], p / 3), (z[1], x[1], p / 3)]
        elif op == 1:
            faults = [(a, b, p / 15) for ia, a in enumerate(z) for ib, b in enumerate(x) if ia or ib]
        else:
            faults = []
        for kz, kx, mass in faults:
            i = cols_z.get(kz) if kz is not None else None
            j = cols_x.get(kx) if kx is not None else None
            unmatched += (kz is not None and i is None) + (kx is not None and j is None)
            if j is None:
                continue
            if kz is None:
                U[j] = U[j] + mass
            elif i is not None:
                J[(j, i)] = J.get((j, i), 0.0) + mass
    keys = sorted(J)
    src = np.array([i for _, i in keys], np.int32)
    ptr = np.zeros(n_x + 1, np.int32)
    np.cumsum(np.bincount(np.array([j for j, _ in keys], np.int64), minlength=n_x), out=ptr[1:])
    ratio = np.minimum(np.array([J[k] for k in keys], np.float64) / np.asarray(probs_z, np.float64)[src], 1.0) if keys else np.zeros(0)
    base = llrs(np.maximum(U, p / 15 if floor is None else floor)) if mode == "condition" else None
    return ptr, src, llrs(ratio), base, unmatched
