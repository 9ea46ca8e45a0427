"""Plain model of the LSD cluster statistics (qldpc_lsd_stats_batch), of the confidence score and its histogram (qldpc_circuit_plan_use_confidence) and of
the post-selection curve (simulation/postselect.py), each written from its definition in include/qldpc_hip.h.  The statistics come from
lsd_model.lsd(..., trace=) and lsd_model.components: the clusters are rebuilt from nothing as the connected components of (R, A) at termination, so nothing
here shares structure with csrc/lsd.hip or csrc/confidence.hip.  Every number is a Python integer until it is stored: nothing can wrap unseen.

Plain module (no pytest hooks)."""
import math

import numpy as np

import lsd_model as M

NONE = (1 << 64) - 1                      # "no statement"
KINDS = ("cols_1", "cols_2", "cols_inf", "llr_1", "llr_2", "llr_inf")          # QLDPC_CONF_* in order; kind k reads word k + 1


def clusters(G, syndrome, hard, A):
    """the clusters a flag-0 shot ends with -> [(rows, columns)]: R = the ones of s + H hard and the rows of the columns of A"""
    bvec = (np.asarray(syndrome, np.int64) + G.parity(np.asarray(hard, np.int8) & 1)) % 2
    R = 0
    for r in np.flatnonzero(bvec):
        R |= 1 << int(r)
    for j in A:
        R |= G.mask(j)
    return [(M._rows(mask), list(cols)) for mask, cols in M.components(G, R, A)]


def stats_of(cl, weight=None):
    """the eight words of a flag-0 shot from its clusters [(rows, columns)]"""
    a = [len(cols) for _, cols in cl]
    r = [len(rows) for rows, _ in cl]
    W = [sum(int(weight[j]) for j in cols) for _, cols in cl] if weight is not None else [0] * len(cl)
    if not cl:
        return [0] * 8
    return [len(cl), sum(a), sum(x * x for x in a), max(a), sum(W), sum(x * x for x in W), max(W), max(r)]


def lsd_stats(G, syndrome, llr, hard, bits_per_step=1, max_rows=512, weight=None):
    """one shot -> (info of lsd_model.lsd, the eight words as Python integers)"""
    tr = {}
    _, info = M.lsd(G, syndrome, llr, hard, bits_per_step, max_rows, trace=tr, osd0=lambda *a: np.zeros(G.n, np.int8))
    if info[0] != 0:
        return info, [NONE] * 8
    return info, stats_of(clusters(G, syndrome, hard, tr.get("A", [])), weight)


def stats_from_traces(G, shots, info, traces, weight=None):
    """a batch whose model answers are at hand (lsd_shapes.answers) -> uint64[B, 8]"""
    out = np.zeros((shots.synd.shape[0], 8), np.uint64)
    for b in range(shots.synd.shape[0]):
        row = [NONE] * 8 if info[b, 0] != 0 else stats_of(clusters(G, shots.synd[b], shots.hard[b], traces[b].get("A", [])), weight)
        assert all(0 <= v <= NONE for v in row)
        out[b] = np.array(row, np.uint64)
    return out


def score(kind, z, x=None):
    """the score of a trial from the eight words of sector Z and of sector X (None: a one-sector plan); kind: a name of KINDS or its number"""
    k = KINDS.index(kind) if isinstance(kind, str) else int(kind)
    z = [int(v) for v in z]
    x = [int(v) for v in x] if x is not None else [0] * 8
    if z[0] == NONE or x[0] == NONE:
        return NONE
    if k % 3 == 2:
        return max(z[k + 1], x[k + 1])
    return min(z[k + 1] + x[k + 1], NONE - 1)


def scores(kind, Z, X=None):
    """uint64[B] from uint64[B, 8] per sector"""
    return np.array([score(kind, Z[b], None if X is None else X[b]) for b in range(len(Z))], np.uint64)


def bin_of(s, edges):
    """the number of edges <= score"""
    return sum(1 for e in edges if int(e) <= int(s))


def histogram(score_list, outcomes, edges):
    """uint64[nbins, 4]: hist[bin][outcome], outcome = bit0 z_err | bit1 x_err"""
    hist = np.zeros((len(edges) + 1, 4), np.uint64)
    for s, o in zip(score_list, outcomes):
        hist[bin_of(s, edges), int(o) & 3] += np.uint64(1)
    return hist


def curve(hist):
    """for every cut k = 0 .. nbins (accept the trials in bins < k) -> a list of dicts: accepted, failures, failures_z, failures_x, abort_rate, ler,
    std_error (binomial); ler and std_error are nan where nothing is accepted"""
    rows = [[int(v) for v in r] for r in np.asarray(hist)]
    total = sum(sum(r) for r in rows)
    out = []
    for k in range(len(rows) + 1):
        acc = sum(sum(r) for r in rows[:k])
        fail = sum(r[1] + r[2] + r[3] for r in rows[:k])
        fz = sum(r[1] + r[3] for r in rows[:k])
        fx = sum(r[2] + r[3] for r in rows[:k])
        ler = fail / acc if acc else math.nan
        out.append({"accepted": acc, "failures": fail, "failures_z": fz, "failures_x": fx, "abort_rate": (1.0 - acc / total) if total else math.nan,
                    "ler": ler, "std_error": math.sqrt(ler * (1.0 - ler) / acc) if acc else math.nan})
    return out
