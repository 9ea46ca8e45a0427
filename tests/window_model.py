"""Plain numpy model of sliding-window decoding (qldpc_window_decoder_create in include/qldpc_hip.h).  The windows are cut here; every window is
decoded by the CPU oracle's min-sum and OSD-0 (oracle/oracle.py), the checker the other suites use for those two."""
import numpy as np


class Matrix:
    """H in CSR (sorted columns) with the column view the model needs."""

    def __init__(self, indptr, indices, n):
        self.indptr, self.indices, self.n = np.asarray(indptr, np.int64), np.asarray(indices, np.int64), int(n)
        self.m = len(self.indptr) - 1
        self.rows = np.repeat(np.arange(self.m), np.diff(self.indptr))       # row of every CSR entry
        from scipy.sparse import csr_matrix
        self.H = csr_matrix((np.ones(self.indices.size, np.int64), self.indices, self.indptr), shape=(self.m, self.n))

    def parity(self, x):
        """H x over GF(2) for x int[B, n] -> int8[B, m]"""
        x = np.asarray(x, np.int64).reshape(-1, self.n)
        return (np.asarray((self.H @ x.T).T) & 1).astype(np.int8)


def column_layers(M, layer_rows):
    """(tau, span) per column: first layer and last layer - first layer; a column without rows has tau = 0, span = 0."""
    first = np.full(M.n, M.m, np.int64)
    last = np.full(M.n, -1, np.int64)
    np.minimum.at(first, M.indices, M.rows)
    np.maximum.at(last, M.indices, M.rows)
    empty = last < 0
    tau = np.where(empty, 0, first // layer_rows)
    return tau, np.where(empty, 0, last // layer_rows - tau)


def windows(layers, window, commit):
    """[(first layer, end layer, last?)]"""
    out, a = [], 0
    while True:
        last = a + window >= layers
        out.append((a, min(a + window, layers), last))
        if last:
            return out
        a += commit


class WindowModel:
    def __init__(self, indptr, indices, n, prior, layer_rows, window, commit):
        self.M = M = Matrix(indptr, indices, n)
        if layer_rows < 1 or M.m % layer_rows or window < 1 or not 1 <= commit <= window:
            raise ValueError("bad layer_rows / window / commit")
        self.prior = np.asarray(prior, np.float64)
        if not np.isfinite(self.prior).all():
            raise ValueError("prior must be finite")
        self.lr, self.layers = layer_rows, M.m // layer_rows
        self.tau, span = column_layers(M, layer_rows)
        if (span > 1).any():
            raise ValueError(f"column {int(np.flatnonzero(span > 1)[0])} spans more than two consecutive layers")
        self.stages = []
        for a, end, last in windows(self.layers, window, commit):
            cols = np.flatnonzero((self.tau >= a) & (self.tau < end))
            wcol = np.full(M.n, -1, np.int64)
            wcol[cols] = np.arange(cols.size)
            r0, r1 = a * layer_rows, end * layer_rows
            keep = (M.rows >= r0) & (M.rows < r1) & (wcol[M.indices] >= 0)
            ip = np.concatenate([[0], np.cumsum(np.bincount(M.rows[keep] - r0, minlength=r1 - r0))]).astype(np.int32)
            ix = wcol[M.indices[keep]].astype(np.int32)
            committed = np.ones(cols.size, bool) if last else self.tau[cols] < a + commit
            self.stages.append(dict(a=a, end=end, last=last, r0=r0, r1=r1, cols=cols, indptr=ip, indices=ix, prior=self.prior[cols], committed=committed))

    def graph_ids(self):
        """per window, the index of the first window with the same CSR and prior slice"""
        keys = [(s["indptr"].tobytes(), s["indices"].tobytes(), s["prior"].tobytes()) for s in self.stages]
        return [keys.index(k) for k in keys]

    def distinct_graphs(self):
        return len(set(self.graph_ids()))

    def decode(self, orc, syndromes, max_iter=50, alpha=1.0, alpha_mode="dynamical", clip_llr=20.0, trace=None):
        """-> err int8[B, n], conv, iters, osd int32[B], unsat uint8[B].  trace (a list) receives per window
        (stage, window syndromes, window decision, window converged) for the tests of the bookkeeping."""
        M = self.M
        s = np.ascontiguousarray(syndromes, np.int8).reshape(-1, M.m) & 1
        B = s.shape[0]
        r = s.copy()
        err = np.zeros((B, M.n), np.int8)
        conv, iters, osd = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
        for st in self.stages:
            wn = st["cols"].size
            ws = np.ascontiguousarray(r[:, st["r0"]:st["r1"]])
            det, cv, llr, it = orc.minsum_decode_batch(st["indptr"], st["indices"], wn, ws, st["prior"], max_iter=max_iter, alpha=alpha,
                                                       alpha_mode=alpha_mode, damping=1.0, clip_llr=clip_llr)
            for b in np.flatnonzero(cv == 0):
                det[b] = orc.osd0(st["indptr"], st["indices"], wn, ws[b], llr[b], det[b])
            conv += (cv != 0)
            osd += (cv == 0)
            iters += it + 1
            e = np.zeros((B, M.n), np.int8)
            cc = st["cols"][st["committed"]]
            e[:, cc] = det[:, st["committed"]] & 1
            err[:, cc] = e[:, cc]
            r ^= M.parity(e)
            if trace is not None:
                trace.append((st, ws, det.copy(), cv.copy()))
        self.r_final = r
        return err, conv, iters, osd, r.any(axis=1).astype(np.uint8)
