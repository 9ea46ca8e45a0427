"""Plain numpy model of OSD-CS (qldpc_osdcs_batch in include/qldpc_hip.h): OSD-0 followed by a combination sweep.

GF(2) state as the kernel keeps it: U = T^T of the accumulated row transform, rows packed into uint64 words; the reduced form of column h is
the XOR of the rows of U on the support of h.  Scoring follows the definition (the cost of every candidate's solution), computed from the
reduced columns of the final transform.  ``ordering`` replaces the |llr| order (the reference fixtures capture theirs)."""
import numpy as np

SCALE, CLAMP = 1048576.0, 1099511627776.0


def quantise(weights):
    """q_j = floor(w_j * 2^20 + 0.5), the product clamped to +-2^40, as int64 (relay_weight in csrc/minsum_common.h)."""
    x = np.asarray(weights, np.float64) * SCALE
    return np.floor(np.clip(x, -CLAMP, CLAMP) + 0.5).astype(np.int64)


def column_order(llr):
    """Ascending |llr|, NaN as +inf, ties by ascending index."""
    key = np.abs(np.asarray(llr, np.float64))
    key[np.isnan(key)] = np.inf
    return np.argsort(key, kind="stable")


class Graph:
    def __init__(self, indptr, indices, n):
        self.indptr, self.indices, self.n = np.asarray(indptr, np.int64), np.asarray(indices, np.int64), int(n)
        self.m = len(self.indptr) - 1
        self.mw = max(1, (self.m + 63) // 64)
        rows = np.repeat(np.arange(self.m), np.diff(self.indptr))
        order = np.lexsort((rows, self.indices))
        self.colrows = rows[order]
        self.colptr = np.concatenate([[0], np.cumsum(np.bincount(self.indices, minlength=self.n))]).astype(np.int64)

    def rows_of(self, j):
        return self.colrows[self.colptr[j]:self.colptr[j + 1]]

    def parity(self, x):
        return (np.add.reduceat(np.concatenate([np.asarray(x, np.int64)[self.indices], [0]]), self.indptr[:-1]) % 2
                * (np.diff(self.indptr) > 0)).astype(np.int8) if self.m else np.zeros(0, np.int8)


def _bit(words, r):
    return int((int(words[r >> 6]) >> (r & 63)) & 1)


def _reduced(G, U, cols):
    """reduced columns (len(cols) x mw) of `cols` against U (XOR of U's rows on each column's support)."""
    out = np.zeros((len(cols), G.mw), np.uint64)
    for i, j in enumerate(cols):
        rs = G.rows_of(j)
        if rs.size:
            out[i] = np.bitwise_xor.reduce(U[rs], axis=0)
    return out


def _unpack(words, m):
    """uint64[k][mw] -> bool[k][m] (bit r of row r)."""
    b = np.unpackbits(np.ascontiguousarray(words).view(np.uint8).reshape(words.shape[0], -1), axis=1, bitorder="little")
    return b[:, :m].astype(bool)


def eliminate(G, syndrome, llr, hard, ordering=None):
    """The part of one shot that knows neither the weights nor the order: the sweep over the whole column order -> dict(outside bool, osd0 int8[n], pivots
    [(column, row)], and for the scoring U, hard, seq)."""
    m, n, mw = G.m, G.n, G.mw
    hard = np.asarray(hard, np.int8) & 1
    U = np.zeros((m + 2, mw), np.uint64)
    for r in range(m):
        U[r, r >> 6] = np.uint64(1 << (r & 63))
    b = (np.asarray(syndrome, np.int64) + G.parity(hard)) % 2
    for r in np.flatnonzero(b):
        U[m + 1, r >> 6] |= np.uint64(1 << (int(r) & 63))
    used = np.zeros(mw, np.uint64)
    if m % 64:
        used[mw - 1] = np.uint64(((1 << 64) - 1) ^ ((1 << (m % 64)) - 1))
    seq = column_order(llr) if ordering is None else np.asarray(ordering, np.int64)
    pivots = []                                                             # (column, row)
    for j in seq:
        rs = G.rows_of(j)
        if not rs.size:
            continue
        v = np.bitwise_xor.reduce(U[rs], axis=0)
        z = v & ~used
        nz = np.flatnonzero(z)
        if not nz.size:
            continue
        w = int(nz[0])
        zw = int(z[w])
        p = 64 * w + ((zw & -zw).bit_length() - 1)
        mask = v.copy()
        mask[w] &= ~np.uint64(1 << (p & 63))
        hit = ((U[:, w] >> np.uint64(p & 63)) & np.uint64(1)).astype(bool)
        U[hit] ^= mask
        used[w] |= np.uint64(1 << (p & 63))
        pivots.append((int(j), p))
    bvec = U[m + 1]
    outside = bool(np.any(bvec & ~used))
    x0 = hard.copy()
    for j, p in pivots:
        x0[j] = hard[j] ^ _bit(bvec, p)
    return dict(outside=outside, osd0=x0, pivots=pivots, U=U, hard=hard, seq=seq)


def reduced_columns(G, E):
    """the non-pivot columns of an elimination in the column order and their reduced columns against its final transform -> (T list, BT bool[len(T)][m]);
    kept in E: they depend on neither the weights nor the order"""
    if "BT" not in E:
        is_piv = np.zeros(G.n, bool)
        is_piv[[j for j, _ in E["pivots"]]] = True
        T = [int(j) for j in E["seq"] if not is_piv[j]]
        RT = _reduced(G, E["U"], T)
        E["T"], E["BT"] = T, _unpack(RT, G.m) if T else np.zeros((0, G.m), bool)
    return E["T"], E["BT"]


def score(G, E, weights, order):
    """The combination sweep on an elimination E of eliminate() -> the dict of osd_cs."""
    m = G.m
    outside, x0, pivots, hard = E["outside"], E["osd0"], E["pivots"], E["hard"]
    res = dict(outside=outside, osd0=x0, pivots=pivots)
    if outside:
        res.update(solution=None, flips=(-1, -1), cost=None, T=None)
        return res
    q = quantise(weights)
    sq = np.zeros(m, np.int64)
    pc = np.full(m, -1, np.int64)
    for j, p in pivots:
        sq[p] = -q[j] if x0[j] else q[j]
        pc[p] = j
    T, BT = reduced_columns(G, E)
    sig = np.where(hard[T] == 1, -1, 1).astype(np.int64) if T else np.zeros(0, np.int64)
    d1 = sig * q[T] + BT.astype(np.int64) @ sq if T else np.zeros(0, np.int64)
    lam = min(int(order), len(T))
    pairs = [(a, bb) for a in range(lam) for bb in range(a + 1, lam)]
    d2 = np.array([d1[a] + d1[bb] - 2 * int((BT[a] & BT[bb]).astype(np.int64) @ sq) for a, bb in pairs], np.int64)
    deltas = np.concatenate([[0], d1, d2]).astype(np.int64)
    k = int(np.argmin(deltas))                                              # first minimum: the earlier candidate wins ties
    x = x0.copy()
    flips = (-1, -1)
    if 1 <= k <= len(T):
        comb, flips = BT[k - 1], (T[k - 1], -1)
    elif k > len(T):
        a, bb = pairs[k - 1 - len(T)]
        comb, flips = BT[a] ^ BT[bb], (T[a], T[bb])
    if k:
        for j in flips:
            if j >= 0:
                x[j] ^= 1
        for r in np.flatnonzero(comb):
            x[pc[r]] ^= 1
    res.update(solution=x.astype(np.int8), flips=flips, cost=int(q[x0 == 1].sum() + deltas[k]), T=T, deltas=deltas, pairs=pairs)
    return res


def osd_cs(G, syndrome, llr, hard, weights, order, ordering=None):
    """One shot -> dict(solution int8[n], flips (int, int), outside bool, osd0 int8[n], cost int, pivots list, T list).
    outside = True: s + H hard is not in the column space (the library then returns qldpc_osd0_batch's answer; solution is None here)."""
    return score(G, eliminate(G, syndrome, llr, hard, ordering), weights, order)


def osd_cs_batch(G, syndromes, llr, hard, weights, order, ordering=None):
    """B shots -> (solution int8[B, n] (None rows for outside shots), flips int32[B, 2], outside bool[B], osd0 int8[B, n])."""
    B = len(syndromes)
    sol = np.zeros((B, G.n), np.int8)
    flips = np.full((B, 2), -1, np.int32)
    outside = np.zeros(B, bool)
    osd0 = np.zeros((B, G.n), np.int8)
    for i in range(B):
        r = osd_cs(G, syndromes[i], llr[i], hard[i], weights, order, None if ordering is None else ordering[i])
        outside[i], osd0[i] = r["outside"], r["osd0"]
        if not r["outside"]:
            sol[i], flips[i] = r["solution"], r["flips"]
    return sol, flips, outside, osd0
