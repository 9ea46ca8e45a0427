"""Plain model of BP+LSD (qldpc_lsd_batch in include/qldpc_hip.h), written from the definition: every round it rebuilds the clusters as the
connected components of (R, A) from nothing and decides a cluster's validity by building a basis of its own columns from nothing.  It keeps no
transform, no labels and no caches, so it shares no structure with csrc/lsd.hip.  Row sets are Python integers (bit r = row r of H).

Shots that end with flag 1 or 2 get OSD-0's answer, taken from tests/osd_cs_model.py (its sweep over the whole column order)."""
import numpy as np

import osd_cs_model as CS


class Graph(CS.Graph):
    def __init__(self, indptr, indices, n):
        super().__init__(indptr, indices, n)
        self._mask, self._cols = {}, {}

    def cols_of(self, r):
        """the columns of row r as a frozenset of ints"""
        if r not in self._cols:
            self._cols[r] = frozenset(int(j) for j in self.indices[self.indptr[r]:self.indptr[r + 1]])
        return self._cols[r]

    def mask(self, j):
        """the rows of column j as an integer"""
        if j not in self._mask:
            v = 0
            for r in self.rows_of(j):
                v |= 1 << int(r)
            self._mask[j] = v
        return self._mask[j]


def column_keys(llr):
    """key(j) = (|llr_j| with NaN as +inf, j) as a list of tuples"""
    a = np.abs(np.asarray(llr, np.float64))
    a[np.isnan(a)] = np.inf
    return [(float(a[j]), j) for j in range(a.size)]


def _rows(v):
    out = []
    while v:
        low = v & -v
        out.append(low.bit_length() - 1)
        v ^= low
    return out


def components(G, R, A):
    """connected components of the bipartite graph on (R, A) -> [(row mask, [columns of A inside, in A's order])]; every row of a column of A is in R"""
    comps = []                                     # [mask, columns]
    for r in _rows(R):
        comps.append([1 << r, []])
    for j in A:
        cm = G.mask(j)
        assert cm & ~R == 0
        hit = [c for c in comps if c[0] & cm]
        merged = [0, []]
        for c in hit:
            merged[0] |= c[0]
            merged[1] += c[1]
            comps.remove(c)
        merged[1].append(j)
        comps.append(merged)
    pos = {j: i for i, j in enumerate(A)}
    return [(mask, sorted(cols, key=pos.get)) for mask, cols in comps]


def _reduce(basis, v, combo=0):
    """v against a basis {lowest bit: (vector, combination)} -> what is left of it, and the combination of basis members taken"""
    while v:
        low = v & -v
        if low not in basis:
            break
        bv, bc = basis[low]
        v ^= bv
        combo ^= bc
    return v, combo


def span_basis(G, cols):
    """basis of the span of `cols` in their order -> (basis, pivots): pivots = the columns independent of the ones before them; a member's combination is
    a bit set over the positions in `pivots`"""
    basis, pivots = {}, []
    for j in cols:
        v, combo = _reduce(basis, G.mask(j), 1 << len(pivots))
        if v:
            basis[v & -v] = (v, combo)
            pivots.append(j)
    return basis, pivots


def lsd(G, syndrome, llr, hard, bits_per_step=1, max_rows=512, trace=None, osd0=None):
    """one shot -> (solution int8[n], info (flag, rounds, |R|, |A|)); trace (a dict, optional) receives A, the pivots, the clusters of every round and the size
    of every round's list N_t.
    osd0(syndrome, llr, hard) answers the shots that end with flag 1 or 2; the default is the sweep of tests/osd_cs_model.py, which is OSD-0's answer
    where s + H hard lies in the column space (a flag-2 shot never does: pass the oracle's or the library's OSD-0 there)."""
    assert 1 <= bits_per_step <= 64 and 1 <= max_rows <= 1024
    hard = np.asarray(hard, np.int8) & 1
    bvec = (np.asarray(syndrome, np.int64) + G.parity(hard)) % 2
    b = 0
    for r in np.flatnonzero(bvec):
        b |= 1 << int(r)
    key = column_keys(llr)
    A, inA, R, rounds = [], set(), b, 0
    valid_memo = {}

    def fail(flag):
        sol = osd0(syndrome, llr, hard) if osd0 is not None else CS.eliminate(G, syndrome, llr, hard)["osd0"]
        return np.asarray(sol, np.int8), (flag, 0, 0, 0)

    while True:
        invalid = []
        comps = components(G, R, A)
        for mask, cols in comps:
            k = (mask & b, tuple(cols))
            if k not in valid_memo:                                          # (a pure function of the cluster: computed from nothing on first sight)
                valid_memo[k] = _reduce(span_basis(G, cols)[0], mask & b)[0] == 0
            if not valid_memo[k]:
                invalid.append(mask)
        if trace is not None:
            trace.setdefault("clusters", []).append([(bin(mask).count("1"), len(cols)) for mask, cols in comps])
        if not invalid:
            break
        rounds += 1
        picks = set()
        for mask in invalid:
            cand = set().union(*(G.cols_of(r) for r in _rows(mask))) - inA
            if not cand:
                return fail(2)
            picks.update(sorted(cand, key=key.__getitem__)[:bits_per_step])
        grown = R
        for j in picks:
            grown |= G.mask(j)
        if trace is not None:
            trace.setdefault("lists", []).append(len(picks))                  # |N_t| of every round that found its candidates (a capped one too)
        if bin(grown).count("1") > max_rows:
            return fail(1)
        A += sorted(picks, key=key.__getitem__)
        inA |= picks
        R = grown
    basis, pivots = span_basis(G, A)
    left, combo = _reduce(basis, b)
    assert left == 0
    sol = hard.copy()
    for i, j in enumerate(pivots):
        if (combo >> i) & 1:
            sol[j] ^= 1
    if trace is not None:
        trace["A"], trace["pivots"] = list(A), pivots
    return sol, (0, rounds, bin(R).count("1"), len(A))


def lsd_batch(G, syndromes, llr, hard, bits_per_step=1, max_rows=512, osd0=None):
    """-> (solution int8[B, n], info int32[B, 4])"""
    syndromes = np.asarray(syndromes).reshape(-1, G.m)
    B = syndromes.shape[0]
    llr, hard = np.asarray(llr, np.float64).reshape(B, G.n), np.asarray(hard).reshape(B, G.n)
    sol, info = np.zeros((B, G.n), np.int8), np.zeros((B, 4), np.int32)
    for i in range(B):
        sol[i], info[i] = lsd(G, syndromes[i], llr[i], hard[i], bits_per_step, max_rows, osd0=osd0)
    return sol, info
