"""An independent model of OSD-w, performOSD_enhanced(order, max_combinations, ordering), in plain numpy and itertools.  TEST CODE.

The oracle's orc_osdw and the library's osdw_kernel were written side by side and share their structure (packed rows, a rank / unrank enumeration, one
float sum per candidate); this module shares none of it: dense matrices, a textbook Gauss-Jordan routine that takes the first row at or below `row` with a
one in the column, itertools.combinations for the sweep, and a metric in exact integer arithmetic.

The metric.  Every |llr| is a double, hence k * 2^-e exactly; all of a shot's |llr| are scaled by one power of two to integers, the penalty
1e10 + w * 1e8 of an unsatisfied answer is an integer anyway, and the metric of a candidate is a Python int: it does not depend on the order of the sum.
Most cases of tests/osdw_shapes.py draw llr from the multiples of 1/8 with |llr| <= 64 (68 on the 20-column capacity case): then
1e10 + w * 1e8 + sum |llr| < 2^45 (w <= 30710 rows) with three fraction bits is exact in f64 IN ANY summation order, the model's integers are the very numbers the kernel and
the oracle compute, equal metrics are real ties, and the model is a bit-level reference for both.  On other inputs (the 44 reference cases with normal llr)
two metrics would have to agree to within a rounding error of a sum of n terms for the model to choose differently; none of the cases does.
Non-finite llr follow IEEE as the kernel's sum does: a term is bit * |llr|, so 0 * inf and any NaN make the metric NaN (no comparison with it holds), a set
bit on an infinite |llr| makes it +inf.

What the model returns beside the solution is a record of the path taken: w0 (unsatisfied checks of the OSD-0 answer), K (test positions), the number of
candidates tested, the winner's index in enumeration order and its weight (-1: the OSD-0 answer stays), and how often each branch of the selection rule fired:

  first_valid                  a satisfying candidate while the best so far is not one: taken whatever its metric
  better_valid                 a satisfying candidate with a strictly smaller metric than the satisfying best
  better_invalid               an unsatisfying candidate with a strictly smaller metric, before any satisfying one
  tie_kept_earlier             a candidate of the kind that could replace the best, with exactly its metric: the earlier one stays
  invalid_after_valid_ignored  an unsatisfying candidate after a satisfying one
  valid_over_smaller_invalid   (a subset of first_valid) the satisfying candidate's metric is LARGER than the unsatisfying best it replaces

The sweep is entered only when the OSD-0 answer misses the syndrome.  A Gauss-Jordan elimination with zero free variables solves every consistent system,
so that happens exactly when the syndrome is outside the column space of H -- and then no vector at all satisfies it: with 0/1 inputs no candidate of a
sweep is ever "valid", and of the branches above only better_invalid, tie_kept_earlier and "nothing better" can fire through performOSD_enhanced (the
reference, the oracle and the kernel all carry the valid branches as dead code).  `select` below is the rule on its own, so that the valid branches of the
MODEL are still checked against the rule as stated (tests/test_osdw_domain_cpu.py feeds it made-up candidate lists).

`mistake` runs a deliberately wrong copy of the model (MISTAKES); the CPU module asserts that each one changes an answer of the table."""
from itertools import combinations
from math import comb

import numpy as np

BRANCHES = ("first_valid", "better_valid", "better_invalid", "tie_kept_earlier", "invalid_after_valid_ignored", "valid_over_smaller_invalid")
MISTAKES = {
    "wmax_is_order": "wmax = order in place of min(order, K)",
    "maxc_plus_one": "one candidate more than max_combinations",
    "maxc_minus_one": "one candidate fewer than max_combinations",
    "colex": "co-lexicographic enumeration inside a weight class in place of lexicographic",
    "le_valid": "<= in the valid branch",
    "valid_needs_metric": "a valid candidate does not override an invalid best of smaller metric",
    "le_invalid": "<= in the invalid branch",
    "unstable_second_sort": "the sort of the non-pivot positions breaks ties by DESCENDING position",
    "nan_first": "NaN keys sorted first in place of last",
    "all_columns": "test positions drawn from all columns in place of the non-pivot ones",
    "stale_eperm": "e_permuted of the workgroup's previous shot kept (not cleared)",
    "first_candidate_free": "best metric not initialised from the OSD-0 answer: the first candidate is always taken",
}
NAN, INF = "nan", "inf"


def keys_of(llr, mistake=None):
    a = np.abs(np.asarray(llr, np.float64))
    return np.where(np.isnan(a), -np.inf if mistake == "nan_first" else np.inf, a)


def gauss_jordan(A, s):
    """Textbook Gauss-Jordan over GF(2) on copies of the dense A [m, n] and s [m] -> (A, s, pivot_rows, pivot_cols)"""
    A, s = np.array(A, np.uint8) & 1, np.array(s, np.uint8) & 1
    m, n = A.shape
    row, prow, pcol = 0, [], []
    for col in range(n):
        if row >= m:
            break
        below = np.flatnonzero(A[row:, col])
        if below.size == 0:
            continue
        p = row + int(below[0])
        if p != row:
            A[[row, p]] = A[[p, row]]
            s[[row, p]] = s[[p, row]]
        others = np.flatnonzero(A[:, col])
        others = others[others != row]
        A[others] ^= A[row]
        s[others] ^= s[row]
        prow.append(row)
        pcol.append(col)
        row += 1
    return A, s, prow, pcol


class Metric:
    """exact metrics of one shot: ints on a common power-of-two scale, or NAN / INF"""

    def __init__(self, llr):
        a = np.abs(np.asarray(llr, np.float64))
        self.nan, self.inf = np.isnan(a), np.isinf(a)
        fin = [float(x).as_integer_ratio() if np.isfinite(x) else (0, 1) for x in a]
        self.scale = max(d for _, d in fin) if fin else 1
        self.w = [p * (self.scale // d) for p, d in fin]

    def __call__(self, sol, weight):
        sol = np.asarray(sol) & 1
        if self.nan.any() or (self.inf & (sol == 0)).any():
            return NAN
        if self.inf.any():
            return INF
        base = (10 ** 10 + int(weight) * 10 ** 8) if weight > 0 else 0
        return base * self.scale + sum(self.w[j] for j in np.flatnonzero(sol))


def less(a, b):
    """a < b as IEEE doubles would have it, on ints / NAN / INF"""
    if a == NAN or b == NAN or a == INF:
        return False
    return True if b == INF else a < b


def same(a, b):
    return a != NAN and b != NAN and a == b


def select(w0_metric, candidates, mistake=None):
    """The selection rule on its own: `candidates` yields (weight, metric) in enumeration order -> (winner index or -1, counters)"""
    fired = dict.fromkeys(BRANCHES, 0)
    best, best_metric, found_valid = -1, w0_metric, False
    for idx, (wt, mt) in enumerate(candidates):
        if mistake == "first_candidate_free" and idx == 0:
            best, best_metric, found_valid = 0, mt, wt == 0
            continue
        if wt == 0:
            if not found_valid and not (mistake == "valid_needs_metric" and not less(mt, best_metric)):
                fired["first_valid"] += 1
                fired["valid_over_smaller_invalid"] += int(less(best_metric, mt))
                best, best_metric, found_valid = idx, mt, True
            elif found_valid and (less(mt, best_metric) or (mistake == "le_valid" and same(mt, best_metric))):
                fired["better_valid"] += 1
                best, best_metric = idx, mt
            elif found_valid and same(mt, best_metric):
                fired["tie_kept_earlier"] += 1
        elif found_valid:
            fired["invalid_after_valid_ignored"] += 1
        elif less(mt, best_metric) or (mistake == "le_invalid" and same(mt, best_metric)):
            fired["better_invalid"] += 1
            best, best_metric = idx, mt
        elif same(mt, best_metric):
            fired["tie_kept_earlier"] += 1
    return best, fired


def candidate_count(K, order, maxc):
    total = sum(comb(K, w) for w in range(1, min(order, K) + 1))
    return min(total, maxc) if maxc and maxc > 0 else total


def osdw(H, syndrome, llr, hard, order, maxc=None, ordering=None, mistake=None, stale=None):
    """-> (solution int8 [n], record).  H dense [m, n]; maxc None or <= 0: no limit; ordering None: stable ascending (|llr|, column) with NaN as +inf.
    `stale` (mistake "stale_eperm" only): the e_permuted the workgroup's previous shot left behind; the record returns this shot's as rec["eperm"]."""
    H = np.asarray(H, np.uint8) & 1
    m, n = H.shape
    syndrome, hard = np.asarray(syndrome, np.int64) & 1, np.asarray(hard, np.int64) & 1
    key = keys_of(llr, mistake)
    ordering = np.argsort(key, kind="stable") if ordering is None else np.asarray(ordering, np.int64)
    H64 = H.astype(np.int64)
    Hp = H64[:, ordering]                                    # the ORIGINAL permuted matrix: recompute below reads it
    residual = (syndrome + H64 @ hard) % 2
    _, s_red, prow, pcol = gauss_jordan(Hp, residual)
    s_red = s_red.astype(np.int64)
    e_perm = np.zeros(n, np.int64) if mistake != "stale_eperm" or stale is None else np.array(stale, np.int64)
    e_perm[pcol] = s_red[prow]
    sol0 = hard.copy()
    sol0[ordering] = (hard[ordering] + e_perm) % 2
    w0 = int(((H64 @ sol0) % 2 != syndrome).sum())
    rec = dict(w0=w0, K=0, tested=0, winner=-1, winner_weight=-1, eperm=e_perm.copy(), **dict.fromkeys(BRANCHES, 0))
    if w0 == 0 or order <= 0:
        return sol0.astype(np.int8), rec
    is_pivot = np.zeros(n, bool)
    is_pivot[pcol] = True
    free = list(range(n)) if mistake == "all_columns" else [c for c in range(n) if not is_pivot[c]]
    if not free:
        return sol0.astype(np.int8), rec
    k2 = key[ordering[free]]
    if mistake == "unstable_second_sort":
        free = [free[i] for i in sorted(range(len(free)), key=lambda i: (k2[i], -free[i]))]
    else:
        free = [free[i] for i in np.argsort(k2, kind="stable")]
    test = free[:order + 10]
    K = len(test)
    wmax = order if mistake == "wmax_is_order" else min(order, K)
    limit = int(maxc) if maxc and maxc > 0 else 0
    if limit:
        limit += {"maxc_plus_one": 1, "maxc_minus_one": -1}.get(mistake, 0)
        if limit <= 0:
            limit = -1                                                        # (nothing tested)
    metric = Metric(llr)
    flips, sols = [], []

    def walk():
        for w in range(1, wmax + 1):
            sets = combinations(range(K), w)
            if mistake == "colex":
                sets = sorted(combinations(range(K), w), key=lambda c: c[::-1])
            for cset in sets:
                if limit and len(flips) >= max(limit, 0):
                    return
                e = e_perm.copy()
                for t in cset:
                    e[test[t]] ^= 1
                for r, c in zip(prow, pcol):                                  # pivot by pivot, each reading what the earlier ones wrote
                    e[c] = (s_red[r] + Hp[r] @ e - Hp[r, c] * e[c]) % 2
                sol = hard.copy()
                sol[ordering] = (hard[ordering] + e) % 2
                wt = int(((H64 @ sol) % 2 != syndrome).sum())
                flips.append(cset)
                sols.append(sol)
                yield wt, metric(sol, wt)

    best, fired = select(metric(sol0, w0), walk(), mistake)
    rec.update(fired, K=K, tested=len(flips), winner=best, winner_weight=len(flips[best]) if best >= 0 else -1)
    return (sols[best] if best >= 0 else sol0).astype(np.int8), rec


def osdw_batch(H, synd, llr, hard, order, maxc=None, ordering=None, mistake=None, grid=64):
    """every shot of a call -> (solutions int8 [B, n], [record]).  Under "stale_eperm" shot b inherits the e_permuted of shot b - grid, as a workgroup
    that looped `item += gridDim.x` without clearing it would."""
    B = len(synd)
    out, recs = np.zeros((B, np.asarray(H).shape[1]), np.int8), []
    for b in range(B):
        stale = recs[b - grid]["eperm"] if mistake == "stale_eperm" and b >= grid else None
        out[b], r = osdw(H, synd[b], llr[b], hard[b], order, maxc, None if ordering is None else ordering[b], mistake, stale)
        recs.append(r)
    return out, recs
