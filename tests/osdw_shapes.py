"""Seeded cases for OSD-w (qldpc_osdw_batch: performOSD_enhanced with order > 0) over the domain its host checks accept, and the edges of the literal
elimination under it.  tests/test_osdw_domain_cpu.py checks with the model (tests/osdw_model.py) and the oracle alone that every case holds what it is
named for; tests/test_osdw_domain_gpu.py runs them.  Plain module (no pytest hooks); deterministic from osd_shapes.SEED.

The rules below restate what qldpc_osdw_batch (csrc/gf2.hip) decides on the host in plain arithmetic: an independent statement, not a copy the library reads.

Most cases are hand-built on one kind of matrix, `stacked(r, f, extra)`: [I_r | F] over `extra` further rows (a zero row, a copy of row 0, row 0 + row 1),
with |llr| ascending in the column index so that the elimination order is the column order, the pivots are the r identity columns (no swap) and the f columns
of F are the non-pivot positions, least reliable first.  With a zero row whose syndrome bit is one, every answer misses exactly that check: the metric is
1e10 + 1e8 + sum |llr| over the answer's ones, the answer is hard + e, and flipping the non-pivot column c toggles e[c] and the pivots in the support of F[:, c].
The pivots carry |llr| of 1/8 .. r/8 (under one in all), the non-pivot columns 30, 32, 34, ..: a flip set gains |llr[c]| for every column with hard[c] = 1 and
loses it for every other, so `hard` marks the winner.  What a case expects (K, candidates, winner, branches) is written in TABLE by hand from that.

Two things the batch recipe cannot do, and why (the CPU module asserts both):
  * no candidate of a sweep is ever valid (osdw_model's docstring): the three valid branches of the selection rule cannot fire through the entry point;
  * K = min(n - rank, order + 10) and with it the candidate count are the same for every swept shot of one call: a call cannot mix long and short
    candidate lists, only swept shots, satisfiable ones (w0 = 0) and -- on a matrix of full column rank -- K = 0 shots."""
from math import comb
from types import SimpleNamespace

import numpy as np

import osd_shapes as OS

# ---------------------------------------------------------------------------------------------------------------- the host's rules
MAX_ORDER, MAX_CAND, GRID = 10, 65536, 64          # kOsdwMaxOrder, kOsdwMaxCand, the launcher's grid = min(B, 64)
ELIM_MAX = 150 * 1024                              # kOsdElimMax
MODEL_MAX = 5000                                   # candidates per shot up to which the model runs; beyond, the oracle alone
ORDER_TEXT, CAND_TEXT, LDS_TEXT = "above the supported maximum 10", "flip sets per shot; pass max_combinations <= 65536", "matrix too large for the LDS scratch"
ERR_INVALID, ERR_UNSUPPORTED = -1, -4


def nwords_of(n):
    return ((n + 7) // 8 + 7) // 8


def elim_lds_bytes(m, nwords):
    return 5 * m + 8 * nwords + 40


def worst_candidates(n, order, maxc):
    """the bound the host refuses by: sum_{w <= min(order, K')} C(K', w) with K' = min(n, order + 10), cut by max_combinations"""
    k = min(n, order + 10)
    worst = sum(comb(k, w) for w in range(1, min(order, k) + 1))
    return min(worst, maxc) if maxc and maxc > 0 else worst


def verdict(m, n, order, maxc):
    """-> None (accepted) or (return code, text of the message), in the order the host checks"""
    if order > MAX_ORDER:
        return ERR_INVALID, ORDER_TEXT
    if n == 0 or m == 0:
        return None
    if worst_candidates(n, order, maxc) > MAX_CAND:
        return ERR_UNSUPPORTED, CAND_TEXT
    if elim_lds_bytes(m, nwords_of(n)) > ELIM_MAX:
        return ERR_UNSUPPORTED, LDS_TEXT
    return None


def grid_of(B):
    return min(B, GRID)


def trips_of(B):
    """shots the busiest workgroup takes"""
    return -(-B // grid_of(B))


# ---------------------------------------------------------------------------------------------------------------- matrices
def _rng(name, *what):
    return OS._rng("osdw:" + name, *what)


def stacked(name, r, f, extra=("zero",)):
    rng = _rng(name, 1)
    F = (rng.random((r, f)) < 0.5).astype(np.uint8)
    top = np.concatenate([np.eye(r, dtype=np.uint8), F], axis=1)
    rows = {"zero": lambda: np.zeros(r + f, np.uint8), "dup0": lambda: top[0].copy(), "sum01": lambda: top[0] ^ top[1]}
    return np.concatenate([top] + [rows[k]()[None, :] for k in extra], axis=0)


def ascending_llr(r, f, B=1):
    """pivot columns 1/8 .. r/8, non-pivot columns 30, 32, ..: the elimination order is the column order"""
    return np.tile(np.concatenate([np.arange(1, r + 1) / 8.0, 30.0 + 2.0 * np.arange(f)]), (B, 1))


def eighths(rng, shape, top=512):
    return rng.integers(-top, top + 1, shape) / 8.0


def marked(H, r, f, sets, seed_name):
    """one shot per entry of `sets` (test positions whose column gets hard = 1) on a stacked matrix: the syndrome random on the identity rows, one on the
    first extra row (a zero row, or the second of two equal rows -- outside the column space either way)"""
    rng = _rng(seed_name, 2)
    B, (m, n) = len(sets), H.shape
    synd = (rng.random((B, m)) < 0.5).astype(np.int8)
    synd[:, r] = 1 ^ (synd[:, 0] if H[r].any() else 0)
    hard = np.zeros((B, n), np.int8)
    for b, s in enumerate(sets):
        hard[b, [r + t for t in s]] = 1
    return synd, ascending_llr(r, f, B), hard


def dep_matrix(name, n, r=6):
    """stacked(r, n - r) over a zero row (degree 0), a copy of row 0 and row 0 + row 1; the last column a copy of column r, the one before it a single one
    (a row of degree 1 where F leaves one empty is not forced; the zero row, the equal rows and the equal columns are)"""
    A = stacked(name, r, n - r, ("zero", "dup0", "sum01"))
    A[:, n - 2] = 0
    A[r - 1, n - 2] = 1
    A[r + 1, n - 2] = A[0, n - 2]
    A[r + 2, n - 2] = A[0, n - 2] ^ A[1, n - 2]
    A[:, n - 1] = A[:, r]
    return A


def outside_syndromes(H, r, rng, B):
    """random syndromes, inconsistent on the zero row below the r identity rows"""
    synd = (rng.random((B, H.shape[0])) < 0.5).astype(np.int8)
    synd[:, r] = 1
    return synd


def tall_matrix(m, r=12, f=12):
    """stacked(r, f) on top, then m - r - 1 copies of its rows in turn and a zero row: rank r, f non-pivot columns, every pivot step updates about
    m / r * (row weight) rows and leaves as many all-zero rows behind"""
    top = stacked("tall", r, f, ())
    return np.concatenate([top, top[np.arange(m - r - 1) % r], np.zeros((1, r + f), np.uint8)])


# ---------------------------------------------------------------------------------------------------------------- the cases
# name -> (builder, order, maxc, expectations, note).  A builder returns (H, synd, llr, hard, ordering or None).  Expectations, checked against the model
# (the oracle's answers where the model does not run) by the CPU module:
#   K, tested: of every swept shot;  swept: how many shots enter the sweep (default: all);  winner: (index, weight) per shot, -1 = the OSD-0 answer stays;
#   fires: branches that fire at least once in the case;  refused: the verdict of the host's rules.
def _k0():
    H = np.concatenate([np.eye(4, dtype=np.uint8), np.array([[1, 1, 0, 0], [0, 1, 1, 1]], np.uint8)])
    rng = _rng("k0", 2)
    synd = (rng.random((4, 6)) < 0.5).astype(np.int8)
    synd[:, 4] = 1 ^ synd[:, 0] ^ synd[:, 1]                              # row 4 = row 0 + row 1 of the identity: inconsistent
    return H, synd, eighths(rng, (4, 4)), (rng.random((4, 4)) < 0.5).astype(np.int8), None


def _marked(name, r, f, sets, extra=("zero",)):
    def build():
        H = stacked(name, r, f, extra)
        return (H,) + marked(H, r, f, sets, name) + (None,)
    return build


def _cut_tie():
    H = stacked("k_cut_tie", 3, 13, ("dup0",))
    synd, llr, hard = marked(H, 3, 13, [(10, 11), (10, 11)], "k_cut_tie")
    llr[:, 3 + 11] = llr[:, 3 + 10]                                        # the 11th and 12th non-pivot positions tie across the cut at order + 10 = 11
    llr[1] = -llr[1]
    return H, synd, llr, hard, None


def _tie_pair():
    H = stacked("sel_tie", 3, 13)
    H[:, 3 + 5] = H[:, 3 + 7] = H[:, 3 + 4]                                # equal columns with equal |llr|: candidates of exactly the same metric
    synd, llr, hard = marked(H, 3, 13, [(4, 7), (4, 7)], "sel_tie")
    llr[:, 3 + 5:3 + 8] = llr[0, 3 + 4]                                    # (a run of equal magnitudes keeps the order the column order)
    hard[1, 3 + 5] = 1                                                     # second shot: three equal gains, the first still wins
    return H, synd, llr, hard, None


def _n1():
    H = np.zeros((1, 1), np.uint8)
    return H, np.ones((2, 1), np.int8), np.array([[2.5], [-2.5]]), np.array([[0], [1]], np.int8), None


def _n1_k0():
    H = np.ones((2, 1), np.uint8)
    return H, np.array([[1, 0], [0, 1], [1, 1]], np.int8), np.array([[1.0], [2.0], [3.0]]), np.array([[0], [1], [1]], np.int8), None


def _zero_row(n, sets):
    """1 x n with an empty row: rank 0, every column a test position; hard marks the winning flip set"""
    def build():
        B = len(sets)
        hard = np.zeros((B, n), np.int8)
        for b, s in enumerate(sets):
            hard[b, list(s)] = 1
        return np.zeros((1, n), np.uint8), np.ones((B, 1), np.int8), ascending_llr(0, n, B), hard, None
    return build


def _inputs(name, n, B=6, with_nonfinite=False):
    def build():
        H = dep_matrix(name, n)
        rng = _rng(name, 2)
        synd = outside_syndromes(H, 6, rng, B)
        llr = eighths(rng, (B, n), 64)                                     # |llr| <= 8 in eighths over n columns: runs of equal magnitude everywhere
        hard = (rng.random((B, n)) < 0.4).astype(np.int8)
        if with_nonfinite:
            for b, vals in enumerate(((np.nan,), (np.inf, -np.inf), (np.nan, np.inf), (-0.0, 0.0, -0.0), (np.inf,), (-np.inf, np.nan, -0.0))):
                llr[b, rng.permutation(n)[:len(vals)]] = vals
        return H, synd, llr, hard, None
    return build


def _lds_line(m):
    """three shots on tall_matrix(m): the copies' syndrome bits agree with their originals, the zero row's is one, so every answer misses that check alone
    (the second shot: and one copy's) and `hard` marks the winner as on the small stacked matrices"""
    def build():
        H = tall_matrix(m)
        rng = _rng("lds", 2)
        top = (rng.random((3, 12)) < 0.5).astype(np.int8)
        synd = np.concatenate([top, top[:, np.arange(m - 13) % 12], np.ones((3, 1), np.int8)], axis=1)
        synd[1, m - 2] ^= 1
        hard = np.zeros((3, 24), np.int8)
        hard[0, 12 + 10], hard[1, 12 + 3] = 1, 1
        return H, synd, ascending_llr(12, 12, 3), hard, None
    return build


TRIP_B = 64 + 64 + 5


def _trips(kind):
    """B = 133: workgroup b takes shots b, b + 64 and (b < 5) b + 128.  "small": satisfiable shots (every third, one place on with each trip: a workgroup
    goes satisfiable -> swept, swept -> satisfiable or swept -> swept) among swept ones, random llr / hard, so that order, pivots, e_permuted and the
    winner change from one trip to the next; "tall": satisfiable and K = 0 shots on the matrix of full column rank; "ordering": the small matrix with a caller's ordering, a random permutation on every third shot and
    the sorted order elsewhere."""
    def build():
        rng = _rng("trips_" + kind, 2)
        if kind == "tall":
            H = _k0()[0]
        else:
            H = stacked("trips", 4, 12, ("zero", "sum01"))
        m, n = H.shape
        B = TRIP_B
        llr, hard = eighths(rng, (B, n)), (rng.random((B, n)) < 0.4).astype(np.int8)
        err = (rng.random((B, n)) < 0.3).astype(np.int64)
        synd = ((H.astype(np.int64) @ err.T) % 2).T.astype(np.int8)
        sat = (np.arange(B) % 64) % 3 == (np.arange(B) // 64) % 3
        bad = (rng.random((B, m)) < 0.5).astype(np.int8)
        if kind == "tall":
            bad[:, 4] = 1 ^ bad[:, 0] ^ bad[:, 1]
        else:
            bad[:, 4] = 1
        synd[~sat] = bad[~sat]
        ordering = None
        if kind == "ordering":
            key = np.abs(llr)
            ordering = np.argsort(key, axis=1, kind="stable").astype(np.int32)
            for b in range(1, B, 3):
                ordering[b] = rng.permutation(n)
        return H, synd, llr, hard, ordering
    return build


T3 = 13 + 78 + 286                 # candidates of order 3 over K = 13
TABLE = {
    # ---- K edges
    "k0_tall": (_k0, 2, None, dict(K=0, tested=0, winner=[(-1, -1)] * 4), "6 x 4 of full column rank, syndromes outside its column space: no test position"),
    "k1": (_marked("k1", 4, 1, [(), (0,)]), 3, None, dict(K=1, tested=1, winner=[(-1, -1), (0, 1)], fires=("better_invalid",)), "one non-pivot column"),
    "k_below_order": (_marked("k_below_order", 4, 3, [(0, 1, 2), (1,)]), 4, None, dict(K=3, tested=7, winner=[(6, 3), (1, 1)], fires=("better_invalid",)),
                      "K = order - 1: wmax = K, 2^3 - 1 candidates"),
    "k_exact": (_marked("k_exact", 3, 12, [(10, 11), (11,)]), 2, None, dict(K=12, tested=78, winner=[(77, 2), (11, 1)], fires=("better_invalid",)),
                "K = order + 10 exactly: the last test position is the last non-pivot column"),
    "k_cut_tie": (_cut_tie, 1, None, dict(K=11, tested=11, winner=[(10, 1), (10, 1)], fires=("better_invalid",)),
                  "13 non-pivot columns, K = 11: equal |llr| at the 11th and 12th, the lower position is tested (and wins)"),
    "n1": (_n1, 2, None, dict(K=1, tested=1, winner=[(-1, -1), (0, 1)], fires=("better_invalid",)), "n = 1 and m = 1: a 1 x 1 zero matrix"),
    "n1_k0": (_n1_k0, 1, None, dict(K=0, tested=0, swept=2, winner=[(-1, -1)] * 3), "n = 1 with its column a pivot; the third syndrome is satisfiable"),
    "m1": (_zero_row(6, [(5,), (0, 3)]), 2, None, dict(K=6, tested=21, winner=[(5, 1), (8, 2)], fires=("better_invalid",)), "m = 1: one empty row"),
    # ---- capacity (the model is excused above MODEL_MAX candidates; the oracle is not)
    "cap_65535": (_zero_row(17, [(9, 10, 11, 12, 13, 14, 15, 16), (0, 16), ()]), 8, None, dict(K=17, tested=65535), "the largest count accepted uncut"),
    "cap_n18_refused": (_zero_row(18, [()]), 8, None, dict(refused=(ERR_UNSUPPORTED, CAND_TEXT)), "106761 candidates without max_combinations"),
    "cap_n18_cut": (_zero_row(18, [(3, 5, 7, 9, 11, 13), (17,)]), 8, 65536, dict(K=18, tested=65536), "the same cut to the whole slab"),
    "cap_order10": (_zero_row(20, [(0, 1, 2, 3, 4), (19,)]), 10, 65536, dict(K=20, tested=65536), "the largest order on the largest test list, cut"),
    "order11_refused": (_zero_row(4, [()]), 11, 16, dict(refused=(ERR_INVALID, ORDER_TEXT)), "order 11"),
    # ---- max_combinations on order 3 over K = 13 (13 + 78 + 286 = 377): `hard` marks candidate maxc - 1 and candidate maxc
    "cut_1": (_marked("cut", 3, 13, [(0, 1)]), 3, 1, dict(K=13, tested=1, winner=[(0, 1)], fires=("better_invalid",)), "max_combinations = 1"),
    "cut_c1m": (_marked("cut", 3, 13, [(11, 12)]), 3, 12, dict(K=13, tested=12, winner=[(11, 1)], fires=("better_invalid",)), "C(K,1) - 1"),
    "cut_c1": (_marked("cut", 3, 13, [(0, 1, 12)]), 3, 13, dict(K=13, tested=13, winner=[(12, 1)], fires=("better_invalid",)), "C(K,1): the whole first class"),
    "cut_c1p": (_marked("cut", 3, 13, [(0, 1, 2)]), 3, 14, dict(K=13, tested=14, winner=[(13, 2)], fires=("better_invalid",)), "C(K,1) + 1: one pair"),
    "cut_256": (_marked("cut", 3, 13, [(2, 10, 11, 12)]), 3, 256, dict(K=13, tested=256, winner=[(255, 3)], fires=("better_invalid",)), "one candidate per thread"),
    "cut_257": (_marked("cut", 3, 13, [(2, 3, 4, 5, 11, 12)]), 3, 257, dict(K=13, tested=257, winner=[(256, 3)], fires=("better_invalid",)),
                "the first candidate of a thread's second round wins"),
    "cut_total": (_marked("cut", 3, 13, [(10, 11, 12)]), 3, T3, dict(K=13, tested=T3, winner=[(T3 - 1, 3)], fires=("better_invalid",)), "the uncut total"),
    "cut_total1": (_marked("cut", 3, 13, [(10, 11, 12)]), 3, T3 + 1, dict(K=13, tested=T3, winner=[(T3 - 1, 3)], fires=("better_invalid",)), "the total + 1"),
    "cut_none": (_marked("cut", 3, 13, [(10, 11, 12)]), 3, 0, dict(K=13, tested=T3, winner=[(T3 - 1, 3)], fires=("better_invalid",)), "0: no limit"),
    # ---- the selection rule
    "sel_deep": (_marked("sel_deep", 3, 13, [(9, 11, 12), (3, 8)]), 3, None, dict(K=13, tested=T3, winner=[(13 + 78 + 284, 3), (13 + 37, 2)], fires=("better_invalid",)),
                 "the winner has weight 3 resp. 2 and lies past index 256 resp. in the second class"),
    "sel_tie": (_tie_pair, 1, None, dict(K=11, tested=11, winner=[(4, 1), (4, 1)], fires=("better_invalid", "tie_kept_earlier")),
                "two resp. three candidates of exactly equal metric: the earliest is kept"),
    "sel_none": (_marked("sel_none", 3, 13, [(), ()]), 2, None, dict(K=12, tested=78, winner=[(-1, -1)] * 2), "no candidate improves: the OSD-0 answer is returned"),
    # ---- inputs
    "in_nonfinite": (_inputs("in_nonfinite", 20, with_nonfinite=True), 2, None, dict(K=12, tested=78), "NaN, +-inf, -0.0 and runs of equal |llr|; nonzero hard; "
                     "rows of degree 0 and 1, equal rows, equal columns"),
    "n63": (_inputs("n63", 63), 1, None, dict(K=11, tested=11), "one word, short by a bit"),
    "n64": (_inputs("n64", 64), 2, 100, dict(K=12, tested=78), "one full word"),
    "n65": (_inputs("n65", 65), 2, None, dict(K=12, tested=78), "one column in the second word"),
    "n129": (_inputs("n129", 129), 2, None, dict(K=12, tested=78), "one column in the third word"),
    # ---- the LDS line of the elimination scratch, 5 m + 48 bytes at one row word
    "lds_13097": (_lds_line(13097), 1, None, dict(K=11, tested=11), "65533 bytes: the last launch within 64 KiB"),
    "lds_13098": (_lds_line(13098), 1, None, dict(K=11, tested=11), "65538 bytes: the first launch above 64 KiB"),
    "lds_30710": (_lds_line(30710), 1, None, dict(K=11, tested=11), "153598 bytes: the last accepted"),
    "lds_30711": (_lds_line(30711), 1, None, dict(refused=(ERR_UNSUPPORTED, LDS_TEXT)), "153603 bytes: refused"),
    # ---- second and third trips of a workgroup
    "trips_small": (_trips("small"), 3, None, dict(K=12, tested=12 + 66 + 220, swept=None), "133 shots: satisfiable and swept shots alternate in every workgroup"),
    "trips_tall": (_trips("tall"), 3, None, dict(K=0, tested=0, swept=None), "133 shots: satisfiable and K = 0 shots alternate"),
    "trips_ordering": (_trips("ordering"), 2, 70, dict(K=12, tested=70, swept=None), "133 shots under a caller's ordering, a third of them not sorted by |llr|"),
}
RUN = [n for n in TABLE if "refused" not in TABLE[n][3]]
REFUSED = [n for n in TABLE if "refused" in TABLE[n][3]]
TRIPS = ("trips_small", "trips_tall", "trips_ordering")
WRAPPER_CASES = ("k_exact", "sel_deep", "cut_257")          # distinct |llr| in every shot: the host argsort of decoding/osd.py has no tie to break
_CASES, _MODEL, _ORACLE = {}, {}, {}


def case(name):
    if name not in _CASES:
        build, order, maxc, expect, note = TABLE[name]
        H, synd, llr, hard, ordering = build()
        ip, ix, _ = _csr_of(H)
        _CASES[name] = SimpleNamespace(name=name, H=H, m=H.shape[0], n=H.shape[1], indptr=ip, indices=ix, order=order, maxc=maxc, expect=expect, note=note,
                                       synd=np.ascontiguousarray(synd, np.int8), llr=np.ascontiguousarray(llr, np.float64),
                                       hard=np.ascontiguousarray(hard, np.int8), ordering=ordering, B=len(synd),
                                       refused=expect.get("refused"), modelled=expect.get("tested") is None or expect["tested"] <= MODEL_MAX)
    return _CASES[name]


def _csr_of(H):
    r, c = np.nonzero(H)
    ip, ix = OS._csr(r.astype(np.int64), c.astype(np.int64), H.shape[0])
    return ip, ix, H.shape[1]


def model_answers(name, mistake=None):
    """(solutions, records) of the model on the case, computed once per (case, mistake) and left unchanged"""
    import osdw_model as M
    if (name, mistake) not in _MODEL:
        c = case(name)
        _MODEL[name, mistake] = M.osdw_batch(c.H, c.synd, c.llr, c.hard, c.order, c.maxc, c.ordering, mistake, GRID)
    return _MODEL[name, mistake]


def oracle_answers(orc, name):
    if name not in _ORACLE:
        c = case(name)
        _ORACLE[name] = np.stack([orc.osdw(c.indptr, c.indices, c.n, c.synd[b], c.llr[b], c.hard[b], c.order, c.maxc,
                                           None if c.ordering is None else c.ordering[b]) for b in range(c.B)])
    return _ORACLE[name]
