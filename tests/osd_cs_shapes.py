"""Seeded matrices, shots and weights for OSD-CS (qldpc_osdcs_batch, qldpc_osdcs_batch_dev) over every shape, sort form and order it accepts.
tests/test_osd_cs_domain_cpu.py checks with the numpy model alone that the cases have the properties they are named for and holds the mirror below against
the library's own layout (osd_cs_layout, csrc/osd_plan.h); tests/test_osd_cs_domain_gpu.py runs them.  Plain module (no pytest hooks); deterministic.

The matrices come from the builders of tests/osd_shapes.py (a family of the same name is the same matrix there and here), the shot classes too (without the
explicit ordering, which OSD-CS does not take); what is added here: three kinds of matrix, three classes of shot aimed at the winner of the sweep, three sets
of weights.  `cs_layout` restates the library's layout rule in plain arithmetic: an independent statement, not a copy the library reads.  A family's labels
(sort form at each of its orders, threads, row words, GF(2) rank, non-pivot columns) are written in TABLE by hand."""
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np

import osd_cs_model as M
import osd_shapes as OS

SHOTS = 2                          # per class; 1 on the families of FEW_SHOTS (the model walks all n columns of a shot twice)
BIG_BATCH = 600                    # more shots than the 512 workgroups of the grid
BIG_FAMILY = "m65x150"
OWN_CLASSES = ("settled", "single wins", "pair wins")
WEIGHT_SETS = ("priors", "equal", "mixed")
EDGE_ORDERS, BIG_ORDERS, MAX_ORDER = (0, 1, 2, 7, 64), (7, 64), 64
UNSUPPORTED_TEXT = "OSD-CS supports m <= 1024 and n <= 65535"

# ---------------------------------------------------------------------------------------------------------------- the mirror
CHUNK = 64                         # kCsChunk: columns per chunk of the sweep


def cs_offsets(m, n, order, global_sort):
    """byte offsets of the pieces behind U (usedw, pvcol, pvrow, R, TR, pflag, misc) and the total, for one sort form"""
    mw = (m + 63) // 64
    u = (m + 2) * mw * 8
    off = OS._ru(u if global_sort else max(u, n * 12 + 16 + OS.SORT_CNT), 16)          # U, aliased by the sort scratch in the LDS form
    at = []
    for size in (16 * 8, OS._ru(2 * m, 8), OS._ru(2 * m, 8), CHUNK * mw * 8, max(order, 1) * mw * 8, OS._ru((n + 31) // 32 * 4, 16), 2048):
        at.append(off)
        off += size
    return at, off + 16


def cs_layout(m, n, order):
    """-> (lds_bytes, global_sort, block): the dynamic LDS of osd_cs_kernel, whether its column sort runs in global memory, its threads.
    The LDS sort is taken while its layout fits 160 KiB; global_sort is None (lds_bytes 0) if neither form fits."""
    for global_sort in (False, True):
        total = cs_offsets(m, n, order, global_sort)[1]
        if total <= OS.LDS_MAX:
            return total, global_sort, OS._wide_block(m)
    return 0, None, OS._wide_block(m)


def cs_accepts(m, n):
    """osdcs_supported: the size limits, and the layout at the largest order"""
    return m <= 1024 and n <= 65535 and cs_layout(m, n, MAX_ORDER)[1] is not None


def n_edge(m, order):
    """the largest n whose sort still runs in LDS"""
    return OS.largest(lambda n: cs_layout(m, n, order)[1] is False, 1, 65535)


N_CS_130_0, N_CS_1024_0, N_CS_1024_64 = n_edge(130, 0), n_edge(1024, 0), n_edge(1024, 64)
N_CS_MID = 10600                   # between the order-64 and the order-0 edge at m = 1024

# ---------------------------------------------------------------------------------------------------------------- the families
# name: (kind, m, n, extra, orders, sort form at each of them (L: in LDS, G: in global memory), threads, row words, GF(2) rank, non-pivot columns, what it
# reaches).  Kinds of osd_shapes.build_matrix, and here: "ones" a single row of random entries; "dupcol" a "dep" matrix of n - 1 columns and column 0 again
# at the end; "identfirst" an "ident" matrix whose shots have the |llr| of the identity columns scaled down to the front of the order.
E, B = EDGE_ORDERS, BIG_ORDERS
TABLE = {
    # row words and workgroup sizes: osd_wide_block gives 256 threads up to m = 254, m + 2 in whole waves up to 958, 1024 from 959
    "m1x70": ("ones", 1, 70, None, E, "LLLLL", 256, 1, 1, 69, "one row: one word with one bit used"),
    "m63x150": ("dep", 63, 150, None, E, "LLLLL", 256, 1, 62, 88, "one word, short by a bit"),
    "m64x150": ("dep", 64, 150, None, E, "LLLLL", 256, 1, 61, 89, "m % 64 == 0 in the only word"),
    "m65x150": ("dep", 65, 150, None, E, "LLLLL", 256, 2, 64, 86, "one row in the second word"),
    "s128x1024": ("dep", 128, 1024, None, E, "LLLLL", 256, 2, 127, 897, "m % 64 == 0 at two words"),
    "s129x1024": ("dep", 129, 1024, None, E, "LLLLL", 256, 3, 128, 896, "one row in the third word"),
    "m254": ("dep", 254, 640, None, E, "LLLLL", 256, 4, 252, 388, "m + 2 == 256 threads: 16 groups of 16 lanes"),
    "m255": ("dep", 255, 640, None, E, "LLLLL", 320, 4, 253, 387, "first 320-thread workgroup: 20 groups, 5 waves in the sort and the minimum"),
    "m958": ("dep", 958, 2400, None, B, "LL", 960, 15, 957, 1443, "960 threads, 15 words"),
    "m959": ("dep", 959, 2400, None, B, "LL", 1024, 15, 957, 1443, "first 1024-thread workgroup"),
    "m960": ("dep", 960, 2400, None, B, "LL", 1024, 15, 958, 1442, "m % 64 == 0 at the last of 15 words"),
    "m961": ("dep", 961, 2400, None, B, "LL", 1024, 16, 956, 1444, "16 words: every lane of a group holds one"),
    "m1022": ("dep", 1022, 2560, None, B, "LL", 1024, 16, 1016, 1544, "m + 2 == 1024 threads"),
    "m1023": ("dep", 1023, 2560, None, B, "LL", 1024, 16, 1022, 1538, "m + 2 > 1024 threads: the rhs row has no group of its own in phase C"),
    "m1024": ("dep", 1024, 2560, None, B, "LL", 1024, 16, 1022, 1538, "m % 64 == 0 at 16 words and m + 2 > 1024; 2016 pairs at order 64, TR of 64 x 16 words"),
    "ident1024": ("ident", 1024, 2524, None, B, "LL", 1024, 16, 1024, 1500, "full row rank at m = 1024: every row of the last word pivots"),
    "ident192": ("ident", 192, 592, None, E, "LLLLL", 256, 3, 192, 400, "full row rank at m % 64 == 0"),
    # the sort form: 12 n bytes of sort scratch beside the rest of the layout, TR carved per order
    "cs130_nfit": ("dep", 130, N_CS_130_0, None, E, "LLGGG", 256, 3, 129, N_CS_130_0 - 129, "the largest n sorted in LDS at m = 130, order 0 (and 1)"),
    "cs130_nover": ("dep", 130, N_CS_130_0 + 1, None, E, "GGGGG", 256, 3, 129, N_CS_130_0 - 128, "one column more: the sort in global memory at every order"),
    "cs1024_nfit": ("dep", 1024, N_CS_1024_64, None, B, "LL", 1024, 16, 1023, N_CS_1024_64 - 1023, "the largest n sorted in LDS at m = 1024, order 64"),
    "cs1024_nover": ("dep", 1024, N_CS_1024_64 + 1, None, B, "LG", 1024, 16, 1023, N_CS_1024_64 - 1022, "one column more: global at order 64, LDS at 7"),
    "cs1024_mid": ("dep", 1024, N_CS_MID, None, (0, 64), "LG", 1024, 16, 1023, N_CS_MID - 1023, "between the two edges: one handle takes both forms"),
    "u200x65534": ("dep", 200, 65534, None, B, "GG", 256, 4, 199, 65335, "the largest n of the OSD-0 row-transform kernels behind the redo list"),
    "u129x65535": ("dep", 129, 65535, None, B, "GG", 256, 3, 128, 65407, "the largest n: the redo list goes to OSD-0's global kernel"),
    # scoring edges
    "tall300x40": ("dep", 300, 40, None, E, "LLLLL", 320, 5, 40, 0, "rank == n: no non-pivot column, lambda = 0"),
    "tall300x41": ("dupcol", 300, 41, None, E, "LLLLL", 320, 5, 40, 1, "exactly one non-pivot column: one single, no pair at any order"),
    "empty130x20": ("empty", 130, 20, None, E, "LLLLL", 256, 3, 0, 20, "rank 0: the sweep loop never runs, every column is a single of delta q"),
    "halfdup256": ("halfdup", 256, 600, None, E, "LLLLL", 320, 4, 128, 472, "rank m / 2 at m % 64 == 0: half the rows never pivot"),
    "doubled200": ("doubled", 200, 600, None, E, "LLLLL", 256, 4, 188, 412, "every column twice: a single of delta 0 beside every pivot"),
    "h300_gj": ("heavy", 300, 700, OS.D_GJ_300, E, "LLLLL", 320, 5, 299, 401, "one column of degree 63: col_rows padded to 63 entries everywhere"),
    "h300_d290": ("heavy", 300, 700, 290, E, "LLLLL", 320, 5, 299, 401, "one column of degree 290"),
    "identfirst192": ("identfirst", 192, 592, None, E, "LLLLL", 256, 3, 192, 400, "three chunks in which all 64 columns pivot, then rank reached"),
    "n63": ("dep", 40, 63, None, E, "LLLLL", 256, 1, 38, 25, "one short chunk"),
    "n64": ("dep", 40, 64, None, E, "LLLLL", 256, 1, 38, 26, "one exact chunk"),
    "n65": ("dep", 40, 65, None, E, "LLLLL", 256, 1, 39, 26, "one column into the second chunk"),
    # refused
    "r129x65536": ("dep", 129, 65536, None, (), None, 256, 3, 128, 65408, "n > 65535: QLDPC_ERR_UNSUPPORTED"),
    "m1025": ("dep", 1025, 2200, None, (), None, 1024, 17, 1015, 1185, "m > 1024: QLDPC_ERR_UNSUPPORTED"),
}
del E, B
WIDE_CLASSES = ("random syndrome", "tie runs", "non-finite llr", "single wins", "pair wins")
FEW_SHOTS = ("u200x65534", "u129x65535", "cs130_nfit", "cs130_nover", "cs1024_nfit", "cs1024_nover", "cs1024_mid", "r129x65536")
RUN = [name for name in TABLE if TABLE[name][5] is not None]
WINNER_FAMILIES = {"L": "m254", "G": "cs130_nover"}          # where the CPU module wants OSD-0, a single and a pair each to win, under every weight set
ALIAS_FAMILIES = {"L": "m255", "G": "cs130_nover"}

_FAMILIES, _SHOTS, _ELIM, _ANSWERS = {}, {}, OrderedDict(), {}


def family(name):
    if name not in _FAMILIES:
        kind, m, n, extra, orders, forms, block, mw, rank, nonpivot, note = TABLE[name]
        if kind == "ones":
            rng = OS._rng(name)
            cols = np.flatnonzero(rng.random(n) < 0.5)
            ip, ix = OS._csr(np.zeros(cols.size, np.int64), cols.astype(np.int64), 1)
            f = SimpleNamespace(name=name, kind=kind, m=m, n=n, indptr=ip, indices=ix, max_col_deg=1, null_rows=None)
        elif kind == "dupcol":
            g = OS.build_matrix(name, "dep", m, n - 1)
            r = np.repeat(np.arange(m), np.diff(g.indptr))
            c = g.indices.astype(np.int64)
            ip, ix = OS._csr(np.concatenate([r, r[c == 0]]), np.concatenate([c, np.full(int((c == 0).sum()), n - 1)]), m)
            f = SimpleNamespace(name=name, kind=kind, m=m, n=n, indptr=ip, indices=ix, max_col_deg=g.max_col_deg, null_rows=g.null_rows)
        else:
            f = OS.build_matrix(name, "ident" if kind == "identfirst" else kind, m, n, extra)
            f.kind = kind
        f.orders, f.forms, f.block, f.mw, f.rank, f.nonpivot, f.note, f.refused = orders, forms, block, mw, rank, nonpivot, note, forms is None
        f.per_class = 1 if name in FEW_SHOTS else SHOTS
        _FAMILIES[name] = f
    return _FAMILIES[name]


def model_graph(f):
    if not hasattr(f, "G"):
        f.G = M.Graph(f.indptr, f.indices, f.n)
    return f.G


# ---------------------------------------------------------------------------------------------------------------- the weights
def weights(f, wset):
    """"priors": positive and distinct; "equal": all 1.0, so the candidate index decides every tie; "mixed": signs, exact zeros and magnitudes beyond the
    +-2^40 clamp of the quantisation (3e6 * 2^20 > 2^40), all finite"""
    rng = OS._rng(f.name, 300)
    pri = rng.uniform(0.5, 6.0, f.n)
    if wset == "priors":
        return pri
    if wset == "equal":
        return np.ones(f.n)
    assert wset == "mixed"
    w, idx, k = pri.copy(), rng.permutation(f.n), max(1, f.n // 20)
    w[idx[:k]] *= -1.0
    w[idx[k:2 * k]] = 0.0
    w[idx[2 * k:2 * k + 4]] = (3e6, -3e6, 1e300, -1e300)
    return w


# ---------------------------------------------------------------------------------------------------------------- the shots
def nonpivots(f, llr):
    """the non-pivot columns of a shot in its column order: they follow from H and the order alone"""
    e = M.eliminate(model_graph(f), np.zeros(f.m, np.int8), llr, np.zeros(f.n, np.int8))
    piv = np.zeros(f.n, bool)
    piv[[j for j, _ in e["pivots"]]] = True
    return [int(j) for j in e["seq"] if not piv[j]]


def own_shots(f, cls, B):
    """The classes aimed at the winner.  An error pattern e (sparse, with every column whose "mixed" weight is negative and none of the huge positive ones:
    no candidate is lighter under any of the weight sets, barring accidents) and its syndrome.  "settled": hard = e, OSD-0 has nothing to do and is kept (under "mixed" on the shots whose e is the negative columns and nothing else);
    "single wins": hard = e but for one non-pivot column, so the single that flips it gives e back; "pair wins": but for the first two non-pivot columns
    of the order, so that pair does (from order 2 on)."""
    rng = OS._rng(f.name, 200 + OWN_CLASSES.index(cls), B)
    mixed = weights(f, "mixed")
    err = OS._sparse_rows(rng, B, f.n, int(np.clip(f.n // 25, 1, 60)))
    if cls == "settled":
        err[0::2] = 0                  # (every other shot: the negative columns alone, the lightest vector there is under "mixed")
    err[:, mixed < 0] = 1
    err[:, mixed > 1e5] = 0
    synd = OS._syndromes(f, err)
    llr = rng.normal(1.0, 3.0, (B, f.n))
    hard = err.copy()
    for b in range(B if cls != "settled" else 0):
        T = nonpivots(f, llr[b])
        pick = T[:2] if cls == "pair wins" else T[int(rng.integers(0, 8)):][:1] if len(T) > 8 else T[:1]
        hard[b, pick] ^= 1
    return SimpleNamespace(synd=synd, llr=llr, hard=hard, ordering=None)


def classes_of(f):
    """every class but the explicit ordering; at n >= 65534 (half a second of model per shot and class) those that bear on what is new there: the sort of
    65535 keys with ties and non-finite values, the redo list, candidate numbers beyond 65535"""
    every = [c for c in OS.classes_of(f) if c != "explicit ordering"] + list(OWN_CLASSES)
    return [c for c in every if c in WIDE_CLASSES] if f.n >= 65534 else every


def class_shots(f, cls, B):
    s = own_shots(f, cls, B) if cls in OWN_CLASSES else OS.class_shots(f, cls, B)
    if f.kind == "identfirst":         # the identity columns first in every order (ties and non-finite values keep their places among themselves)
        s.llr[:, f.n - f.m:] *= 2.0 ** -40
    return s


def batch(name):
    """every class of the family side by side in one call -> SimpleNamespace(cls [B], synd, llr, hard), cached and left unchanged by every user"""
    if name not in _SHOTS:
        f = family(name)
        S = {c: class_shots(f, c, f.per_class) for c in classes_of(f)}
        cat = lambda k: np.ascontiguousarray(np.concatenate([getattr(S[c], k) for c in S]))          # noqa: E731
        _SHOTS[name] = SimpleNamespace(cls=np.repeat(list(S), f.per_class), synd=cat("synd"), llr=cat("llr"), hard=cat("hard"))
    return _SHOTS[name]


def big_batch(kind):
    """BIG_BATCH shots of BIG_FAMILY: "classes" every class side by side in equal shares, "outside" all of them outside the column space"""
    f = family(BIG_FAMILY)
    if kind == "outside":
        return OS.class_shots(f, "random syndrome", BIG_BATCH)
    cs = classes_of(f)
    S = [class_shots(f, c, BIG_BATCH // len(cs)) for c in cs]
    cat = lambda k: np.ascontiguousarray(np.concatenate([getattr(x, k) for x in S]))          # noqa: E731
    return SimpleNamespace(cls=np.repeat(cs, BIG_BATCH // len(cs)), synd=cat("synd"), llr=cat("llr"), hard=cat("hard"))


# ---------------------------------------------------------------------------------------------------------------- the model's answers
def eliminate_all(f, synd, llr, hard):
    """M.eliminate of every shot, one after the other: the model is short numpy calls under the interpreter lock, and a pool of 2 or 8 threads took
    twice as long as none (measured at 1024 x 2560 and 200 x 65534)"""
    G = model_graph(f)
    return [M.eliminate(G, synd[b], llr[b], hard[b]) for b in range(synd.shape[0])]


def eliminations(name):
    """the eliminations of batch(name): they know neither weights nor order, so every (weight set, order) scores the same ones.  Those of the last two
    families are kept (a shot's reduced columns are up to 13 MB)."""
    if name not in _ELIM:
        s = batch(name)
        _ELIM[name] = eliminate_all(family(name), s.synd, s.llr, s.hard)
        while len(_ELIM) > 2:
            _ELIM.popitem(last=False)
    return _ELIM[name]


def scored(f, elims, w, order):
    """M.score of every elimination -> (solution int8 [B, n], flips int32 [B, 2], outside bool [B], osd0 int8 [B, n], cost int64 [B]); rows of outside
    shots hold the model's OSD-0 solution (the library's answer there is qldpc_osd0_batch's, which the caller asks for) and cost 0"""
    B, G = len(elims), model_graph(f)
    sol, flips, out = np.zeros((B, f.n), np.int8), np.full((B, 2), -1, np.int32), np.zeros(B, bool)
    osd0, cost = np.zeros((B, f.n), np.int8), np.zeros(B, np.int64)
    for b, e in enumerate(elims):
        r = M.score(G, e, w, order)
        out[b], osd0[b] = r["outside"], r["osd0"]
        sol[b] = r["osd0"] if r["outside"] else r["solution"]
        if not r["outside"]:
            flips[b], cost[b] = r["flips"], r["cost"]
    return sol, flips, out, osd0, cost


def answers(name, wset):
    """{order: scored(..)} of batch(name) under one weight set, computed once and left unchanged"""
    if (name, wset) not in _ANSWERS:
        f = family(name)
        w = weights(f, wset)
        _ANSWERS[name, wset] = {order: scored(f, eliminations(name), w, order) for order in f.orders}
    return _ANSWERS[name, wset]


def winners(flips, outside):
    """-> the kinds of winner among the shots inside the column space: "osd0", "single", "pair" """
    fl = flips[~outside]
    return {"osd0": int(((fl[:, 0] < 0) & (fl[:, 1] < 0)).sum()), "single": int(((fl[:, 0] >= 0) & (fl[:, 1] < 0)).sum()), "pair": int((fl[:, 1] >= 0).sum())}
