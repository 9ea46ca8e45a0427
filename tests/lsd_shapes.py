"""Seeded matrices and shots for BP+LSD (qldpc_lsd_batch), from the builders of tests/osd_shapes.py with m <= 130 and n <= 300, and the model's answers to
them (tests/lsd_model.py), computed once per (matrix, shots, bits_per_step, max_rows), shared by every test and left unchanged.  Plain module (no pytest
hooks); deterministic from the seeds of osd_shapes.  tests/test_lsd_cpu.py checks that the special shots have the properties they are named for;
tests/test_lsd_gpu.py holds the kernel to the answers.

`layout` restates lsd_layout of csrc/lsd_plan.h in plain arithmetic: an independent statement of it, not a copy the library reads."""
from types import SimpleNamespace

import numpy as np

import lsd_model as M
import osd_shapes as S

# ---------------------------------------------------------------------------------------------------------------- the mirror of csrc/lsd_plan.h
LDS_MAX = 160 * 1024
LIST_CAP = 128


def _ru(x, a):
    return (x + a - 1) // a * a


def layout(m, n, cdeg, max_rows):
    """dynamic LDS bytes of lsd_kernel: lsd_layout, csrc/lsd_plan.h (every piece rounded up to 16 bytes)"""
    w = (max_rows + 63) // 64
    pieces = [(max_rows + 1) * w * 8,                                        # U and the reduced right-hand side
              w * 8, w * 8,                                                  # pivoted rows, the mask of the column being added
              max_rows * 8, max_rows * 4,                                    # per label: least key, least index of that key
              m * 2,                                                         # local index of a row of H
              (n + 31) // 32 * 4, (n + 31) // 32 * 4,                        # member of A, picked in this round
              max_rows * 2, max_rows * 2, max_rows * 2, max_rows * 2, max_rows * 2, max_rows * 2,      # label, cache, candidate, row of H, pivot column, last pick
              max_rows,                                                      # per label: valid / picking / out of candidates
              max(cdeg, 1) * 2,                                              # labels of the rows of the column being added
              LIST_CAP * 8, LIST_CAP * 2, LIST_CAP * 2,                      # the round's list in LDS: keys, columns, sorted columns
              64 * 4]
    return sum(_ru(p, 16) for p in pieces)


def supported(m, n, cdeg, max_rows):
    """lsd_supported: n < 65535, m <= 65535 and the layout at max_rows within 160 KiB"""
    return n < 65535 and m <= 65535 and layout(m, n, cdeg, max_rows) <= LDS_MAX


# ---------------------------------------------------------------------------------------------------------------- the matrices
MATRICES = {                         # key: (name that seeds it, kind of osd_shapes.build_matrix, m, n)
    "dep": ("lsd_dep130", "dep", 130, 300),                # sparse random columns of weight 2-4, one dependent row
    "ident": ("lsd_ident128", "ident", 128, 300),          # random columns and an identity block: every syndrome is reachable; m % 64 == 0
    "doubled": ("lsd_doubled120", "doubled", 120, 280),    # every column twice: dependent columns inside A
    "tiny": ("lsd_tiny130x9", "dep", 130, 9),              # nine columns: most rows have degree 0
}
_MATS, _ANSWERS = {}, {}


def matrix(key):
    """-> (family of osd_shapes.build_matrix, lsd_model.Graph), cached"""
    if key not in _MATS:
        f = S.build_matrix(*MATRICES[key])
        _MATS[key] = (f, M.Graph(f.indptr, f.indices, f.n))
    return _MATS[key]


def _shots(synd, llr, hard):
    return SimpleNamespace(synd=np.ascontiguousarray(synd, np.int8), llr=np.ascontiguousarray(llr, np.float64), hard=np.ascontiguousarray(hard, np.int8))


def general_on(f, G, rng, B, quick=False):
    """the mixed batch of `general` on any matrix (tests/lsd_domain_shapes.py uses it too).  quick: the columns of the error and of the hard decision are
    among the least reliable ones and no syndrome is random, so the clusters stay small and the model quick"""
    E, hard = np.zeros((B, f.n), np.int8), np.zeros((B, f.n), np.int8)
    llr = rng.normal(1.0, 3.0, (B, f.n))
    if quick:
        llr = 2.0 + np.abs(llr)
    for b in range(B):
        E[b, rng.choice(f.n, min(1 + b % 6, f.n), replace=False)] = 1
        hard[b, rng.choice(f.n, min(b % 4, f.n), replace=False)] = 1
        if b % 3 == 1:
            llr[b] = np.round(llr[b])                                        # many ties, zeros among them
            llr[b, rng.choice(f.n, min(3, f.n), replace=False)] = [np.nan, np.inf, -np.inf][:min(3, f.n)]
        if quick:
            low = np.flatnonzero(E[b] | hard[b])
            llr[b, low] = rng.choice([0.0, 0.25, 0.5, 0.5, 1.0], low.size)
            llr[b] *= rng.choice([-1.0, 1.0], f.n)
    synd = np.stack([G.parity(e) for e in E])
    for b in range(B):
        if b % 8 == 7:
            hard[b] = E[b]
        elif b % 8 == 3 and not quick:
            synd[b] = rng.random(f.m) < 0.5
    return _shots(synd, llr, hard)


def general(key, B=24, seed=0):
    """a mixed batch: sparse errors of weight 1 .. 6 over a sparse hard decision, a third of them with tied and non-finite |llr|, every eighth shot with
    zero residual (hard = the error), every eighth a random syndrome (many seeds; it may lie outside the column space)"""
    f, G = matrix(key)
    return general_on(f, G, np.random.default_rng([S.SEED, seed, B] + [ord(c) for c in key]), B)


def single_seed(key="ident"):
    """hard = 0 and a syndrome of weight one, on the first rows of degree >= 2"""
    f, G = matrix(key)
    rows = np.flatnonzero(np.diff(f.indptr) >= 2)[:6]
    rng = np.random.default_rng([S.SEED, 1] + [ord(c) for c in key])
    synd = np.zeros((rows.size, f.m), np.int8)
    synd[np.arange(rows.size), rows] = 1
    return _shots(synd, rng.normal(1.0, 3.0, (rows.size, f.n)), np.zeros((rows.size, f.n), np.int8))


def merging(key="dep"):
    """two seeds on the two (or more) rows of ONE column, which carries the least |llr| of the shot: round 1 picks it for both, and the clusters merge"""
    f, G = matrix(key)
    cols = [j for j in range(f.n) if G.rows_of(j).size >= 2][:6]
    rng = np.random.default_rng([S.SEED, 2] + [ord(c) for c in key])
    llr = 2.0 + np.abs(rng.normal(1.0, 3.0, (len(cols), f.n)))
    synd = np.zeros((len(cols), f.m), np.int8)
    for i, j in enumerate(cols):
        synd[i, G.rows_of(j)[:2]] = 1
        llr[i, j] = 0.25
    return _shots(synd, llr, np.zeros((len(cols), f.n), np.int8))


def apart(key="ident"):
    """two seeds on rows that share no column and no neighbour row, each with its identity column the least reliable one: two clusters to the end"""
    f, G = matrix(key)
    rng = np.random.default_rng([S.SEED, 3] + [ord(c) for c in key])
    first_unit = f.n - f.m                                                   # the identity block: column first_unit + r has row r only
    pairs = []
    for a in range(f.m):
        na = {int(r) for j in G.cols_of(a) for r in G.rows_of(j)}
        for b in range(a + 1, f.m):
            nb = {int(r) for j in G.cols_of(b) for r in G.rows_of(j)}
            if not na & nb:
                pairs.append((a, b))
                break
        if len(pairs) == 6:
            break
    llr = 2.0 + np.abs(rng.normal(1.0, 3.0, (len(pairs), f.n)))
    synd = np.zeros((len(pairs), f.m), np.int8)
    for i, (a, b) in enumerate(pairs):
        synd[i, [a, b]] = 1
        llr[i, [first_unit + a, first_unit + b]] = [0.5, 0.25]
    return _shots(synd, llr, np.zeros((len(pairs), f.n), np.int8))


def duplicates(key="doubled"):
    """the doubled matrix (columns 2 c and 2 c + 1 are equal): one seed whose two least reliable columns are a pair of twins -- with bits_per_step = 2
    round 1 adds both, and the second depends on the first"""
    f, G = matrix(key)
    rng = np.random.default_rng([S.SEED, 4] + [ord(c) for c in key])
    cols = [2 * c for c in range(6)]
    llr = 2.0 + np.abs(rng.normal(1.0, 3.0, (len(cols), f.n)))
    synd = np.zeros((len(cols), f.m), np.int8)
    for i, j in enumerate(cols):
        synd[i, G.rows_of(j)[0]] = 1
        llr[i, [j, j + 1]] = [0.25, -0.25]                                   # a tie in |llr| as well: the index decides
    return _shots(synd, llr, np.zeros((len(cols), f.n), np.int8))


def empty_rows(key="tiny"):
    """seeds on rows of degree 0 (alone, and beside a seed that has columns): flag 2 whatever the cap"""
    f, G = matrix(key)
    deg = np.diff(f.indptr)
    bare, full = np.flatnonzero(deg == 0), np.flatnonzero(deg > 0)
    rng = np.random.default_rng([S.SEED, 5] + [ord(c) for c in key])
    synd = np.zeros((4, f.m), np.int8)
    synd[0, bare[0]] = 1
    synd[1, [bare[1], full[0]]] = 1
    synd[2, bare[:70]] = 1                                                   # more seeds than a cap of 64 holds: still flag 2, not flag 1
    synd[3, full[0]] = 1                                                     # (and one without: whatever the nine columns make of it)
    return _shots(synd, rng.normal(1.0, 3.0, (4, f.n)), np.zeros((4, f.n), np.int8))


def answers(key, name, shots, bits_per_step, max_rows):
    """the model on `shots` -> (solution int8[B, n] -- zeros where the flag is not 0: OSD-0 answers those --, info int32[B, 4], traces), cached under
    (key, name, bits_per_step, max_rows)"""
    k = (key, name, bits_per_step, max_rows)
    if k not in _ANSWERS:
        f, G = matrix(key)
        B = shots.synd.shape[0]
        sol, info, traces = np.zeros((B, f.n), np.int8), np.zeros((B, 4), np.int32), []
        for b in range(B):
            tr = {}
            sol[b], info[b] = M.lsd(G, shots.synd[b], shots.llr[b], shots.hard[b], bits_per_step, max_rows, trace=tr, osd0=lambda *a: np.zeros(f.n, np.int8))
            traces.append(tr)
        _ANSWERS[k] = (sol, info, traces)
    return _ANSWERS[k]


def rows_per_round(trace):
    """|R| at the start of every round and at the end"""
    return [sum(rows for rows, _ in clusters) for clusters in trace["clusters"]]
