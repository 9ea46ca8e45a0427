"""Seeded matrices and shots for OSD-0 (qldpc_osd0_batch) over every kernel form its dispatch can reach and both sides of every boundary between them.
tests/test_osd_domain_cpu.py checks with the oracle alone that the cases have the properties they are named for and pins the mirror below at
hand-computed points; tests/test_osd_domain_gpu.py runs them and asserts after every call that qldpc_osd0_last_path reports the labelled kernel.
Plain module (no pytest hooks); deterministic from SEED.

`rule_path` restates the library's rule -- osd0_plan and the three LDS layouts of csrc/osd_plan.h, which osd0_listed_launch (csrc/gf2.hip) executes; DESIGN.md 4
has it as a table -- in plain arithmetic: an independent statement of it, not a copy the library reads (tests/test_osd_plan_cpu.py holds the two
against each other over the whole range).  A family's label (`path`, `w16`, `rank`) is written in TABLE by hand; the CPU module asserts that the mirror
and the oracle agree with it, the GPU module that the library does.  ("plan_osd_lds' mode 2" in a TABLE note is mode 2 of the reference-order kernel:
`reforder_lds(.., 2)` here, osd_ref_layout in the library.)"""
from types import SimpleNamespace

import numpy as np

SEED = 20261019
SHOTS = 6                          # per class
BIG_BATCH = 600                    # more shots than the 512 workgroups of an OSD-0 grid
CLASSES = ("sparse error", "hard solves", "all zero", "random syndrome", "constant |llr|", "tie runs", "non-finite llr", "explicit ordering")
FLAG_OSD_LDS, FLAG_OSD_REFORDER, FLAG_OSD_UG, FLAG_OSD_GLOBAL = 0x20000, 0x80000, 0x400, 0x800
FLAG_SETS = (FLAG_OSD_REFORDER, FLAG_OSD_UG, FLAG_OSD_UG | FLAG_OSD_REFORDER, FLAG_OSD_GLOBAL, FLAG_OSD_LDS)
UNSUPPORTED_TEXT = "matrix too large for the LDS scratch"

# ---------------------------------------------------------------------------------------------------------------- the mirror
LDS_MAX = 160 * 1024               # what every OSD-0 launcher allows itself of the CU's LDS
ELIM_MAX = 150 * 1024              # kOsdElimMax (csrc/osd_plan.h): the global kernel's LDS scratch
CHUNK = 1024                       # P.K: columns per chunk
BLOCK_COLS = 16                    # kGjBlock and kOsdBlock (csrc/osd_plan.h)
SORT_CNT = 256 * 16 * 4 + 16 * 4 + 64


def _ru(x, a):
    return (x + a - 1) // a * a


def gj_lds(m, n, cd):
    """dynamic LDS of osd0_gj_kernel: osd_gj_layout, csrc/osd_plan.h"""
    mw = (m + 63) // 64
    off = _ru(max((m + 2) * mw * 8, n * 12 + 16 + SORT_CNT), 16)            # U, aliased by the sort scratch
    off += CHUNK * 2 + CHUNK + _ru(CHUNK * cd * 2, 8)                       # sidx, alive, colrows
    off += 2 * _ru(m * 2, 8)                                                # pvcol, pvrow
    off += 3 * BLOCK_COLS * mw * 8 + 32 * 8 + (4 + 5 * BLOCK_COLS + 8) * 4  # R + Cb, usedw, blk
    off += _ru((m + 2) * 4, 16)                                             # tlist
    return off + 16


def gjg_lds(m, n, cd):
    """dynamic LDS of osd0_gjg_kernel: osd_gjg_layout, csrc/osd_plan.h (n does not enter: the sort scratch is in global memory)"""
    mw = (m + 63) // 64
    off = _ru(SORT_CNT, 16)
    off += CHUNK * 2 + CHUNK + _ru(CHUNK * cd * 2, 8)
    off += 2 * _ru(m * 2, 8)
    off += BLOCK_COLS * mw * 8 + 128 * 8 + (4 + 2 * BLOCK_COLS + 4) * 4
    return off + 16


def reforder_lds(m, n, cd, mode):
    """dynamic LDS of osd0_lds_kernel<mode == 2>: osd_ref_layout, csrc/osd_plan.h"""
    mw = (m + 63) // 64
    off = _ru(max((m + 2) * mw * 8, n * 12 + 16 + SORT_CNT), 16) if mode == 1 else 0
    off += CHUNK * 2 + CHUNK + CHUNK * cd * 2
    off += _ru(m * 2, 8)
    off += BLOCK_COLS * mw * 8 + (4 + 6 * BLOCK_COLS + 4) * 4 + 64
    off += SORT_CNT if mode == 2 else 0
    return off + 16


def plan_mode(m, n, cd, flags):
    """the reference-order form osd0_plan (csrc/osd_plan.h) settles on -> 0 (no reference-order form), 1 (row transform in LDS), 2 (in HBM / L2)"""
    if m > 4096 or n >= 65535 or m < 1:
        return 0
    for mode in ((1, 2) if m <= 1024 and not flags & FLAG_OSD_UG else (2,)):
        if reforder_lds(m, n, cd, mode) <= LDS_MAX:
            return mode
    return 0


def elim_lds(m, n):
    """elim_lds_bytes with the row words osd_global_nwords, csrc/osd_plan.h"""
    nwords = ((n + 7) // 8 + 7) // 8
    return 16 + nwords * 8 + m * 4 + 8 + m + 16


def _wide_block(m):
    return min(1024, _ru(max(m + 2, 256), 64))           # osd_wide_block, csrc/osd_plan.h


def rule_path(m, n, max_col_deg, flags=0):
    """-> SimpleNamespace(path, w16, block, mode, redo, refused): the kernel that is given every shot ("SMALL", "GJ", "GJG", "REFORDER_LDS", "REFORDER_UG",
    "GLOBAL", or "NONE" with refused = True), whether GJ runs its <W16 = true> form, the threads per workgroup, the reference-order form planned (the
    low bits of qldpc_osd0_last_path's detail) and whether a second launch is queued behind a free-pivot kernel (QLDPC_OSD_DETAIL_REDO)."""
    cd = max(max_col_deg, 1)
    out = SimpleNamespace(path="NONE", w16=False, block=0, mode=0, redo=False, refused=False)
    if m < 1 or n < 1:
        return out
    if not flags & (FLAG_OSD_LDS | FLAG_OSD_UG | FLAG_OSD_GLOBAL) and m <= 128 and n <= 1024:       # osd0_plan: the one-wave kernel
        out.path, out.block = "SMALL", 64
        return out
    took = None
    if not flags & (FLAG_OSD_REFORDER | FLAG_OSD_GLOBAL):                                           # osd0_plan: the free-pivot kernels
        if not flags & FLAG_OSD_UG and m <= 1024 and n < 65535 and gj_lds(m, n, cd) <= LDS_MAX:     # GJ: m <= 1024, osd_gj_layout fits
            took = "GJ"
        if took is None and m <= 4096 and n < 65535 and gjg_lds(m, n, cd) <= LDS_MAX:               # GJG: m <= 4096, osd_gjg_layout fits
            took = "GJG"
    out.mode = 0 if flags & FLAG_OSD_GLOBAL else plan_mode(m, n, cd, flags)
    if took:
        out.path, out.redo = took, True          # (mode 0 cannot happen here: both free-pivot layouts are larger than the reference-order kernel's mode 2)
        out.block = _wide_block(m) if took == "GJ" else 1024
        out.w16 = took == "GJ" and (m + 63) // 64 == 16 and out.block == 1024                       # Osd0Plan::w16
    elif out.mode:
        out.path = "REFORDER_LDS" if out.mode == 1 else "REFORDER_UG"
        out.block = _wide_block(m) if out.mode == 1 else 1024
    elif elim_lds(m, n) > ELIM_MAX:
        out.refused = True
    else:
        out.path, out.block = "GLOBAL", 1024 if m >= 512 or n >= 2048 else 256                      # osd0_plan: the global kernel's threads
    return out


def largest(pred, lo, hi):
    """the largest x in [lo, hi] with pred(x), for a pred that holds up to some x and never after; pred(lo) must hold and pred(hi) must not"""
    assert pred(lo) and not pred(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if pred(mid) else (lo, mid)
    return lo


# the computed edges of the families below (column weight 2-4 everywhere but in the one heavy column)
N_GJ_200 = largest(lambda n: gj_lds(200, n, 4) <= LDS_MAX, 1, 65534)
N_GJ_1008 = largest(lambda n: gj_lds(1008, n, 4) <= LDS_MAX, 1, 65534)
D_GJ_300 = largest(lambda d: gj_lds(300, 700, d) <= LDS_MAX, 4, 297)
D_GJG_300 = largest(lambda d: gjg_lds(300, 700, d) <= LDS_MAX, 4, 297)
D_UG_300 = largest(lambda d: reforder_lds(300, 700, d, 2) <= LDS_MAX, 4, 297)
D_GJ_1008 = largest(lambda d: gj_lds(1008, 2500, d) <= LDS_MAX, 4, 1000)

# ---------------------------------------------------------------------------------------------------------------- the families
# name: (kind, m, n, extra, path, W16 form, GF(2) rank, what it reaches).  Kinds (see _build): "dep" sparse random columns of weight 2-4 with one row
# the sum of two others; "heavy" the same with column 0 replaced by one of degree `extra`; "doubled" every column of a "dep" matrix twice; "ident"
# random columns followed by an identity block; "empty" no entries; "halfdup" rows m/2 .. m-1 copies of rows 0 .. m/2-1; "plain" random columns only.
TABLE = {
    # the one-wave kernel's edge: m <= 128 && n <= 1024
    "s128x1024": ("dep", 128, 1024, None, "SMALL", False, 127, "last matrix of the one-wave kernel"),
    "s129x1024": ("dep", 129, 1024, None, "GJ", False, 128, "one row too many for it; 64 rows + 1 in the third word"),
    "s128x1025": ("dep", 128, 1025, None, "GJ", False, 127, "one column too many for it; m % 64 == 0"),
    # osd_gj: workgroup sizes (256 threads up to m = 254, 1024 from m = 959), row words (15 -> 16 at m = 961), m + 2 > 1024 threads
    "m254": ("dep", 254, 640, None, "GJ", False, 252, "m + 2 == 256 threads"),
    "m255": ("dep", 255, 640, None, "GJ", False, 253, "first 320-thread workgroup"),
    "m958": ("dep", 958, 2400, None, "GJ", False, 957, "960 threads, 15 words"),
    "m959": ("dep", 959, 2400, None, "GJ", False, 957, "first 1024-thread workgroup, 15 words: the non-W16 form at 1024 threads"),
    "m960": ("dep", 960, 2400, None, "GJ", False, 958, "m % 64 == 0: a full last word, 15 words"),
    "m961": ("dep", 961, 2400, None, "GJ", True, 956, "first W16 matrix: one row in the 16th word"),
    "m1022": ("dep", 1022, 2560, None, "GJ", True, 1016, "m + 2 == 1024 threads"),
    # (m1023 is the regression case of the W16 kernel's overlapped row updates: they gave rows to lanes as q = 16 * lane + .. <= 1023 and so never
    #  reached the right-hand side row m + 1 = 1024; m1024 and ident1024 have it at 1025)
    "m1023": ("dep", 1023, 2560, None, "GJ", True, 1022, "m + 2 > 1024 threads: the rhs row has no thread of its own"),
    "m1024": ("dep", 1024, 2560, None, "GJ", True, 1022, "last W16 matrix: m % 64 == 0 and m + 2 > 1024 threads"),
    # osd_gjg at its natural sizes
    "m1025": ("dep", 1025, 2200, None, "GJG", False, 1015, "first matrix beyond osd_gj: 17 words"),
    "m2048": ("dep", 2048, 3000, None, "GJG", False, 1988, "m % 64 == 0, 32 words"),
    "m4095": ("dep", 4095, 5000, None, "GJG", False, 3862, "64 words, the last one short by a bit"),
    "m4096": ("dep", 4096, 5000, None, "GJG", False, 3867, "last matrix of osd_gjg: m % 64 == 0"),
    "m4097": ("dep", 4097, 5000, None, "GLOBAL", False, 3896, "first matrix beyond every row-transform kernel"),
    # 12 n bytes of sort scratch push osd_gj out of LDS
    "m200_nfit": ("dep", 200, N_GJ_200, None, "GJ", False, 199, "the largest n osd_gj takes at m = 200"),
    "m200_nover": ("dep", 200, N_GJ_200 + 1, None, "GJG", False, 199, "one column more: osd_gjg at m <= 1024"),
    "m1008_nfit": ("dep", 1008, N_GJ_1008, None, "GJ", True, 1007, "the largest n osd_gj takes at the production m"),
    "m1008_nover": ("dep", 1008, N_GJ_1008 + 1, None, "GJG", False, 1007, "one column more"),
    # the end of the uint16 column tables
    "u200x65534": ("dep", 200, 65534, None, "GJG", False, 199, "the largest n of the row-transform kernels"),
    "u129x65535": ("dep", 129, 65535, None, "GLOBAL", False, 128, "n == 65535 is the uint16 tables' pad value: global kernel"),
    # 2048 bytes of chunk supports per unit of max_col_deg
    "h300_gj": ("heavy", 300, 700, D_GJ_300, "GJ", False, 299, "the heaviest column osd_gj takes at m = 300"),
    "h300_gj1": ("heavy", 300, 700, D_GJ_300 + 1, "GJG", False, 298, "one more: osd_gjg"),
    "h300_gjg": ("heavy", 300, 700, D_GJG_300, "GJG", False, 298, "the heaviest column osd_gjg takes"),
    "h300_gjg1": ("heavy", 300, 700, D_GJG_300 + 1, "REFORDER_UG", False, 298, "one more: only plan_osd_lds' mode 2 still fits, every shot in reference order"),
    "h300_ug1": ("heavy", 300, 700, D_UG_300 + 1, "GLOBAL", False, 298, "one more than that takes: the global kernel"),
    "h1008_gj1": ("heavy", 1008, 2500, D_GJ_1008 + 1, "GJG", False, 1006, "production m with a column one above osd_gj's 160 KiB"),
    # degenerate shapes
    "tiny130x9": ("dep", 130, 9, None, "GJ", False, 9, "fewer columns than one 16-column block"),
    "tall300x40": ("dep", 300, 40, None, "GJ", False, 40, "tall: rank == n, the sweep runs out of columns"),
    "doubled200": ("doubled", 200, 600, None, "GJ", False, 188, "every column twice: dependent columns dropped in batches"),
    "ident1024": ("ident", 1024, 2524, None, "GJ", True, 1024, "full row rank at m % 64 == 0: every row of the last word pivots (W16)"),
    "ident192": ("ident", 192, 592, None, "GJ", False, 192, "full row rank at m % 64 == 0 (non-W16)"),
    "empty130x20": ("empty", 130, 20, None, "GJ", False, 0, "rank 0: no sweep at all"),
    "halfdup256": ("halfdup", 256, 600, None, "GJ", False, 128, "half the rows duplicated: rank about m / 2, m % 64 == 0"),
    # the global kernel's own edge, then beyond everything
    "m30710": ("plain", 30710, 64, None, "GLOBAL", False, 64, "largest scratch the literal elimination accepts"),
    "refused": ("plain", 30720, 64, None, "NONE", False, 64, "elim_lds_bytes > 150 KiB: QLDPC_ERR_UNSUPPORTED, no kernel"),
}
# the families whose label depends on a flag somewhere (every kind of boundary, both sides): run again under FLAG_SETS
FLAG_FAMILIES = ("s128x1024", "s129x1024", "s128x1025", "m254", "m255", "m958", "m959", "m960", "m961", "m1022", "m1023", "m1024", "m1025", "m2048",
                 "m4095", "m4096", "m200_nfit", "m200_nover", "m1008_nfit", "m1008_nover", "u200x65534", "h300_gj", "h300_gj1", "h300_gjg",
                 "h300_gjg1", "h1008_gj1")
PRESORT_FAMILIES = ("m961", "m1024", "m1025", "m4096")
# no test carries the n >= 65534 cases together with the m >= 4096 ones
GROUPS = {"wide": ("u200x65534", "u129x65535"), "tall": ("m4095", "m4096", "m4097")}

_FAMILIES, _SHOTS = {}, {}


def _rng(name, *what):
    return np.random.default_rng([SEED] + [ord(ch) for ch in name] + [int(w) for w in what])


def _columns(rng, rows, n, wmin, wmax):
    """n random columns over the row ids `rows`, weight uniform in wmin .. wmax, no repeated entry -> (row, column) coordinate arrays"""
    w = rng.integers(wmin, wmax + 1, n)
    R = rng.integers(0, len(rows), (n, wmax))
    while True:
        S = np.sort(R, axis=1)
        bad = np.flatnonzero((S[:, 1:] == S[:, :-1]).any(axis=1))
        if bad.size == 0:
            break
        R[bad] = rng.integers(0, len(rows), (bad.size, wmax))
    keep = np.arange(wmax)[None, :] < w[:, None]
    cols = np.broadcast_to(np.arange(n)[:, None], R.shape)
    return np.asarray(rows)[R[keep]], cols[keep]


def _csr(r, c, m):
    order = np.lexsort((c, r))
    r, c = r[order], c[order]
    assert r.size == 0 or not ((r[1:] == r[:-1]) & (c[1:] == c[:-1])).any()
    indptr = np.zeros(m + 1, np.int64)
    np.add.at(indptr, r + 1, 1)
    return np.cumsum(indptr).astype(np.int32), c.astype(np.int32)


def _build(name):
    path, w16, rank, note = TABLE[name][4:]
    return SimpleNamespace(**vars(build_matrix(name, *TABLE[name][:4])), path=path, w16=w16, rank=rank, note=note, refused=path == "NONE")


def build_matrix(name, kind, m, n, extra=None):
    """the matrix of a family without its labels (tests/osd_cs_shapes.py builds its own families with this): seeded by the name"""
    rng = _rng(name)
    null_rows = None
    if kind in ("dep", "heavy", "doubled"):
        n0 = n // 2 if kind == "doubled" else n
        a, b, dep = (int(x) for x in rng.choice(m, 3, replace=False))
        r, c = _columns(rng, np.setdiff1d(np.arange(m), [dep]), n0, 2, 3)
        if kind == "heavy":                  # column 0 becomes the heavy one, clear of the three rows of the dependency
            keep = c != 0
            hr = rng.permutation(np.setdiff1d(np.arange(m), [a, b, dep]))[:extra]
            r, c = np.concatenate([r[keep], hr]), np.concatenate([c[keep], np.zeros(extra, np.int64)])
        both = np.setxor1d(c[r == a], c[r == b])                      # row dep = row a + row b: column weights 2 .. 4
        r, c = np.concatenate([r, np.full(both.size, dep)]), np.concatenate([c, both])
        if kind == "doubled":
            r, c = np.concatenate([r, r]), np.concatenate([2 * c, 2 * c + 1])
        null_rows = (a, b, dep)
    elif kind == "ident":
        r, c = _columns(rng, np.arange(m), n - m, 2, 4)
        r, c = np.concatenate([r, np.arange(m)]), np.concatenate([c, n - m + np.arange(m)])
    elif kind == "empty":
        r, c = np.zeros(0, np.int64), np.zeros(0, np.int64)
        null_rows = (0,)
    elif kind == "halfdup":
        r, c = _columns(rng, np.arange(m // 2), n, 1, 2)
        r, c = np.concatenate([r, r + m // 2]), np.concatenate([c, c])
        null_rows = (0, m // 2)
    else:
        assert kind == "plain"
        r, c = _columns(rng, np.arange(m), n, 2, 4)
    ip, ix = _csr(np.asarray(r, np.int64), np.asarray(c, np.int64), m)
    cdeg = int(np.bincount(ix, minlength=n).max()) if ix.size else 0
    return SimpleNamespace(name=name, kind=kind, m=m, n=n, indptr=ip, indices=ix, max_col_deg=cdeg, null_rows=null_rows)


def family(name):
    if name not in _FAMILIES:
        _FAMILIES[name] = _build(name)
    return _FAMILIES[name]


def matrix(f):
    """scipy CSR of the family's H (int32 entries)"""
    from scipy.sparse import csr_matrix
    return csr_matrix((np.ones(f.indices.size, np.int32), f.indices, f.indptr), shape=(f.m, f.n))


def dense(f):
    return np.asarray(matrix(f).todense(), dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------- the shots
def _sparse_rows(rng, B, n, k):
    out = np.zeros((B, n), np.int8)
    for b in range(B):
        out[b, rng.choice(n, min(k, n), replace=False)] = 1
    return out


def _syndromes(f, E):
    return np.asarray((matrix(f) @ E.T.astype(np.int32)) % 2, dtype=np.int8).T.copy() if f.indices.size else np.zeros((E.shape[0], f.m), np.int8)


def outside(f, synd):
    """bool [B]: the syndrome is outside the column space of H by the family's own witness (rows whose sum over GF(2) is the zero row)"""
    return synd[:, list(f.null_rows)].sum(axis=1) % 2 == 1


def class_shots(f, cls, B=SHOTS):
    """the shots of one class -> SimpleNamespace(synd int8 [B, m], llr f64 [B, n], hard int8 [B, n], ordering int32 [B, n] or None)"""
    ci = CLASSES.index(cls)
    rng = _rng(f.name, 100 + ci, B)
    m, n = f.m, f.n
    k_err, k_hard = int(np.clip(n // 25, 1, 60)), int(np.clip(n // 10, 1, 200))
    E = _sparse_rows(rng, B, n, k_err)
    synd = _syndromes(f, E)
    llr = rng.normal(1.0, 3.0, (B, n))
    hard = _sparse_rows(rng, B, n, k_hard)
    ordering = None
    if cls == "hard solves":
        hard = E.copy()
    elif cls == "all zero":
        synd[:], llr[:], hard[:] = 0, 0.0, 0
    elif cls == "random syndrome":
        assert f.null_rows is not None
        synd = (rng.random((B, m)) < 0.5).astype(np.int8)
        fix = ~outside(f, synd)
        synd[fix, f.null_rows[0]] ^= 1
    elif cls == "constant |llr|":
        llr = np.where(rng.random((B, n)) < 0.5, -2.5, 2.5)
    elif cls == "tie runs":
        for b in range(B):
            if b % 2 == 0:       # keys that differ in the last mantissa bit only, against index order
                llr[b, 0::2], llr[b, 1::2] = np.nextafter(1.5, 2.0), 1.5
            else:                # a long run of keys equal in their 40 high bits, descending
                llr[b, :n // 2] = -(1.0 + np.arange(n // 2)[::-1] * 2.0 ** -45)
    elif cls == "non-finite llr":
        g = max(1, n // 40)
        for b in range(B):
            pos = rng.permutation(n)[:6 * g].reshape(6, -1) if n >= 6 * g else np.arange(6).reshape(6, 1) % n
            for vals, p in zip((np.inf, -np.inf, np.nan, -0.0, 5e-324, -1e-310), pos):
                llr[b, p] = vals
    elif cls == "explicit ordering":
        ordering = np.stack([rng.permutation(n) for _ in range(B)]).astype(np.int32)
    return SimpleNamespace(synd=synd, llr=llr, hard=hard, ordering=ordering)


def classes_of(f):
    """the classes a family carries: a random syndrome only where rank < m puts it outside the column space"""
    return [c for c in CLASSES if c != "random syndrome" or (f.null_rows is not None and f.rank < f.m)]


def shots(name):
    """-> {class: shots} of the family, cached (and left unchanged by every user)"""
    if name not in _SHOTS:
        f = family(name)
        _SHOTS[name] = {c: class_shots(f, c) for c in classes_of(f)}
    return _SHOTS[name]


def batches(name):
    """The two calls a family's shots make: every class without an ordering in one batch (the kernels meet them side by side in one grid), and the
    explicit-ordering class -> [(class of each shot, synd, llr, hard, ordering or None)]"""
    S = shots(name)
    plain = [c for c in S if S[c].ordering is None]
    cat = lambda k: np.concatenate([getattr(S[c], k) for c in plain])          # noqa: E731
    out = [(np.repeat(plain, SHOTS), cat("synd"), cat("llr"), cat("hard"), None)]
    x = S["explicit ordering"]
    out.append((np.repeat(["explicit ordering"], SHOTS), x.synd, x.llr, x.hard, x.ordering))
    return out


_WANT = {}


def oracle_osd0(orc, f, synd, llr, hard, ordering=None):
    """oracle.osd0 of every shot -> int8 [B, n]; the shots are independent, so they go to a few threads (the oracle call releases the interpreter lock)"""
    from concurrent.futures import ThreadPoolExecutor
    one = lambda b: orc.osd0(f.indptr, f.indices, f.n, synd[b], llr[b], hard[b], None if ordering is None else ordering[b])      # noqa: E731
    with ThreadPoolExecutor(max_workers=8) as ex:
        return np.stack(list(ex.map(one, range(synd.shape[0]))))


def solutions(orc, name):
    """the oracle's answers to batches(name), one array per batch: computed once, shared by every test and left unchanged"""
    if name not in _WANT:
        f = family(name)
        _WANT[name] = [oracle_osd0(orc, f, synd, llr, hard, ordering) for _, synd, llr, hard, ordering in batches(name)]
    return _WANT[name]


def honoured(f, flags_list=FLAG_SETS):
    """the flag sets that change what the mirror says of the family (kernel, reference-order form or redo), one per distinct outcome"""
    base = rule_path(f.m, f.n, f.max_col_deg)
    seen, out = {(base.path, base.mode, base.redo)}, []
    for fl in flags_list:
        r = rule_path(f.m, f.n, f.max_col_deg, fl)
        if (r.path, r.mode, r.redo) not in seen:
            seen.add((r.path, r.mode, r.redo))
            out.append(fl)
    return out
