"""Seeded cases for the resident min-sum kernel (csrc/minsum_resident.hip) over every form and team shape it takes: its twelve instantiations
(<6,3,1,2>, <6,3,2,4>, <8,4,1,2>, <8,4,2,4>, each plain, with damping and as the fused Monte-Carlo kernel), irregular graphs in the
two-rows-per-thread form (ragged and empty second slices, empty rows, degree-1 checks), non-clean priors on both row slices, the limits of the plan
(256 / 257 rows, the 1024-thread team, 60 KiB per shot, S uncut and S cut by the LDS loop) and batches that send a workgroup of the 4096-group
persistent grid on a second `base`.  tests/test_resident_domain_cpu.py checks with the plan program and the oracle alone that the cases are what
they are named for; tests/test_resident_domain_gpu.py decodes them.  Plain module (no pytest hooks); deterministic from the seeds below.

plan() is a SECOND COPY of csrc/resident_plan.h and carve_end() of the kernel's pointer arithmetic, kept on purpose as independent statements: the
CPU module compares the first with the compiled header over a sweep and holds the second inside the planned LDS size.

Every irregular graph except `uncut` and `one_edge` has two empty rows, two degree-1 checks on different columns (the first and the last row, so
that the two-row form meets one in either slice), a degree-0 column and a duplicated row (rows 1 and m - 2).  `i84_m300` has a third degree-1 check
on the column of the first: pinned to opposite syndrome bits on every second shot, they send +inf and -inf into one posterior (NaN)."""
import zlib
from types import SimpleNamespace

import numpy as np

import graph_shapes as GS

SEED = 20261019
GRID_CAP = 4096                 # the persistent grid of both launchers: 256 * 2 * 8 workgroups
TEAM = 1024                     # threads of the largest team, and the budget S = TEAM // TS is cut from
SHOT_BYTES = 60 * 1024
LDS_BUDGET = 64 * 1024
SWITCH = 256                    # the largest one-row-per-thread team
MAX_ITER = 50
CLIPS = (20.0, 6.0, 1.0)
PRIOR_CLASSES = ("uniform", "normal", "negative class", "zero class", "above clip", "all zero", "subnormal", "huge")
SCALES = (0.25, 0.5, 1.0, 1.5)
FORMS = ("plain", "DAMP", "MC")
INSTANCES = ((6, 3, 1, 2), (6, 3, 2, 4), (8, 4, 1, 2), (8, 4, 2, 4))


# ---------------------------------------------------------------------------------------- the plan and the carve, restated
def plan(m, n, nnz, max_row, max_col):
    """-> None where the kernel refuses, else SimpleNamespace(inst (cdeg, vdeg, cpt, vpt), TS, S, uncut (TEAM // TS), block, idle (lanes of the
    block that belong to no team), lds, per_shot)"""
    if min(m, n, nnz) <= 0 or max_row > 8 or max_col > 4:
        return None
    cdeg, vdeg = (6, 3) if max_row <= 6 and max_col <= 3 else (8, 4)
    per_shot = 8 * (m * (cdeg + 1) + n) + 32 + 4 * -(-n // 4)
    if per_shot > SHOT_BYTES:
        return None
    cpt, ts = 1, max(m, -(-n // 2))
    if ts > SWITCH:
        cpt, ts = 2, max(-(-m // 2), -(-n // 4))
    if ts > TEAM:
        return None
    uncut = TEAM // ts
    S = max(1, min(uncut, (LDS_BUDGET - 96) // per_shot))
    block = -(-S * ts // 64) * 64
    return SimpleNamespace(inst=(cdeg, vdeg, cpt, 2 * cpt), TS=ts, S=S, uncut=uncut, block=block, idle=block - S * ts, lds=S * per_shot + 96,
                           per_shot=per_shot)


def carve_end(m, n, cdeg, S):
    """Last byte + 1 the kernel's own pointers reach in the dynamic LDS, from its pointer arithmetic: R [S][m][RST] doubles, V [S][n] doubles, flags
    (unsat[2] per team, active[2]), results [S][4] ints, then at an even int offset the logical accumulators [S] and the block tally [6] (64-bit),
    then the sampled error bytes [S][4 * nq]."""
    rst = cdeg + 1
    flags = 8 * (S * m * rst + S * n)
    lacc = flags + 4 * ((2 * S + 2 + 4 * S + 1) & ~1)
    assert lacc % 8 == 0
    tally = lacc + 8 * S
    errors = tally + 8 * 6
    return errors + S * 4 * ((n + 3) >> 2)


def detail_of(L, inst, damped):
    """the QLDPC_DETAIL_* word qldpc_minsum_decode_path reports for an instantiation (L: the bindings)"""
    return (L.DETAIL_RES_CDEG8 if inst[0] == 8 else 0) | (L.DETAIL_RES_CPT2 if inst[2] == 2 else 0) | (L.DETAIL_DAMPING if damped else 0)


# ---------------------------------------------------------------------------------------- the graphs
# name: (m, n, row cap, (column degree, count) pairs, error rate of the syndromes, expected instantiation or None where the kernel refuses, note)
TABLE = {
    "i63_m256": (256, 512, 6, ((3, 330), (2, 130), (1, 42), (0, 10)), 0.06, (6, 3, 1, 2), "last one-row team: TS 256, S 3 cut from 4, block 768"),
    "i63_m257": (257, 514, 6, ((3, 330), (2, 130), (1, 44), (0, 10)), 0.06, (6, 3, 2, 4), "first two-row team: TS 129, S 3, block 448, 61 idle lanes"),
    "i63_wide": (100, 515, 6, ((3, 70), (2, 110), (1, 120), (0, 215)), 0.06, (6, 3, 2, 4), "n alone sets TS 129: every second row slice empty; S 6"),
    "i63_tall": (600, 700, 6, ((3, 520), (2, 130), (1, 40), (0, 10)), 0.05, (6, 3, 2, 4), "m sets TS 300; S 1; block 320"),
    "i63_team1024": (438, 4096, 6, ((3, 420), (2, 480), (1, 300), (0, 2896)), 0.06, (6, 3, 2, 4), "the 1024-thread team, 16 B under 60 KiB per shot"),
    "i63_team1025": (438, 4097, 6, None, 0.06, None, "i63_team1024 plus one degree-0 column: TS 1025"),
    "i63_bytes_in": (829, 1658, 6, ((3, 1200), (2, 350), (1, 98), (0, 10)), 0.05, (6, 3, 2, 4), "74 m + 32 <= 61 440 holds"),
    "i63_bytes_out": (830, 1660, 6, None, 0.05, None, "i63_bytes_in plus one row on two new columns: 74 m + 32 > 61 440"),
    "i84_bytes_in": (682, 1364, 8, ((4, 300), (3, 700), (2, 300), (1, 54), (0, 10)), 0.05, (8, 4, 2, 4), "90 m + 32 <= 61 440 holds"),
    "i84_bytes_out": (683, 1366, 8, None, 0.05, None, "i84_bytes_in plus one row on two new columns: 90 m + 32 > 61 440"),
    "i84_m70": (70, 150, 8, ((4, 45), (3, 60), (2, 30), (1, 10), (0, 5)), 0.06, (8, 4, 1, 2), "TS 75, S 10 cut from 13"),
    "i84_bycol": (80, 150, 6, ((4, 30), (3, 70), (2, 40), (1, 5), (0, 5)), 0.06, (8, 4, 1, 2), "no row above 6, some columns 4: (8,4) by a column alone"),
    "i84_byrow": (60, 160, 7, ((3, 85), (2, 50), (1, 15), (0, 10)), 0.06, (8, 4, 1, 2), "rows to 7, columns <= 3: (8,4) by a row alone"),
    "i84_m300": (300, 590, 8, ((4, 120), (3, 300), (2, 120), (1, 40), (0, 10)), 0.06, (8, 4, 2, 4), "TS 150, S 2, block 320"),
    "i84_m511": (511, 1021, 8, ((4, 200), (3, 550), (2, 200), (1, 61), (0, 10)), 0.06, (8, 4, 2, 4), "TS 256, S 1, block exactly 256, odd m and n"),
    "uncut": (10, 200, 6, ((3, 14), (2, 6), (1, 4), (0, 176)), 0.08, (6, 3, 1, 2), "S = 1024 // TS = 10 survives the LDS loop; block 1024, 24 idle lanes"),
    "one_edge": (1, 1, 6, None, 0.3, (6, 3, 1, 2), "TS 1, S 654 cut from 1024; a lone degree-1 check"),
}
PAIRS = (("i63_team1024", "i63_team1025"), ("i63_bytes_in", "i63_bytes_out"), ("i84_bytes_in", "i84_bytes_out"))
PLAIN = ("uncut", "one_edge")                                 # no structural extras
NAN_GRAPH = "i84_m300"
FULL_GRAPHS = ("i63_m257", "i84_m70", "i84_m300", "i84_m511")   # every prior class, clip, schedule and non-clean prior
MC_GRAPHS = ("i63_m256", "i63_m257", "i84_m70", "i84_m300")
ACCEPTED = tuple(k for k, v in TABLE.items() if v[5] is not None)

_GRAPHS = {}


def _seed(name, *what):
    return [SEED, zlib.crc32(name.encode())] + [int(w) for w in what]


def _deal(name, m, n, cap, pairs):
    """columns by `pairs`; fixed rows: 0 and m - 1 of degree 1, 1 and m - 2 twins, m // 3 and 2 * m // 3 + 1 empty, 3 full (degree = cap), and on
    the NaN graph row m // 2 of degree 1 on the column of row 0"""
    rng = np.random.default_rng(_seed(name, 0))
    cd = GS.blocks(rng, *pairs)
    assert len(cd) == n
    top = np.flatnonzero(cd == cd.max())
    ones = [int(top[0]), int(top[1])]
    twin = np.sort(top[2:2 + min(4, cap)])
    full = np.sort(top[6:6 + cap])
    fixed = {0: ones[:1], m - 1: ones[1:], 1: twin, m - 2: twin, m // 3: [], 2 * m // 3 + 1: [], 3: full}
    if name == NAN_GRAPH:
        fixed[m // 2] = ones[:1]
    assert len(fixed) == (8 if name == NAN_GRAPH else 7)
    return GS.deal(rng, m, cd, fixed=fixed, row_cap=cap)


def graph(name):
    """-> SimpleNamespace(name, m, n, nnz, indptr, indices, H (dense uint8), row_deg, col_deg, rate, inst, note, plan, pinned {row: bit})"""
    if name in _GRAPHS:
        return _GRAPHS[name]
    m, n, cap, pairs, rate, inst, note = TABLE[name]
    if name == "one_edge":
        ip, ix = np.array([0, 1], np.int32), np.array([0], np.int32)
    elif name == "uncut":
        rng = np.random.default_rng(_seed(name, 0))
        ip, ix = GS.deal(rng, m, GS.blocks(rng, *pairs), row_cap=cap)
    elif name == "i63_team1025":
        ip, ix = graph("i63_team1024").indptr, graph("i63_team1024").indices            # one more column, of degree 0
    elif pairs is None:
        small = graph(name.replace("_out", "_in"))                                       # one more row on two new columns
        ip = np.concatenate([small.indptr, [small.nnz + 2]]).astype(np.int32)
        ix = np.concatenate([small.indices, [small.n, small.n + 1]]).astype(np.int32)
    else:
        ip, ix = _deal(name, m, n, cap, pairs)
    assert len(ip) == m + 1
    rd, cd = GS.degrees(ip, ix, n)
    H = np.zeros((m, n), np.uint8)
    H[np.repeat(np.arange(m), rd), ix] = 1
    g = SimpleNamespace(name=name, m=m, n=n, nnz=len(ix), indptr=ip, indices=ix, H=H, row_deg=rd, col_deg=cd, rate=rate, inst=inst, note=note,
                        plan=plan(m, n, len(ix), int(rd.max()), int(cd.max())), pinned={0: 1, m // 2: 0} if name == NAN_GRAPH else {})
    _GRAPHS[name] = g
    return g


def slice_of(g, row):
    """which of a thread's row slices holds `row` (member + c * TS)"""
    return row // g.plan.TS


def batch(g):
    """64 shots, or 65 where 64 is a multiple of S > 1: the last group of a decode is ragged"""
    return 65 if g.plan.S > 1 and 64 % g.plan.S == 0 else 64


# ---------------------------------------------------------------------------------------- priors
def _rng(g, *what):
    return np.random.default_rng(_seed(g.name, *what))


def overflow_column(g):
    """A column of degree >= 3 whose checks all have other columns: with 1.5e308 on those, the unclipped messages of iteration 0 into it are
    alpha_0 * 1.5e308 each, and three of one sign overflow."""
    ok = [j for j in np.flatnonzero(g.col_deg >= 3) if (g.row_deg[g.H[:, j] > 0] >= 2).all()]
    return int(ok[int(_rng(g, 8).integers(0, len(ok)))])


def priors(g):
    """The prior classes of regular_shapes.priors on an irregular graph, every one clean (finite, no -0.0) -> {class name: f64 [n]}"""
    n = g.n
    base = np.log((1 - g.rate) / g.rate)
    nine, seven = max(1, n // 9), max(1, n // 7)
    out = {"uniform": np.full(n, base),
           "normal": base + _rng(g, 1).normal(0.0, 0.5, n),
           "negative class": GS.by_class(_rng(g, 2), n, [-1.5, 4.0], sizes=[nine, n - nine]),
           "zero class": GS.by_class(_rng(g, 3), n, [0.0, 4.0], sizes=[nine, n - nine]),
           "above clip": GS.by_class(_rng(g, 4), n, [27.0, 4.0], sizes=[seven, n - seven]),
           "all zero": np.zeros(n)}
    if n >= 7:
        out["subnormal"] = GS.by_class(_rng(g, 5), n, [5e-324, 1e-310, 3.0], sizes=[3, 3, n - 6])
        huge = np.full(n, 4.0)
        j = overflow_column(g)
        others = np.flatnonzero(g.H[g.H[:, j] > 0].any(axis=0))
        huge[others[others != j]] = 1.5e308
        out["huge"] = huge
    return out


NOT_CLEAN = (np.inf, -np.inf, np.nan, -0.0)


def not_clean_columns(g):
    """Eight columns (four where the team has one row slice), one per value of NOT_CLEAN and row slice: column [v][c] lies in a row of slice c that
    has at least three columns, no two of them in one row -> int array [4, slices]"""
    slices = 1 + (g.m > g.plan.TS and g.plan.inst[2] == 2)
    rng = _rng(g, 6)
    rows = [np.flatnonzero((g.row_deg >= 3) & (np.arange(g.m) // g.plan.TS == c)) for c in range(slices)]
    out, used = np.zeros((4, slices), np.int64), set()
    for c in range(slices):
        pick = rng.choice(rows[c], 4, replace=False)
        for v, i in enumerate(pick):
            cols = [int(j) for j in g.indices[g.indptr[i]:g.indptr[i + 1]] if int(j) not in used]
            out[v, c] = cols[0]
            used.add(cols[0])
    return out


def not_clean_prior(g):
    """the `normal` prior with +inf, -inf, NaN and -0.0 on not_clean_columns(g)"""
    pr = priors(g)["normal"].copy()
    for v, cols in zip(NOT_CLEAN, not_clean_columns(g)):
        pr[cols] = v
    return pr


# ---------------------------------------------------------------------------------------- syndromes
def syndromes_of(g, errors):
    return ((np.asarray(errors, np.int32) @ g.H.T.astype(np.int32)) & 1).astype(np.int8)


def syndromes(g, B, prior=None, salt=0):
    """The convention of regular_shapes.syndromes: B syndromes of random errors, then (B >= 2) an all-zero one last and (B >= 3) an unrealisable
    (random) one first, and (B >= 4, with a prior) second the syndrome of the error that the prior's signs state.  Even shots draw every bit with
    probability g.rate * SCALES[(b / 2) % 4]; odd shots draw bit j with the probability its prior states, 1 / (1 + exp(prior[j])) (a NaN prior: no
    error).  g.pinned {row: bit} overrides those rows on every second shot (the NaN graph's two degree-1 checks on one column)."""
    rng = _rng(g, 7, salt, B)
    q = np.full((B, g.n), g.rate) * np.asarray(SCALES)[(np.arange(B) // 2) % 4][:, None]
    if prior is not None:
        with np.errstate(over="ignore"):
            q[1::2] = 1.0 / (1.0 + np.exp(np.asarray(prior, np.float64)))
    else:
        q[1::2] = g.rate
    S = syndromes_of(g, rng.random((B, g.n)) < q)
    if B >= 3:
        S[0] = rng.random(g.m) < 0.5
    if B >= 4 and prior is not None:
        S[1] = syndromes_of(g, (np.asarray(prior) < 0)[None, :])[0]
    for i, bit in g.pinned.items():
        S[0::2, i] = bit
    if B >= 2:
        S[-1] = 0
    return S


def logicals(g, k=3):
    """k random rows over the columns: what the Monte-Carlo plan compares e xor e_hat against"""
    return (_rng(g, 9).random((k, g.n)) < 0.5).astype(np.uint8)


# ---------------------------------------------------------------------------------------- the decode cases of the GPU module
def decode_cases():
    """-> list of SimpleNamespace(id, kind, graph, prior (class name or "not clean"), clip, B, max_iter, alpha_mode, alpha, damping, salt)"""
    out = []

    def add(kind, gname, prior, clip=20.0, max_iter=MAX_ITER, alpha_mode="dynamical", alpha=1.0, damping=1.0, salt=0):
        out.append(SimpleNamespace(id=f"{kind}-{gname}-{prior.replace(' ', '_')}-clip{clip:g}", kind=kind, graph=gname, prior=prior, clip=clip,
                                   B=batch(graph(gname)), max_iter=max_iter, alpha_mode=alpha_mode, alpha=alpha, damping=damping, salt=salt))
    for gname in ACCEPTED:
        for prior in ("uniform", "normal"):
            add("team", gname, prior, salt=1)
    for gname in FULL_GRAPHS:
        for prior in PRIOR_CLASSES:
            for clip in CLIPS:
                add("prior", gname, prior, clip)
        add("damped", gname, "normal", 6.0, damping=0.85)
        add("const", gname, "negative class", 6.0, alpha_mode="alvarado", alpha=0.8)
        add("seq", gname, "negative class", 6.0, alpha_mode="alvarado-autoregressive", alpha=np.array([0.55, 0.7, 0.9]))
        add("iter0", gname, "normal", max_iter=0)
        add("iter1", gname, "normal", max_iter=1)
        add("dirty", gname, "not clean")
        add("dirty_damped", gname, "not clean", damping=0.85)
    assert len({c.id for c in out}) == len(out)
    return out


def prior_of(g, case):
    return not_clean_prior(g) if case.prior == "not clean" else priors(g)[case.prior]


# ---------------------------------------------------------------------------------------- second trip of the persistent loop
SECOND_TRIP = {"i84_m300": 2 * GRID_CAP + 2 + 1, "i84_m511": GRID_CAP + 100}


def second_trip(name):
    """-> (graph, B, first shot of the second `base`, syndromes): workgroup 0 (and, with S = 2, a ragged workgroup 1) decodes a second group.  The
    first shot of the second trip is unrealisable (random bits), the last of the batch all-zero: both verdicts occur on the second `base`."""
    g = graph(name)
    B = SECOND_TRIP[name]
    first = GRID_CAP * g.plan.S
    synd = syndromes(g, B, priors(g)["normal"], salt=2)
    synd[first] = _rng(g, 10).random(g.m) < 0.5
    return g, B, first, synd


# ---------------------------------------------------------------------------------------- Monte-Carlo cases
MC_SEED, MC_P = 20261019, 0.06
MC_BEGIN = 1000


def mc_count(g):
    """a shot count that is no multiple of S and gives every slot of a few groups work"""
    c = 3 * 64 + 5
    return c if c % g.plan.S else c + 1


MC_PIECES = ("i84_m70", 4 * 61 + 3, 61)                 # (graph, count, plan batch): one call cut into pieces of 61 shots
MC_TRIP = ("i84_m511", GRID_CAP + 150)                  # more than 4096 shots in one piece: failure records exported from a second trip
MC_DAMPING = 0.85                                       # not fused: sample, decode through the DAMP kernel, judge


def mc_cases():
    """-> list of SimpleNamespace(id, graph, begin, count, use_osd, fixed (FLAG_FIXED_ITERS), damping, batch (None: one piece))"""
    out = []

    def add(kind, gname, count, use_osd=True, fixed=False, damping=1.0, batch=None, begin=MC_BEGIN):
        out.append(SimpleNamespace(id=f"{kind}-{gname}-{'osd' if use_osd else 'bp'}-{'fixed' if fixed else 'exit'}", graph=gname, begin=begin, count=count,
                                   use_osd=use_osd, fixed=fixed, damping=damping, batch=batch))
    for gname in MC_GRAPHS:
        for use_osd in (True, False):
            for fixed in (False, True):
                add("mc", gname, mc_count(graph(gname)), use_osd, fixed)
        add("damped", gname, mc_count(graph(gname)), damping=MC_DAMPING)
    add("pieces", MC_PIECES[0], MC_PIECES[1], batch=MC_PIECES[2])
    add("trip", MC_TRIP[0], MC_TRIP[1])
    assert len({c.id for c in out}) == len(out)
    return out
