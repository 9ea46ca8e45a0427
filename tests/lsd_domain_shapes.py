"""Seeded matrices and shots that take BP+LSD (qldpc_lsd_batch, csrc/lsd.hip) over the sizes, caps and round-list forms it accepts beyond the four small
matrices of tests/lsd_shapes.py: more than 256 local rows, 16 row words, round lists on both sides of the LDS list capacity, columns of more than 64
rows, bit tables of more than 256 words, long rows, the largest layout that fits and the hand-over rule (a matrix OSD-0 refuses is refused).  Each
family has the edge it exists for written next to it; tests/test_lsd_domain_cpu.py asserts on the model that the shots reach the edges,
tests/test_lsd_domain_gpu.py holds the kernel to the model's answers.  Plain module (no pytest hooks); deterministic from the seeds of osd_shapes.

`accepted` restates lsd_graph_supported (csrc/lsd.hip) from the two mirrors: the layout rule of lsd_shapes and OSD-0's refusal of osd_shapes."""
from types import SimpleNamespace

import numpy as np

import lsd_model as M
import lsd_shapes as LS
import lsd_stats_model as SM
import osd_shapes as S

LDS_TEXT = "needs more LDS"
HANDOVER_TEXT = "over to OSD-0"
ROWS_TEXT = "m <= 65535"


def accepted(m, n, cdeg, max_rows):
    """lsd_graph_supported: the layout fits, and OSD-0 (which gets the flag-1 and flag-2 shots) takes the matrix"""
    return LS.supported(m, n, cdeg, max_rows) and not S.rule_path(m, n, cdeg).refused


# ---------------------------------------------------------------------------------------------------------------- star forests
def build_stars(name, degrees):
    """A forest of stars: centre c is row c; it has degrees[c] leaf rows, a column (centre, leaf) for each, and behind them in index order one unit
    column (centre only).  Rows 0 .. S-1 are the centres, the leaves follow centre by centre; the columns of centre c are col0[c] .. col0[c] + degrees[c],
    the unit column last.  A seed on a centre alone is solved exactly when its unit column joins A."""
    degrees = np.asarray(degrees, np.int64)
    Sn = degrees.size
    col0 = np.concatenate([[0], np.cumsum(degrees + 1)])[:-1]
    leaf0 = Sn + np.concatenate([[0], np.cumsum(degrees)])[:-1]
    r, c = [], []
    for k in range(Sn):
        d = int(degrees[k])
        cols = col0[k] + np.arange(d + 1)
        r += [np.full(d + 1, k), leaf0[k] + np.arange(d)]
        c += [cols, cols[:d]]
    r, c = np.concatenate(r), np.concatenate(c)
    m, n = int(Sn + degrees.sum()), int((degrees + 1).sum())
    ip, ix = S._csr(r.astype(np.int64), c.astype(np.int64), m)
    return SimpleNamespace(name=name, kind="stars", m=m, n=n, indptr=ip, indices=ix, max_col_deg=int(np.bincount(ix, minlength=n).max()), null_rows=None,
                           degrees=degrees, col0=col0)


def star_shot(f, ranks, rng):
    """hard = 0, a seed on every centre of `ranks` ({centre: rank of its unit column among its own columns, 0 = least key}); the keys of different centres
    interleave.  ranks == "equal": every centre seeded and every |llr| equal, so the index alone orders (a unit column then ranks last: degrees[c])."""
    synd, llr = np.zeros(f.m, np.int8), np.full(f.n, 1.5)
    if isinstance(ranks, str):
        assert ranks == "equal"
        synd[:f.degrees.size] = 1
        return synd, llr, {c: int(f.degrees[c]) for c in range(f.degrees.size)}
    llr = (40.0 + rng.random(f.n)) * rng.choice([-1.0, 1.0], f.n)            # the centres without a seed: behind every key in play
    for c, k in ranks.items():
        d = int(f.degrees[c])
        assert 0 <= k <= d
        order = list(range(k)) + [d] + list(range(k, d))                     # positions (leaf columns 0 .. d-1, unit column d) in ascending key
        mag = np.arange(d + 1) * 0.1 + rng.random(d + 1) * 0.09
        llr[f.col0[c] + np.asarray(order)] = mag * rng.choice([-1.0, 1.0], d + 1)
        synd[c] = 1
    return synd, llr, dict(ranks)


def star_closed_form(f, ranks, bps, max_rows):
    """what the definition gives for a star shot, by counting -> (info, [|N_t|]): a centre of degree d whose unit column has rank k picks for
    k // bps + 1 rounds, bps columns a round until its d + 1 run out; a leaf column brings one row, the unit column none"""
    rows, cols, lists, t = len(ranks), 0, [], 0
    if not ranks:
        return (0, 0, 0, 0), []
    while True:
        t += 1
        listed = 0
        for c, k in ranks.items():
            if k // bps + 1 >= t:
                took = min(bps, int(f.degrees[c]) + 1 - (t - 1) * bps)
                listed += took
                rows += took - (1 if k // bps + 1 == t else 0)
        if listed == 0:
            break
        lists.append(listed)
        if rows > max_rows:
            return (1, 0, 0, 0), lists
        cols += listed
    return (0, len(lists), rows, cols), lists


def build_twins(name, m):
    """m rows, columns 2 r and 2 r + 1 both the unit column of row r: whichever twin joins A first pivots, the other depends on it"""
    ip, ix = S._csr(np.repeat(np.arange(m), 2).astype(np.int64), np.arange(2 * m).astype(np.int64), m)
    return SimpleNamespace(name=name, kind="twins", m=m, n=2 * m, indptr=ip, indices=ix, max_col_deg=1, null_rows=None)


def _mixed(rng, centres, f):
    return {int(c): int(rng.integers(0, f.degrees[c] + 1)) for c in centres}


def _first(k, rank, then=None):
    """the first k centres at `rank`, then the centres of `then` ({centre: rank})"""
    return {**{c: rank for c in range(k)}, **(then or {})}


# name: (S, D, [shot recipes], what it reaches).  A recipe is "equal", a dict of ranks, or ("mixed", centres): random ranks on those centres.
STARS = {
    "s64d4": (64, 4, [_first(64, 3), _first(63, 3, {63: 4}), "equal", _first(64, 0), ("mixed", 40), ("mixed", 64)],
              "row degree 5; bps = 2: lists of exactly 128 (also with every key equal), final |R| = 256 and 257, 64 seeds"),
    "s43d3": (43, 3, [_first(43, 2), "equal", ("mixed", 43), ("mixed", 20)],
              "row degree 4; bps = 3: lists of exactly 129 = the LDS list capacity + 1 (also with every key equal)"),
    "s129d2": (129, 2, [_first(129, 1), "equal", ("mixed", 129), _first(128, 1)],
               "row degree 3; bps = 1: lists of 129 and 128, final |R| = 258 and 256: the row loops make a second pass"),
    "s257d1": (257, 1, [_first(257, 1), "equal", _first(256, 0), _first(257, 0), ("mixed", 257), _first(128, 1)],
               "row degree 2; lists of 257 (more entries than threads; also with every key equal), final |R| = 256, 257 and 514"),
    "s512d1": (512, 1, [_first(512, 1), "equal", _first(128, 0), _first(192, 0), _first(320, 0), ("mixed", 512)],
               "ends on all 1024 rows at max_rows = 1024 (lists of 512; bps = 2: one list of 1024); exactly 128, 192 and 320 seeds"),
    "s513d2": (513, 2, [_first(300, 2, {c: 0 for c in range(300, 513)}), _first(512, 1), _first(513, 0), ("mixed", 340)],
               "513 seeds under max_rows = 1024, stopped by the rows of the second round; 512 seeds that end on exactly 1024 rows"),
    "s1024d0": (1024, 0, ["equal", _first(1024, 0), _first(64, 0), _first(128, 0), _first(192, 0), _first(320, 0)],
                "row degree 1; exactly 64, 128, 192, 320 and 1024 seeds (T b starts as whole words); one list of 1024"),
    "s8d7": (8, 7, ["equal", _first(8, 7), ("mixed", 8), ("mixed", 5), _first(8, 4)], "row degree 8: two unrolled groups of four in the row scan"),
    "s2d300": (2, 300, [{0: 70}, {0: 200, 1: 65}, "equal", {1: 299}], "rows of degree 301 with bps = 64: 63 threshold rescans a round, the unit column ranked past 64"),
}
# (shots, bits_per_step, max_rows) every star family runs at; max_rows == |R| of a shot (flag 0) beside |R| - 1 (flag 1) at 256, 257 and 1024
STAR_PARAMS = {
    "s64d4": ((2, 1024), (2, 256), (2, 255), (2, 257), (1, 512), (64, 320)),
    "s43d3": ((3, 512), (1, 512), (3, 128)),
    "s129d2": ((1, 512), (2, 387), (1, 257)),
    "s257d1": ((1, 1024), (1, 256), (1, 255), (1, 257), (2, 514)),
    "s512d1": ((1, 1024), (1, 1023), (2, 1024)),
    "s513d2": ((1, 1024), (3, 1024)),
    "s1024d0": ((1, 1024), (1, 1023), (5, 320)),
    "s8d7": ((1, 64), (3, 64), (4, 64), (8, 33)),
    "s2d300": ((64, 1024), (64, 128), (7, 1024)),
}

# ---------------------------------------------------------------------------------------------------------------- the other families
CAP = 1024
M_DEP = 1016                       # with columns of weight <= 4 the largest accepted n puts the layout at exactly 160 KiB (the CPU module asserts it)
HEAVY = (64, 65, 130)
# name: (kind, m, n or None where it is computed below, extra, what it reaches)
TABLE = {
    "ident1024": ("ident", 1024, 2500, None, "random errors of weight 150-300: clusters that end on more than 960 rows (16 row words in use), lists beyond 256"),
    "dep_wide": ("dep", M_DEP, None, None, "the largest n accepted at max_rows = 1024 (the whole 160 KiB in use); pivots on columns beyond 8192"),
    "u200": ("dep", 200, 65534, None, "the last column index, 65533, pivots; bit tables of 2048 words; run at the largest cap accepted"),
    "heavy64": ("heavy", 300, 700, 64, "a column of exactly 64 rows: one full chunk"),
    "heavy65": ("heavy", 300, 700, 65, "a column of 65 rows: one row in the second chunk"),
    "heavy130": ("heavy", 300, 700, 130, "a column of 130 rows: three chunks, the least label in any of them"),
    "twins130": ("twins", 130, 260, None, "every unit column twice, the twins tied in |llr|: in a list beyond the LDS capacity the index decides which one pivots"),
    "tall": ("plain", None, 64, None, "the largest m OSD-0 accepts: flag 0 and flag 2 (most rows have no column); one row more is refused"),
}
_FAM, _GRAPH, _SHOTS, _ANSWERS = {}, {}, {}, {}


def _cdeg(kind, m, n, extra):
    return S.build_matrix("lsd_domain_probe_" + kind, kind, m, n, extra).max_col_deg


def edges():
    """the computed edges (from the families' own max_col_deg) -> SimpleNamespace(n_wide, cap_u200, m_tall, cap_65535)"""
    if "edges" not in _FAM:
        cd = _cdeg("dep", M_DEP, 9000, None)
        n_wide = S.largest(lambda n: accepted(M_DEP, n, cd, CAP), 1, 65534)
        cdu = _cdeg("dep", 200, 65534, None)
        cap_u = S.largest(lambda r: accepted(200, 65534, cdu, r), 1, 1025)
        cdt = _cdeg("plain", 30000, 64, None)
        m_tall = S.largest(lambda m: accepted(m, 64, cdt, 512), 1, 65535)
        cap_big = S.largest(lambda r: LS.supported(65535, 64, cdt, r), 1, 1024)
        _FAM["edges"] = SimpleNamespace(n_wide=n_wide, cd_wide=cd, cap_u200=cap_u, cd_u200=cdu, m_tall=m_tall, cd_tall=cdt, cap_65535=cap_big)
    return _FAM["edges"]


def family(name):
    """-> the matrix (a namespace like osd_shapes.build_matrix's), cached"""
    if name not in _FAM:
        if name in STARS:
            Sn, D = STARS[name][:2]
            _FAM[name] = build_stars("lsd_domain_" + name, [D] * Sn)
        else:
            kind, m, n, extra, _ = TABLE[name]
            E = edges()
            m = E.m_tall if name == "tall" else m
            n = E.n_wide if name == "dep_wide" else n
            _FAM[name] = build_twins("lsd_domain_" + name, m) if kind == "twins" else S.build_matrix("lsd_domain_" + name, kind, m, n, extra)
    return _FAM[name]


def graph(name):
    if name not in _GRAPH:
        f = family(name)
        _GRAPH[name] = M.Graph(f.indptr, f.indices, f.n)
    return _GRAPH[name]


def default_cap(name):
    return {"u200": edges().cap_u200, "tall": 512, "heavy64": 512, "heavy65": 512, "heavy130": 512}.get(name, CAP)


def params(name):
    """the (bits_per_step, max_rows) pairs a family runs at"""
    if name in STARS:
        return STAR_PARAMS[name]
    if name in ("ident1024", "dep_wide"):
        return ((4, CAP), (64, CAP))
    if name == "u200":
        return ((1, default_cap(name)), (2, default_cap(name)))
    if name == "tall":
        return ((1, 512), (2, 512))
    if name == "twins130":
        return ((2, CAP), (2, 130), (1, 512), (2, 129))
    extra = TABLE[name][3]
    return ((4, 512), (1, extra - 1), (64, 512))                             # extra - 1: below the three seeds plus the rows the heavy column brings


def _ns(synd, llr, hard, **more):
    return SimpleNamespace(synd=np.ascontiguousarray(synd, np.int8), llr=np.ascontiguousarray(llr, np.float64), hard=np.ascontiguousarray(hard, np.int8), **more)


def general(f, G, B, rng):
    """lsd_shapes.general's recipe in its quick form -> (synd, llr, hard)"""
    sh = LS.general_on(f, G, rng, B, quick=True)
    return sh.synd, sh.llr, sh.hard


def shots(name):
    """the family's batch (4 to 12 shots), cached and left unchanged; star families carry `ranks`, heavy ones `rows` (the three seeds of shot 0)"""
    if name in _SHOTS:
        return _SHOTS[name]
    f, G, rng = family(name), graph(name), S._rng("lsd_domain_" + name, 1)
    more = {}
    if name in STARS:
        out, ranks = [], []
        for rec in STARS[name][2]:
            if isinstance(rec, tuple):
                rec = _mixed(rng, rng.permutation(f.degrees.size)[:rec[1]], f)
            s, l, rk = star_shot(f, rec, rng)
            out.append((s, l, np.zeros(f.n, np.int8)))
            ranks.append(rk)
        synd, llr, hard = (np.stack(x) for x in zip(*out))
        more["ranks"] = ranks
    elif name in ("ident1024", "dep_wide"):
        B = 4
        E = np.zeros((B, f.n), np.int8)
        for b, w in enumerate((150, 200, 250, 300)):
            E[b, rng.choice(f.n, w, replace=False)] = 1
        synd, llr, hard = np.stack([G.parity(e) for e in E]), rng.normal(1.0, 3.0, (B, f.n)), np.zeros((B, f.n), np.int8)
    elif name == "u200":
        synd, llr, hard = general(f, G, 6, rng)
        last = f.n - 1                                                       # shot 0: the last column carries the least key and its rows are the seeds
        synd[0], hard[0] = 0, 0
        synd[0, G.rows_of(last)] = 1
        llr[0] = 2.0 + np.abs(llr[0])
        llr[0, last] = -0.125
    elif name.startswith("heavy"):
        synd, llr, hard = general(f, G, 8, rng)
        extra = TABLE[name][3]
        rows = G.rows_of(0)
        assert rows.size == extra and np.all(np.diff(rows) > 0)
        seeds = rows[[0, extra // 2, extra - 1]]                             # extra = 130: positions 0, 65, 129, one in each 64-row chunk of the column
        synd[0], hard[0] = 0, 0
        synd[0, seeds] = 1
        llr[0] = 2.0 + np.abs(llr[0])
        llr[0, 0] = 0.125
        more["rows"] = seeds
    elif name == "twins130":
        synd, hard = np.zeros((5, f.m), np.int8), np.zeros((5, f.n), np.int8)
        llr = np.full((5, f.n), -1.5)
        for b, k in enumerate((130, 130, 64, 65, 130)):                      # with bps = 2: lists of 260, 260, 128, 130 and 260
            synd[b, :k] = 1
        mag = 0.5 + rng.random(f.m)
        llr[1, 0::2], llr[1, 1::2] = -mag, mag                               # tied inside every pair only, the pairs in random key order
        llr[4, 0::2], llr[4, 1::2] = mag, np.nextafter(mag, 0.0)             # no tie at all: the odd twin is one ulp lesser, and pivots
    else:
        assert name == "tall"
        deg = np.diff(f.indptr)
        bare, full = np.flatnonzero(deg == 0), np.flatnonzero(deg > 0)
        B = 6
        E = np.zeros((B, f.n), np.int8)
        for b in range(B):
            E[b, rng.choice(f.n, 1 + b, replace=False)] = 1
        synd, llr, hard = np.stack([G.parity(e) for e in E]), rng.normal(1.0, 3.0, (B, f.n)), np.zeros((B, f.n), np.int8)
        synd[4, bare[-1]] ^= 1                                               # a seed on the last row without a column, beside seeds that have some
        synd[5] = 0
        synd[5, [bare[0], full[0]]] = 1
    _SHOTS[name] = _ns(synd, llr, hard, **more)
    return _SHOTS[name]


def answers(name, bits_per_step, max_rows):
    """the model on shots(name) -> (solution int8[B, n] -- zeros where the flag is not 0 --, info int32[B, 4], traces), cached"""
    k = (name, bits_per_step, max_rows)
    if k not in _ANSWERS:
        f, G, sh = family(name), graph(name), shots(name)
        B = sh.synd.shape[0]
        sol, info, traces = np.zeros((B, f.n), np.int8), np.zeros((B, 4), np.int32), []
        for b in range(B):
            tr = {}
            sol[b], info[b] = M.lsd(G, sh.synd[b], sh.llr[b], sh.hard[b], bits_per_step, max_rows, trace=tr, osd0=lambda *a: np.zeros(f.n, np.int8))
            traces.append(tr)
        _ANSWERS[k] = (sol, info, traces)
    return _ANSWERS[k]


def weights(n, seed=7):
    """a seeded uint16 table that holds 0 and 65535"""
    w = np.random.default_rng([seed, n]).integers(0, 65536, n).astype(np.uint16)
    w[0], w[n // 2] = 0, 65535
    return w


_STATS = {}


def stats(name, bits_per_step, max_rows, weight):
    """the eight words of every shot from the cached traces; weight: None, "seeded" or "ones" (all 65535)"""
    k = (name, bits_per_step, max_rows, weight)
    if k not in _STATS:
        f = family(name)
        w = {None: None, "seeded": weights(f.n), "ones": np.full(f.n, 65535, np.uint16)}[weight]
        _, info, traces = answers(name, bits_per_step, max_rows)
        _STATS[k] = (w, SM.stats_from_traces(graph(name), shots(name), info, traces, w))
    return _STATS[k]


NAMES = tuple(STARS) + tuple(TABLE)
