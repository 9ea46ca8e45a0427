"""Seeded generator of structured Tanner graphs for the workgroup BP kernels (csrc/minsum_wg2.hip, csrc/minsum_wg.hip) and their hand-overs.

The packaged circuit-level matrices are structurally one matrix (row degree 35, column degrees {0, 2 .. 6}, even nnz, m in 288 .. 1008).  Every family
here straddles one line of the host code that those matrices never reach; the comment beside a family names the line.  A family claims a decoder form
(`expected`: what qldpc_minsum_decode_path must report for each of its priors) and a structure (`claims`); tests/test_wg_shapes_cpu.py checks the
structure and that the claim follows from the selection rules restated below, tests/test_wg_shapes_gpu.py checks the claim against the library and every
decode against the CPU checker.  Plain module (no pytest hooks); deterministic from the seed; CSR rows sorted, no repeated edges.

rule_path() and the constants below are a SECOND COPY of the host selection logic (plan_resident, regular_supported, wg_mode, wg2_build), kept on purpose
as an independent statement of the rules: the GPU module asserts the library's own answer (qldpc_minsum_decode_path) on both sides of every limit
(rowdeg40 / 41, coldeg8 / 9, m1024 / 1025, rowdeg56 / 57, the two LDS pairs, and reg63_m512 / 513: the 512-thread team of plan_regular in
csrc/minsum_regular.hip), so a limit that moves in csrc/ fails there and has to be moved here too.  The regular kernel's other two conditions,
max_iter <= 1024 (its alpha table in LDS, kMaxIterLds) and clip >= 0, are arguments of rule_path(); tests/test_regular_domain_gpu.py asserts them
against the library.
"""
import zlib
from types import SimpleNamespace

import numpy as np

LDS_BYTES = 160 * 1024
WG2_FIXED = 16 * 1025 + 8 * 1025 + 8          # check states of minsum_wg2.hip at fixed offsets (kWg2OffV)
WG2_ROW_DEG, WG2_COL_DEG, WG2_ROWS = 40, 8, 1024
WG_ROW_DEG, REG_INDEX_ROW_DEG = 56, 40
REGULAR_TEAM, REGULAR_MAX_ITER = 512, 1024        # plan_regular of minsum_regular.hip: QLDPC_LB_T threads per team, kMaxIterLds alpha values in LDS


def _up(x, a):
    return (x + a - 1) // a * a


# ---------------------------------------------------------------------------------------- the selection rules, restated
def degrees(indptr, indices, n):
    rd = np.diff(indptr).astype(np.int64)
    cd = np.bincount(indices, minlength=n).astype(np.int64) if len(indices) else np.zeros(n, np.int64)
    return rd, cd


def wg2_lds_bytes(n, nnz):
    """P.lds of wg2_build: fixed part + posteriors + 16-bit edge list padded to pairs + flags + one 16-byte record per chunk."""
    off_el = _up(WG2_FIXED + 8 * n, 16)
    off_f = _up(off_el + (nnz + 1) // 2 * 4, 16)
    return off_f + 32 + (n + 63) // 64 * 16


def wg_lds_bytes(m, n, vglobal):
    """wg_lds_bytes of minsum_wg.hip: posteriors (unless they live in global memory) + 24 bytes per check (one spare) + flags."""
    return (0 if vglobal else _up(8 * n, 16)) + (m + 1) * 24 + 16


def wg2_chunks(col_deg, prior):
    """The column-slot order of wg2_build -- (degree descending, prior bit pattern ascending, index) -- cut into 64-slot chunks ->
    (order, pure flag per chunk, run length per chunk).  A chunk is pure when it is full and one (degree, prior) class."""
    bits = np.ascontiguousarray(prior, np.float64).view(np.uint64)
    n = len(col_deg)
    order = np.lexsort((np.arange(n), bits, -np.asarray(col_deg)))
    nch = (n + 63) // 64
    pure = np.zeros(nch, bool)
    for q in range(nch):
        sl = order[64 * q:64 * q + 64]
        pure[q] = len(sl) == 64 and (col_deg[sl] == col_deg[sl[0]]).all() and (bits[sl] == bits[sl[0]]).all()
    run = np.zeros(nch, np.int64)
    for q in range(nch - 1, -1, -1):
        if pure[q]:
            a, b = order[64 * q], order[64 * (q + 1)] if q + 1 < nch else -1
            same = q + 1 < nch and pure[q + 1] and col_deg[a] == col_deg[b] and bits[a] == bits[b]
            run[q] = 1 + (run[q + 1] if same else 0)
    return order, pure, run


def prior_is_clean(prior):
    prior = np.asarray(prior, np.float64)
    return bool(np.isfinite(prior).all() and not ((prior == 0) & np.signbit(prior)).any())


def resident_takes(m, n, nnz, rd, cd):
    """plan_resident of minsum_resident.hip (the part small graphs can fail: degrees, bytes per shot, team size)."""
    if m <= 0 or n <= 0 or nnz <= 0 or rd.max() > 8 or cd.max() > 4:
        return False
    cdeg = 6 if rd.max() <= 6 and cd.max() <= 3 else 8
    rst = cdeg + 1 if cdeg % 2 == 0 else cdeg
    if (m * rst + n) * 8 + 32 + (n + 3) // 4 * 4 > 60 * 1024:
        return False
    ts = max(m, (n + 1) // 2)
    if ts > 256:
        ts = max((m + 1) // 2, (n + 3) // 4)
    return ts <= 1024


def regular_takes(rd, cd):
    pair = (int(rd.max()), int(cd.max()))
    return pair in ((6, 3), (4, 2), (8, 4)) and (rd == pair[0]).all() and (cd == pair[1]).all()


def rule_path(indptr, indices, n, prior, host_prior=True, damping=1.0, table_flags=False, max_iter=50, clip=20.0):
    """The decoder form the selection rules give (dispatch of csrc/decode_api.hip) for a clean alpha schedule and no kernel-forcing flag;
    table_flags: one of the flags that ask for a form of the table kernel is set.  max_iter and clip matter to the regular kernel alone
    (regular_supported: clip >= 0, plan_regular: max_iter <= 1024); a negative clip is not clean, which the workgroup forms below then see too."""
    m, nnz = len(indptr) - 1, len(indices)
    rd, cd = degrees(indptr, indices, n)
    if m and n and regular_takes(rd, cd) and max(m, (n + 1) // 2) <= REGULAR_TEAM and max_iter <= REGULAR_MAX_ITER and clip >= 0:
        return "REGULAR"
    if resident_takes(m, n, nnz, rd, cd):
        return "RESIDENT"
    tables = n < 65535 and rd.max() < 256                                     # graph.hip: the ELL tables exist
    if not (tables and m > 0 and n > 0 and rd.max() <= WG_ROW_DEG and wg_lds_bytes(m, n, True) <= LDS_BYTES):
        return "STREAM"
    if host_prior and damping == 1.0 and not table_flags and prior_is_clean(prior) and clip > 0 and np.isfinite(clip):
        if (m <= WG2_ROWS and n < 65536 and rd.max() <= WG2_ROW_DEG and cd.max() <= WG2_COL_DEG and nnz >= 1 and
                wg2_lds_bytes(n, nnz) <= LDS_BYTES):
            _, pure, _ = wg2_chunks(cd, prior)
            if 4 * int((~pure).sum()) <= len(pure) + 3:
                return "WG2"
    return "WG"


# ---------------------------------------------------------------------------------------- the builder
def deal(rng, m, col_deg, fixed=None, row_cap=None):
    """Configuration-model graph: column j gets col_deg[j] edges (its stubs), dealt round-robin over the rows in shuffled order; a row that already
    has the column or is full (row_cap) is passed over, a stub no row can take is dropped.  `fixed` {row: columns} is placed first and its edges count
    towards the column degrees; fixed rows take no dealt stubs.  -> (indptr int32, indices int32)."""
    col_deg = np.asarray(col_deg, np.int64)
    rows = [set() for _ in range(m)]
    left = col_deg.copy()
    fixed = fixed or {}
    for i, cols in fixed.items():
        rows[i] = set(int(c) for c in cols)
        for c in rows[i]:
            left[c] -= 1
    assert (left >= 0).all(), "fixed rows exceed a column's degree"
    free = [i for i in range(m) if i not in fixed]
    stubs = np.repeat(np.arange(len(col_deg)), left)
    rng.shuffle(stubs)
    cap = row_cap if row_cap is not None else 1 << 30
    r = 0
    for j in stubs:
        for t in range(len(free)):
            i = free[(r + t) % len(free)]
            if j not in rows[i] and len(rows[i]) < cap:
                rows[i].add(int(j))
                r = (r + t + 1) % len(free)
                break
    indptr = np.zeros(m + 1, np.int32)
    indptr[1:] = np.cumsum([len(s) for s in rows])
    indices = np.array([c for s in rows for c in sorted(s)], np.int32)
    return indptr, indices


def blocks(rng, *pairs):
    """Column degrees from (degree, count) pairs, scattered over the column indices (wg2_build sorts them back together)."""
    d = np.concatenate([np.full(c, g, np.int64) for g, c in pairs])
    rng.shuffle(d)
    return d


def by_class(rng, n, values, sizes=None):
    """A class-valued prior: `values` scattered at random, or with exact class `sizes`."""
    values = np.asarray(values, np.float64)
    if sizes is None:
        return values[rng.integers(0, len(values), n)]
    lab = np.repeat(np.arange(len(values)), sizes)
    assert len(lab) == n
    rng.shuffle(lab)
    return values[lab]


def by_degree(col_deg, values):
    """One prior value per column degree: class boundaries coincide with the degree boundaries."""
    return np.asarray(values, np.float64)[np.asarray(col_deg)]


DEGREE_VALUES = [3.25, 2.5, -1.5, 0.0, 27.0, 4.0, 6.25, 1.125, 5.5, 3.0]      # a negative class, a zero class, one above clip_llr = 20


def syndromes(case, B, salt=0):
    """B syndromes of a family: those of random errors of weight case.err_weight .. 2 * err_weight, then (B >= 2) an all-zero one last and (B >= 3)
    an unrealisable (random) one first.  case.pinned_syndrome {row: bit} overrides those rows on every second shot."""
    rng = np.random.default_rng([case.seed, 7, salt, B])
    m, n = case.m, case.n
    S = np.zeros((B, m), np.int8)
    for b in range(B):
        e = np.zeros(n, np.int8)
        e[rng.choice(n, size=min(n, int(rng.integers(case.err_weight, 2 * case.err_weight + 1))), replace=False)] = 1
        for i in range(m):
            S[b, i] = e[case.indices[case.indptr[i]:case.indptr[i + 1]]].sum() & 1
    if B >= 3:
        S[0] = rng.random(m) < 0.5
    for i, bit in case.pinned_syndrome.items():           # on every second shot (the others keep the bits of their error)
        S[0::2, i] = bit
    if B >= 2:
        S[-1] = 0
    return S


# ---------------------------------------------------------------------------------------- the families
def _case(name, seed, ip, ix, n, priors, expected, **kw):
    rd, cd = degrees(ip, ix, n)
    c = SimpleNamespace(name=name, seed=seed, indptr=ip, indices=ix, n=int(n), m=len(ip) - 1, nnz=len(ix), priors=priors, row_deg=rd, col_deg=cd,
                        expected=expected if isinstance(expected, dict) else {k: expected for k in priors},
                        claims={}, detail_set={}, detail_clear={}, variants=(), damping=1.0, axes=(), err_weight=3, pinned_syndrome={}, relay=False,
                        golden=False, dev_query=False, flag_queries=())
    c.expected_path = c.expected[next(iter(priors))]
    for k, v in kw.items():
        assert hasattr(c, k), k
        setattr(c, k, v)
    return c


def _mixed_prior(n, k):
    """Uniform-degree graph of n = 64 * nch columns: exactly k mixed chunks.  Class sizes 32, 64, .., 64, rest put a boundary in the middle of each of
    the first k chunks; the values ascend so the bit-pattern sort keeps that order."""
    sizes = [32] + [64] * (k - 1)
    sizes.append(n - sum(sizes))
    return np.repeat(2.0 + 0.25 * np.arange(len(sizes)), sizes)


def families(seed=20261016):
    """-> list of cases (SimpleNamespace): name, indptr, indices, n, m, nnz, priors {name: array}, expected {prior name: path}, expected_path,
    claims (structure the CPU suite verifies), detail_set / detail_clear {prior name: [DETAIL_* names]}, variants (flag names to decode with besides
    the common ones), damping, axes (which of the batch / schedule axes this family varies), relay, golden, dev_query, flag_queries."""
    out = []

    def rng_of(name):
        return np.random.default_rng([seed, zlib.crc32(name.encode())])

    def add(name, m, col_deg, priors, expected, fixed=None, row_cap=None, graph_seed=None, **kw):
        rng = rng_of((graph_seed or name) + "/graph")
        ip, ix = deal(rng, m, col_deg, fixed=fixed, row_cap=row_cap)
        n = len(col_deg)
        cd = np.bincount(ix, minlength=n)
        pri = {k: (v(cd) if callable(v) else v) for k, v in priors.items()}
        c = _case(name, zlib.crc32(name.encode()), ip, ix, n, pri, expected, **kw)
        out.append(c)
        return c

    uniform = lambda v=4.0: (lambda cd: np.full(len(cd), v))                  # noqa: E731
    bydeg = lambda cd: by_degree(cd, DEGREE_VALUES)                           # noqa: E731

    # ---- wg2 eligibility (wg2_build, first test: m <= 1024, row degree <= 8 * kWg2Chunks, column degree <= 8) -------------------------------
    for D, path in ((40, "WG2"), (41, "WG")):
        # row degree 40 is the last one whose column slots fit the 20 index registers; 41 also leaves the register-index lean kernel of
        # minsum_wg_launch (row degree <= 8 * kIdxChunks)
        r = rng_of(f"rowdeg{D}")
        cd = blocks(r, (5, 128), (3, 192), (0, 64))
        c = add(f"rowdeg{D}", 60, cd, {"uniform": uniform(), "by degree": bydeg}, path, fixed={0: np.flatnonzero(cd > 0)[:D]}, row_cap=30,
                claims=dict(max_row=D), relay=True, golden=(D == 40), axes=("iter9",) if D == 40 else ("const",),
                detail_clear={} if D == 40 else {"uniform": ["REG_INDICES"]}, detail_set={"uniform": ["LEAN"]})
    for D, path in ((8, "WG2"), (9, "WG")):
        # column degree 8 fills the last of the eoff[8] levels; 9 is not eligible
        r = rng_of(f"coldeg{D}")
        add(f"coldeg{D}", 80, blocks(r, (D, 64), (4, 128), (2, 64)), {"uniform": uniform(), "by degree": bydeg}, path,
            claims=dict(max_col=D), relay=True, axes=("seq",) if D == 8 else ("clip6.5",))
    # every column degree 0 .. 8 in one graph, each class one chunk, dozens of degree-0 columns (the eoff prefix of every level differs); n = 700:
    # nch = 11 < 16 waves, so five waves get an empty wq range, and the last chunk is ragged
    r = rng_of("alldeg")
    add("alldeg", 64, blocks(r, *[(d, 64) for d in range(8, 0, -1)], (0, 188)), {"uniform": uniform(), "by degree": bydeg}, "WG2",
        claims=dict(col_degs=set(range(9)), nch=11, min_deg0=24), relay=True, golden=True, axes=("B1", "B700"), variants=("WG_GENERIC", "WG_ROWMAJOR"))
    # the same spread at production width with a scattered two-valued prior: 18 classes, boundaries wherever they fall
    r = rng_of("alldeg_wide")
    wide = add("alldeg_wide", 1024, blocks(r, *[(d, 560) for d in range(8, 0, -1)], (0, 520)),
               {"two values": lambda cd: by_class(rng_of("p2"), len(cd), [2.5, 6.25]),
                # twelve values in twelve (degree, prior) classes, as the circuit-level priors have them: one per degree, a second one on half of three degrees
                "12 values": lambda cd: (2.0 + 0.375 * np.arange(12))[np.where(np.isin(cd, (8, 6, 4)) & (rng_of("p12").random(len(cd)) < 0.5), 8 + cd // 2 - 1, cd)],
                "negative class": lambda cd: by_class(rng_of("pn"), len(cd), [-1.5, 4.0], sizes=[500, 4500]),
                "zero class": lambda cd: by_class(rng_of("pz"), len(cd), [0.0, 4.0], sizes=[400, 4600]),
                "above clip": lambda cd: by_class(rng_of("pc"), len(cd), [27.0, 4.0], sizes=[700, 4300]),
                # negative controls: one -0.0 (inputs not clean) and an all-distinct prior (every chunk mixed) must take the table kernel
                "one -0.0": lambda cd: np.concatenate([[-0.0], np.full(len(cd) - 1, 4.0)]),
                "all distinct": lambda cd: 3.0 + np.arange(len(cd)) * 1e-3},
               {"two values": "WG2", "12 values": "WG2", "negative class": "WG2", "zero class": "WG2", "above clip": "WG2", "one -0.0": "WG",
                "all distinct": "WG"},
               claims=dict(col_degs=set(range(9)), m=1024), relay=True, axes=("B700", "clip6.5"), err_weight=12, dev_query=True,
               detail_clear={"one -0.0": ["LEAN", "REG_INDICES"]}, detail_set={"all distinct": ["LEAN", "REG_INDICES", "BLOCK_1024"]},
               variants=("WG_GENERIC", "WG_ROWMAJOR", "WG_VGLOBAL"))
    # one column degree only: every slot is in the prefix of the levels below its degree and of none above
    add("uniform_deg1", 16, np.full(640, 1), {"three values": lambda cd: by_class(rng_of("u1"), 640, [-1.5, 1.7, 4.0], sizes=[24, 168, 448]), "uniform": uniform()},
        "WG2", claims=dict(col_degs={1}, max_row=40), relay=True, axes=("iter1",), err_weight=1)
    add("uniform_deg8", 64, np.full(320, 8), {"uniform": uniform()}, "WG2", row_cap=40, claims=dict(col_degs={8}, max_row=40), relay=True, axes=("const",), err_weight=2)
    # odd nnz: the 16-bit edge list is padded to an even count ((nnz + 1) / 2 pairs)
    r = rng_of("odd_nnz")
    add("odd_nnz", 64, blocks(r, (3, 639), (2, 1)), {"uniform": uniform(), "by degree": bydeg}, "WG2", claims=dict(nnz_odd=True), relay=True, golden=True,
        axes=("seq",))
    # n around one and two chunks: a single ragged chunk, exactly one, one + 1 slot, ... (chunk loop bounds c1 = min(n, c0 + 64))
    for n in (63, 64, 65, 127, 128, 129):
        add(f"n{n}", 24, np.full(n, 5), {"uniform": uniform()}, "WG2", claims=dict(n=n, nch=(n + 63) // 64), relay=True, err_weight=1,
            axes=(("B1",), ("iter9",), ("const",), ("seq",), ("clip6.5",), ("iter1",))[n % 6])
    add("nch11", 64, np.full(700, 3), {"uniform": uniform(), "two classes": lambda cd: by_class(rng_of("n11"), 700, [2.5, 6.25], sizes=[320, 380])}, "WG2",
        claims=dict(nch=11), relay=True, golden=True, axes=("clip6.5",))
    # nch = 16 and 17: one chunk per wave exactly, and the first spill-over (wq split); sixteen / seventeen classes of 64 alternate chunk by chunk, so
    # every run length packed into `pure` is 1
    for nch in (16, 17):
        add(f"nch{nch}", 160, np.full(64 * nch, 5), {"class per chunk": lambda cd: by_class(rng_of("cpc"), len(cd), 2.0 + 0.25 * np.arange(len(cd) // 64),
                                                                                        sizes=[64] * (len(cd) // 64)), "uniform": uniform()},
            "WG2", row_cap=40, claims=dict(nch=nch, runs_all_one="class per chunk"), relay=True, axes=("iter9",) if nch == 16 else ("B700",), err_weight=4)
    # m from 1 to the 1024 rows the fixed LDS offsets hold; 1025 takes the table kernel with 1024 threads and no register-resident indices (m > block)
    three = lambda cd: by_class(rng_of("three"), len(cd), [-1.5, 1.7, 4.0], sizes=[len(cd) // 20, len(cd) // 4, len(cd) - len(cd) // 20 - len(cd) // 4])   # noqa: E731
    cd1 = blocks(rng_of("m1"), (1, 40), (0, 24))
    add("m1", 1, cd1, {"three values": lambda cd: by_class(rng_of("m1p"), 64, [-1.5, 1.7, 4.0], sizes=[12, 16, 36])}, "WG2", claims=dict(m=1, max_row=40), relay=True, err_weight=1, axes=("iter9",))
    add("m2", 2, blocks(rng_of("m2"), (2, 30), (1, 20), (0, 14)), {"three values": three}, "WG2", claims=dict(m=2), relay=True,
        err_weight=1, row_cap=40, axes=("const",))
    for m in (24, 63, 64, 65):
        add(f"m{m}", m, blocks(rng_of(f"m{m}"), (5, 64), (3, 64), (2, 64)), {"uniform": uniform(), "by degree": bydeg}, "WG2", claims=dict(m=m), relay=True,
            err_weight=2, axes=(("seq",), ("clip6.5",), ("iter1",), ("B1",))[m % 4])
    for m, path in ((1023, "WG2"), (1024, "WG2"), (1025, "WG")):
        add(f"m{m}", m, blocks(rng_of(f"m{m}"), (6, 512), (4, 512), (3, 512), (2, 512)), {"uniform": uniform(), "by degree": bydeg}, path,
            claims=dict(m=m), relay=True, err_weight=8, axes=("iter9",),
            detail_set={"uniform": ["BLOCK_1024", "LEAN"] + (["REG_INDICES"] if m <= 1024 else [])},
            detail_clear={"uniform": ["REG_INDICES"]} if m == 1025 else {})
    # the LDS bound of wg2_build (P.lds > 160 KB): two graphs that differ only in their number of degree-0 columns; also the longest run of pure chunks
    nnz = 5 * 640
    n_fit = max(n for n in range(15000, 18000) if wg2_lds_bytes(n, nnz) <= LDS_BYTES)
    cd_big = np.zeros(n_fit + 1, np.int64)
    cd_big[rng_of("lds").choice(n_fit, 640, replace=False)] = 5
    for n, path in ((n_fit, "WG2"), (n_fit + 1, "WG")):
        add(f"lds_{path.lower()}", 200, cd_big[:n], {"uniform": uniform()}, path, graph_seed="lds",
            claims=dict(n=n, wg2_lds_fits=(path == "WG2"), longest_run=(n - 640) // 64 if path == "WG2" else None), relay=(path == "WG2"), err_weight=4,
            axes=("B1",))
    # the mixed-chunk rule 4 * mixed <= nch + 3 on one graph: the largest admissible number of mixed chunks, and one more; every class boundary of these
    # priors lies in the middle of a chunk
    nch = 17
    kmax = (nch + 3) // 4
    add("mixed_rule", 160, np.full(64 * nch, 5), {"admissible": lambda cd: _mixed_prior(len(cd), kmax), "one more": lambda cd: _mixed_prior(len(cd), kmax + 1)},
        {"admissible": "WG2", "one more": "WG"}, row_cap=40, claims=dict(mixed={"admissible": kmax, "one more": kmax + 1}), relay=True, err_weight=4, axes=("const",))
    # degree-1 rows (+-inf messages, kernels.py:301-314): none is every family above; some on distinct columns; two on one column with opposite syndrome
    # bits (inf - inf: NaN posteriors, nan_deg1_only == 0)
    cd3 = np.full(640, 3)
    cda = cd3.copy(); cda[[5, 300, 600]] += 1
    add("deg1_distinct", 64, cda, {"uniform": uniform(), "by degree": bydeg}, "WG2", fixed={0: [5], 31: [300], 63: [600]}, row_cap=36,
        claims=dict(deg1_rows=3, deg1_shared=False), detail_set={"uniform": ["DEG1", "NAN_DEG1_ONLY"]}, relay=True, axes=("iter9",),
        variants=("WG_GENERIC", "WG_ROWMAJOR"))
    cdb = cd3.copy(); cdb[5] += 2; cdb[600] += 1
    add("deg1_shared", 64, cdb, {"uniform": uniform(), "by degree": bydeg}, "WG2", fixed={0: [5], 31: [5], 63: [600]}, row_cap=36,
        claims=dict(deg1_rows=3, deg1_shared=True, nan=True), detail_set={"uniform": ["DEG1"]}, detail_clear={"uniform": ["NAN_DEG1_ONLY"]},
        pinned_syndrome={0: 1, 31: 0}, relay=True, golden=True, axes=("B1", "iter1"), variants=("WG_GENERIC", "WG_ROWMAJOR"))
    # odd rows: a first row of full degree 40, every 17th row empty, two identical rows, an all-zero last row
    r = rng_of("odd_rows")
    cd = blocks(r, (6, 128), (4, 256), (1, 64))
    twin = np.sort(r.choice(np.flatnonzero(cd >= 4), 12, replace=False))
    fx = {0: np.flatnonzero(cd > 0)[:40], 3: twin, 4: twin, 119: []}
    fx.update({i: [] for i in range(17, 119, 17)})
    add("odd_rows", 120, cd, {"uniform": uniform(), "by degree": bydeg}, "WG2", fixed=fx, row_cap=24,
        claims=dict(max_row=40, empty_rows=7, twin_rows=(3, 4)), relay=True, axes=("clip6.5",), err_weight=2)

    # ---- the table kernel (minsum_wg.hip) and the hand-over to the streaming kernel ---------------------------------------------------------------
    normal = lambda cd: rng_of("normal").normal(2.5, 1.0, len(cd))          # noqa: E731
    for D, path in ((48, "WG"), (56, "WG"), (57, "STREAM"), (255, "STREAM"), (256, "STREAM")):
        # wg_mode: row degree <= 56 (seven chunks of eight edges); 57 goes to minsum_stream.hip; from 256 on graph.hip builds no ELL tables at all
        r = rng_of(f"rowdeg{D}")
        n = 700 if D < 100 else 1200
        m = 64 if D < 100 else 128
        cd = blocks(r, (5, 200), (3, n - 264), (0, 64))
        add(f"rowdeg{D}", m, cd, {"class": uniform(), "normal": normal}, path, fixed={0: np.flatnonzero(cd > 0)[:D]}, row_cap=36,
            claims=dict(max_row=D), golden=(D == 57), axes=(("iter9",), ("const",), ("seq",), ("clip6.5",), ("B1",))[D % 5],
            detail_clear={"class": ["REG_INDICES"]} if path == "WG" else {}, variants=("WG_GENERIC", "WG_ROWMAJOR") if path == "WG" else ())
    # a hub column that meets every one of 300 rows; a hub row of degree 56 beside rows of degree 2
    r = rng_of("hub_col")
    cd = blocks(r, (3, 600), (2, 100)); cd[17] = 300
    add("hub_col", 300, cd, {"class": uniform(), "normal": normal}, "WG", claims=dict(max_col=300), axes=("seq",), variants=("WG_GENERIC", "WG_ROWMAJOR"))
    r = rng_of("hub_row")
    add("hub_row", 200, np.full(398 + 56, 1), {"class": uniform(), "normal": normal}, "WG", fixed={0: np.arange(56)}, row_cap=2,
        claims=dict(max_row=56, other_rows=2), axes=("iter9",), err_weight=2, variants=("WG_GENERIC", "WG_ROWMAJOR"), dev_query=True)
    # the block switch of minsum_wg_launch: 512 threads up to (m, n) = (512, 4096), 1024 beyond either
    for m, n, big in ((512, 4096, False), (513, 4096, True), (512, 4097, True)):
        r = rng_of(f"block_{m}_{n}")
        add(f"block_{m}_{n}", m, blocks(r, (5, 1024), (2, n - 1024)), {"normal": normal}, "WG", claims=dict(m=m, n=n), err_weight=8, axes=("const",),
            detail_set={"normal": ["BLOCK_1024"]} if big else {}, detail_clear={} if big else {"normal": ["BLOCK_1024"]},
            variants=("WG_GENERIC", "WG_ROWMAJOR"), dev_query=(m == 513))
    # posteriors in global memory by size: n just beyond the all-LDS bound of wg_lds_bytes and the last n within it, with and without damping
    m = 300
    n_lds = max(n for n in range(19000, 21000) if wg_lds_bytes(m, n, False) <= LDS_BYTES)
    for n, vg in ((n_lds, False), (n_lds + 1, True)):
        for damping in (1.0, 0.8):
            r = rng_of("vglobal")
            cd = blocks(r, (4, 1500), (2, 1500), (0, n - 3000))
            add(f"vglobal_{'beyond' if vg else 'within'}_{'damped' if damping != 1.0 else 'plain'}", m, cd, {"normal": normal}, "WG",
                fixed={0: np.flatnonzero(cd > 0)[:56]}, damping=damping, claims=dict(n=n, max_row=56, wg_all_lds=not vg), err_weight=8,
                axes=("iter9",) if damping == 1.0 else ("const",),
                detail_set={"normal": (["VGLOBAL"] if vg else []) + (["DAMPING"] if damping != 1.0 else [])},
                detail_clear={"normal": ([] if vg else ["VGLOBAL"]) + ([] if damping != 1.0 else ["DAMPING"])}, variants=("WG_GENERIC", "WG_ROWMAJOR"))
    # the two small-graph forms, so that the counters of the GPU module see every path: a (6, 3)-regular graph and a small irregular one
    ip = np.arange(0, 6 * 37, 6, dtype=np.int32)
    ix = np.concatenate([np.sort([i, (i + 1) % 36, (i + 3) % 36, 36 + i, 36 + (i + 2) % 36, 36 + (i + 7) % 36]) for i in range(36)]).astype(np.int32)
    rdc, cdc = degrees(ip, ix, 72)
    assert regular_takes(rdc, cdc)
    out.append(_case("regular63", zlib.crc32(b"regular63"), ip, ix, 72, {"uniform": np.full(72, 3.0)}, "REGULAR", claims=dict(regular=(6, 3)), err_weight=2))
    # the largest team of the regular kernel (plan_regular: max(m, (n + 1) / 2) <= 512 threads) and the first graph beyond it, which the resident
    # kernel takes with two checks per thread
    for m, path in ((512, "REGULAR"), (513, "RESIDENT")):
        add(f"reg63_m{m}", m, np.full(2 * m, 3), {"uniform": uniform(3.0)}, path, row_cap=6, claims=dict(regular=(6, 3), m=m, regular_team=(path == "REGULAR")),
            err_weight=40, axes=("iter9",))
    add("small_irregular", 12, blocks(rng_of("si"), (3, 10), (2, 14), (1, 6)), {"uniform": uniform(3.0)}, "RESIDENT", claims=dict(max_row_le=8, max_col_le=4),
        row_cap=8, err_weight=1)
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out

