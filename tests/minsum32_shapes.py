"""Graph shapes and inputs for the single-precision min-sum decoder (csrc/minsum_f32.hip): one family on either side of every line of its host rules.

The rules below are a SECOND COPY of what minsum32_decoder_create_tab decides, written from include/qldpc_hip.h and the kernel's comments and kept
on purpose as an independent statement: the LDS count and its limit, the clean-input form, and the workgroup size the occupancy query starts from.
Every family is sized by searching these functions (_last), never by a literal; tests/test_minsum32_domain_cpu.py checks every claim against the
rules and the numpy model against the scalar f32 loop on every family, tests/test_minsum32_domain_gpu.py checks the rules against
qldpc_minsum32_decoder_info and every decode against the model.  Plain module (no pytest hooks); deterministic from the seed; CSR rows sorted.
"""
import zlib
from types import SimpleNamespace

import numpy as np

import graph_shapes as GS
import layered_shapes as LSH
import minsum32_model as MM

SEED = 20261021
LDS_BYTES = 160 * 1024
ROW_DEG = 56
GENERIC, BLOCK_256, BLOCK_512, BLOCK_1024 = "GENERIC", "BLOCK_256", "BLOCK_512", "BLOCK_1024"      # QLDPC_FLAG_F32_*
F32 = np.float32
TWO100 = 2.0 ** 100
B = LSH.B


def _up(x, a):
    return (x + a - 1) // a * a


# ---------------------------------------------------------------------------------------- the rules, restated
def lds_bytes(m, n):
    """the header's layout: V f32 | 16-byte records | a byte per row | flags"""
    return _up(_up(4 * n, 16) + 16 * m + m, 16) + 16


def accepted(m, n, max_row_deg):
    return 1 <= m < (1 << 24) and 1 <= n < 65535 and max_row_deg <= ROW_DEG and lds_bytes(m, n) <= LDS_BYTES


def clean(prior, alphas, clip, row_deg, flags=()):
    """QLDPC_F32_FORM_CLEAN: no degree-1 check, |prior32| and clip32 <= 2^100, 0 < alpha32 <= 1024 (all after rounding to f32), and no GENERIC flag.
    alphas: the f64 table of the max_iter iterations."""
    with np.errstate(over="ignore"):
        p32, a32, c32 = np.asarray(prior, np.float64).astype(F32), np.asarray(alphas, np.float64).astype(F32), F32(clip)
    return bool(GENERIC not in flags and c32 <= F32(TWO100) and not (np.asarray(row_deg) == 1).any() and ((a32 > 0) & (a32 <= F32(1024.0))).all()
                and (np.abs(p32) <= F32(TWO100)).all())


def first_block(m, n, lds):
    """the workgroup size the occupancy query starts from: all 1024 threads when LDS holds one workgroup per CU, else by the work of a pass"""
    if LDS_BYTES // lds < 2:
        return 1024
    return 512 if max(m, n // 8) > 256 else 256


def _last(ok, lo, hi):
    x = max(v for v in range(lo, hi) if ok(v))
    assert x + 1 < hi and not ok(x + 1)
    return x


def next32(x):
    """the next f32 above x, as an f64"""
    return float(np.nextafter(F32(x), F32(np.inf)))


# ---------------------------------------------------------------------------------------- the families
def rng_of(name):
    return np.random.default_rng([SEED, zlib.crc32(name.encode())])


def _case(name, ip, ix, n, prior, claims, runs=((),), alpha=("dynamical", 1.0), clip=20.0, max_iter=5, err_weight=3, light=(1, 2)):
    """runs: the flag sets the GPU module decodes with; claims: accepted, clean (without flags), first_block"""
    ip, ix = np.asarray(ip, np.int32), np.asarray(ix, np.int32)
    return SimpleNamespace(name=name, seed=zlib.crc32(name.encode()), indptr=ip, indices=ix, n=int(n), m=len(ip) - 1, nnz=len(ix), prior=prior, claims=claims,
                           runs=tuple(tuple(r) for r in runs), alpha=alpha, clip=clip, max_iter=max_iter, err_weight=err_weight, light=tuple(light), row_deg=np.diff(ip))


def alphas_of(c, max_iter=None):
    """the f64 alpha table of the family"""
    tab = {"dynamical": lambda k: 1.0 - 2.0 ** (-(k + 1)), "const": lambda k: float(c.alpha[1])}[c.alpha[0]]
    return np.array([tab(k) for k in range(max_iter or c.max_iter)])


def expected(c, flags=()):
    lds = lds_bytes(c.m, c.n)
    forced = max([int(f[6:]) for f in flags if f.startswith("BLOCK_")] + [0])
    return dict(accepted=accepted(c.m, c.n, int(c.row_deg.max(initial=0))), lds_bytes=lds, clean=clean(c.prior, alphas_of(c), c.clip, c.row_deg, flags),
                first_block=forced or first_block(c.m, c.n, lds), forced=bool(forced), one_wg=LDS_BYTES // lds < 2)


def rows_at_n64(m, name):
    """200 rows of degree 5 scattered over m rows, every other row empty (the *_vg_* recipe of tests/leg_shapes.py)"""
    full = np.sort(rng_of(name + "/rows").choice(m - 1, 200, replace=False))
    cd = np.full(64, 15)
    cd[rng_of(name + "/cd").choice(64, 40, replace=False)] = 16
    return GS.deal(rng_of(name + "/graph"), m, cd, fixed={i: [] for i in np.setdiff1d(np.arange(m), full).tolist()}, row_cap=5)


def clean_graph():
    """60 rows of degree 15 on 300 columns of degree 3: no degree-1 row"""
    return GS.deal(rng_of("clean/graph"), 60, np.full(300, 3))


def queue_case():
    """the graph of the second-shot and last-pass tests: the one above and a row without entries"""
    ip, ix = GS.deal(rng_of("clean/graph"), 61, np.full(300, 3), fixed={60: []})
    return _case("queue", ip, ix, 300, rng_of("queue/prior").normal(2.5, 1.0, 300), dict(accepted=True, clean=True, first_block=256), runs=((), (GENERIC,)),
                 max_iter=9, err_weight=2)


# max_iter at which one shot of the pool first satisfies its syndrome in the pass that only tests (it == max_iter) and another is one iteration short;
# tests/test_minsum32_domain_cpu.py::test_the_last_pass_pair_exists finds the shots with the model and keeps this true
LAST_PASS = dict(max_iter=4, weight=3, pool=64)


def families():
    out = []
    normal = lambda name, n: rng_of(name + "/prior").normal(2.5, 1.0, n)      # noqa: E731
    ip, ix = LSH.core300()
    # ---- the LDS line on the column side: n grown at m = 300, a column of degree 0 apart
    n_last = _last(lambda n: lds_bytes(300, n) <= LDS_BYTES, 30000, 65534)
    assert n_last + 1 < 65535
    for name, n, ok in (("cols_last", n_last, True), ("cols_refused", n_last + 1, False)):
        out.append(_case(name, ip, LSH.spread(rng_of("cols_line"), ix, 3000, n_last), n, normal("cols", n_last + 1)[:n],
                         dict(accepted=ok, clean=True, first_block=1024, line="LDS, columns"), max_iter=4))
    # ---- ... and on the row side: m grown at n = 64, an empty last row apart
    m_last = _last(lambda m: lds_bytes(m, 64) <= LDS_BYTES, 4000, 12000)
    for name, m, ok in (("rows_last", m_last, True), ("rows_refused", m_last + 1, False)):
        ip_, ix_ = rows_at_n64(m_last, "rows_line")
        if not ok:
            ip_ = np.append(ip_, ip_[-1])
        out.append(_case(name, ip_, ix_, 64, GS.by_class(rng_of("rows/prior"), 64, [-1.5, 1.7, 4.0], sizes=[8, 16, 40]),
                         dict(accepted=ok, clean=True, first_block=1024, line="LDS, rows"), max_iter=4, err_weight=2))
    # ---- one workgroup per CU (1024 threads) | two: the last n at m = 300 with room for two and the first without
    n_two = _last(lambda n: LDS_BYTES // lds_bytes(300, n) >= 2, 10000, 30000)
    for name, n, blk in (("two_wg_last", n_two, 512), ("one_wg_first", n_two + 1, 1024)):
        out.append(_case(name, ip, LSH.spread(rng_of("wg_line"), ix, 3000, n_two), n, normal("wg", n_two + 1)[:n],
                         dict(accepted=True, clean=True, first_block=blk, line="one workgroup per CU"), max_iter=4))
    # ---- m = 1500 at a forced 256 threads (six trips of the row loop) and 1024: empty rows, degree-1 rows, columns of degree 0
    r = rng_of("rows_1500")
    cd = GS.blocks(r, (12, 400), (6, 200), (0, 100))
    live = np.flatnonzero(cd > 0)
    fixed = {int(i): [] for i in range(5, 1500, 97)}
    fixed.update({int(i): [int(live[k])] for k, i in enumerate(range(11, 1500, 131))})
    ip_, ix_ = GS.deal(rng_of("rows_1500/graph"), 1500, cd, fixed=fixed, row_cap=20)
    out.append(_case("rows_1500", ip_, ix_, 700, normal("rows_1500", 700), dict(accepted=True, clean=False, first_block=512), runs=((BLOCK_256,), (BLOCK_1024,)),
                     max_iter=6, light=(6, 6)))
    # ---- the lines of the clean form, each on the graph without degree-1 rows, decoded in both forms where both exist
    ipc, ixc = clean_graph()
    base = normal("clean", 300)

    def with_entries(**at):
        p = base.copy()
        for j, v in at.items():
            p[int(j[1:])] = v
        return p
    # light: the weight of the error of shot 1 at which the model converges after iteration 0 (searched per family; the alpha families have none)
    for name, prior, alpha, clip, is_clean, light in (
            ("alpha_1024", base, 1024.0, 20.0, True, 1), ("alpha_above", base, next32(1024.0), 20.0, False, 1),
            ("clip_2p100", base, 0.875, TWO100, True, 1), ("clip_2p101", base, 0.875, 2.0 ** 101, False, 1),
            ("prior_2p100", with_entries(c7=TWO100, c150=-TWO100), 0.875, 20.0, True, 4),
            ("prior_above", with_entries(c7=TWO100, c150=-next32(TWO100)), 0.875, 20.0, False, 2),
            ("prior_rounds_to_2p100", with_entries(c7=TWO100 * (1.0 + 2.0 ** -30), c150=-TWO100 * (1.0 + 2.0 ** -30)), 0.875, 20.0, True, 3)):
        out.append(_case(name, ipc, ixc, 300, prior, dict(accepted=True, clean=is_clean, first_block=256, line="clean"),
                         runs=((), (GENERIC,)) if is_clean else ((),), alpha=("const", alpha), clip=clip, max_iter=6, light=(light, 2)))
    # ---- everything at its bound at once: a column of degree 300 (the hub_col recipe of tests/graph_shapes.py), every prior +-2^100, alpha 1024, clip 2^100
    r = rng_of("extreme")
    cd = GS.blocks(r, (3, 600), (2, 100))
    cd[17] = 300
    ip_, ix_ = GS.deal(rng_of("extreme/graph"), 300, cd)
    out.append(_case("extreme", ip_, ix_, 700, TWO100 * r.choice([-1.0, 1.0], 700), dict(accepted=True, clean=True, first_block=512), runs=((), (GENERIC,)),
                     alpha=("const", 1024.0), clip=TWO100, max_iter=6, light=(5, 2)))
    # ---- no edges at all: creation accepts it (every row has degree 0, the column loop runs no trip); a shot converges iff its syndrome is 0
    out.append(_case("no_edges", np.zeros(6, np.int32), np.zeros(0, np.int32), 7, normal("no_edges", 7), dict(accepted=True, clean=True, first_block=256)))
    out.append(queue_case())
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


_CASES, _REF = [], {}


def all_cases():
    if not _CASES:
        _CASES.extend(families())
    return _CASES


def shots(c):
    return LSH.syndromes(c, c.prior)


def last_pass_pool(c, weight, count):
    return LSH.last_pass_pool(c, weight, count)


def model_decode(c, synd, max_iter=None):
    """the numpy model on the family's inputs; a graph without edges is beyond its gathers, so there the answer is written down: V = prior32"""
    T = max_iter or c.max_iter
    if c.nnz == 0:
        with np.errstate(over="ignore"):
            V = np.tile(np.asarray(c.prior, np.float64).astype(F32), (len(synd), 1))
        conv = (~(np.asarray(synd) & 1).any(axis=1)).astype(np.uint8)
        return (V < 0).astype(np.int8), conv, V.astype(np.float64), np.where(conv == 1, 0, T - 1).astype(np.int32)
    return MM.Minsum32Model(c.indptr, c.indices, c.n, c.prior).decode(synd, max_iter=T, alpha_mode=c.alpha[0], alpha=c.alpha[1], clip_llr=c.clip)


def reference(c):
    """the model's decode of the family's eight shots; computed once, shared, never changed"""
    if c.name not in _REF:
        ref = model_decode(c, shots(c))
        for a in ref:
            a.setflags(write=False)
        _REF[c.name] = ref
    return _REF[c.name]
