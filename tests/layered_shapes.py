"""Graph shapes for the layered-schedule min-sum decoder (csrc/minsum_layered.hip): one family on either side of every line of its host rules.

The rules below are a SECOND COPY of what layered_decoder_create_tab decides, written from include/qldpc_hip.h and the kernel's comments and kept on
purpose as an independent statement: the LDS layout and its four storage forms, the workgroup size, the lanes a layer gives each check and the grid.
Every family is sized by searching these functions (_last), never by a literal, and carries what it claims to hit (form, block, the set of lg over
its layers); tests/test_layered_domain_cpu.py checks the claims against the rules and the numpy model against the scalar loop on every family,
tests/test_layered_domain_gpu.py checks the rules against qldpc_layered_decoder_info field by field and every decode against the model.  A limit
that moves in csrc/ fails there and has to be moved here too.  Plain module (no pytest hooks); deterministic from the seed; CSR rows sorted.
"""
import zlib
from types import SimpleNamespace

import numpy as np

import graph_shapes as GS
import layered_model as LM

SEED = 20261021
LDS_BYTES = 160 * 1024 - 512                      # a CU's LDS less what the kernel keeps for its own barrier reduction
ROW_DEG = 56                                      # sign bits of a check record
LANE_EDGES = 8                                    # edges a lane holds
THREADS_PER_CU = 2048
FORMS = ("V+idx", "V", "VG+idx", "VG")            # in the order they are tried: posteriors and u16 indices in LDS; posteriors only; indices only; neither
B = 8


def _up(x, a):
    return (x + a - 1) // a * a


# ---------------------------------------------------------------------------------------- the rules, restated
def lds_bytes(n, nslots, nlayers, nnz, vg, idxl):
    """[V f64 per column] | a 16-byte and an 8-byte record per slot | nslots + 1 edge offsets | nlayers + 1 layer words | a syndrome byte per slot |
    [a u16 column index per edge] | 16 bytes of flags; V, the indices and the flags start on 16 bytes."""
    o = 0 if vg else _up(8 * n, 16)
    o += 16 * nslots + 8 * nslots + 4 * (nslots + 1) + 4 * (nlayers + 1)
    o = _up(o + nslots, 16)
    o = _up(o + (2 * nnz if idxl else 0), 16)
    return o + 16


def form(n, nslots, nlayers, nnz, vglobal=False, global_idx=False):
    """-> (name of the first form that fits, its bytes), or (None, bytes of the smallest form) when none does.  The u16 indices exist for n <= 65535;
    the two flags take forms away, they never add one."""
    bytes_ = 0
    for k, name in enumerate(FORMS):
        vg, idxl = k >= 2, k % 2 == 0
        if (idxl and (n > 65535 or global_idx)) or (not vg and vglobal):
            continue
        bytes_ = lds_bytes(n, nslots, nlayers, nnz, vg, idxl)
        if bytes_ <= LDS_BYTES:
            return name, bytes_
    return None, bytes_


def block(nnz, nlayers, forced=0):
    """threads per workgroup: by the edges of an average layer"""
    if forced:
        return forced
    mean = nnz // nlayers if nlayers else 0
    return 256 if mean <= 512 else 512 if mean <= 1024 else 1024


def _ceil_log2(x):
    return int(x - 1).bit_length() if x > 1 else 0


def lane_bits(cnt, maxdeg, block_):
    """lg: 2^lg lanes per check.  At most eight edges per lane; then twice the lanes while a lane still has an edge ("edge"), the layer still fits the
    workgroup ("fit") and a check has no more than a wave ("cap").  -> (lg, the condition that stopped the widening).  A row has at most 56 edges, so
    at lg = 6 (64 lanes) "edge" has stopped the loop whenever "cap" would: the cap is never the only reason, no graph can separate it from "edge", and
    it is not reported here for a degree the decoder accepts.  lg is not a field of qldpc_layered_decoder_info: the sets a family claims are statements
    about this restated rule; the GPU module sees lg only through the outputs (a wrong lane count loses or repeats edges of a check)."""
    lg = _ceil_log2(-(-max(maxdeg, 1) // LANE_EDGES))
    while True:
        if (1 << lg) >= max(maxdeg, 1):
            return lg, "edge"
        if (cnt << (lg + 1)) > block_:
            return lg, "fit"
        if lg >= 6:
            return lg, "cap"
        lg += 1


def grid_per_cu(lds, block_):
    """workgroups per compute unit of the persistent grid"""
    return max(1, min(LDS_BYTES // lds, THREADS_PER_CU // block_))


def structure(indptr, indices, n, row_layer=None):
    """-> (row_layer, [(rows, max degree, edges) per layer that runs])"""
    deg = np.diff(indptr)
    lay = LM.greedy_layers(indptr, indices, n) if row_layer is None else np.asarray(row_layer)
    out = []
    for v in np.unique(lay[deg > 0]):
        d = deg[(lay == v) & (deg > 0)]
        out.append((len(d), int(d.max()), int(d.sum())))
    return lay, out


def expected(c):
    """what qldpc_layered_decoder_info must report for the family, by the rules above; accepted = False: creation is refused"""
    _, layers = structure(c.indptr, c.indices, c.n, c.row_layer)
    ns, nl = sum(t[0] for t in layers), len(layers)
    forced = max([int(f[6:]) for f in c.flags if f.startswith("BLOCK_")] + [0])
    name, bytes_ = form(c.n, ns, nl, c.nnz, vglobal="VGLOBAL" in c.flags, global_idx="GLOBAL_IDX" in c.flags)
    blk = block(c.nnz, nl, forced)
    lanes = [lane_bits(cnt, md, blk) for cnt, md, _ in layers]
    return dict(accepted=name is not None and int(np.diff(c.indptr).max(initial=0)) <= ROW_DEG, form=name, lds_bytes=bytes_, block=blk, nslots=ns,
                layers=nl, max_layer_rows=max([t[0] for t in layers] + [0]), max_layer_edges=max([t[2] for t in layers] + [0]),
                lgs={lg for lg, _ in lanes}, stops={(lg, why) for lg, why in lanes}, wraps=[cnt << lg > blk for (cnt, _, _), (lg, _) in zip(layers, lanes)],
                v_global=name in ("VG+idx", "VG"), lds_indices=name in ("V+idx", "VG+idx"), grid_per_cu=grid_per_cu(bytes_, blk) if name else 0)


def _last(ok, lo, hi):
    """the last x in lo .. hi with ok(x), which is followed by one without"""
    x = max(v for v in range(lo, hi) if ok(v))
    assert x + 1 < hi and not ok(x + 1)
    return x


# ---------------------------------------------------------------------------------------- builders
def rng_of(name):
    return np.random.default_rng([SEED, zlib.crc32(name.encode())])


def layered_rows(rng, n, layer_degs, empty_at=()):
    """Rows given layer by layer: the rows of a layer take disjoint slices of a random permutation of the columns.  empty_at: row indices (of the
    result) of rows without entries, layer 0.  -> (indptr, indices, row_layer)"""
    rows, lay = [], []
    for L, degs in enumerate(layer_degs):
        perm, o = rng.permutation(n), 0
        assert sum(degs) <= n
        for d in degs:
            rows.append(np.sort(perm[o:o + d]))
            lay.append(L)
            o += d
    for i in sorted(empty_at):
        rows.insert(i, np.zeros(0, np.int64))
        lay.insert(i, 0)
    ip = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return ip, np.concatenate(rows + [np.zeros(0, np.int64)]).astype(np.int32), np.array(lay, np.int32)


def spread(rng, indices, ncore, n):
    """the ncore columns of a core graph at ascending random places among n: every other column has degree 0 and the colouring does not change"""
    return np.sort(rng.choice(n, ncore, replace=False)).astype(np.int32)[indices]


def even_degrees(nnz, rows):
    """nnz edges over `rows` rows as evenly as possible"""
    return [nnz // rows + (1 if r < nnz % rows else 0) for r in range(rows)]


def syndrome_of(c, e):
    """H e over GF(2) for one error e[n]"""
    par = np.zeros(c.m, np.int64)
    np.add.at(par, np.repeat(np.arange(c.m), np.diff(c.indptr)), np.asarray(e, np.int64)[c.indices])
    return (par & 1).astype(np.int8)


def syndromes(c, prior):
    """B = 8 distinct kinds of shot: an unrealisable one; a light random error (weight c.light[0], on the columns with edges) on top of the prior's own
    hard decision, and one (weight c.light[1]) on top of the zero word -- the shots that converge after some iterations, with messages that are not
    those of the first pass, under a prior with and without negative entries; an error of weight err_weight .. 2 err_weight; a single 1 on a row
    with entries; a single 1 on a row without (when the graph has one; else one more error); the syndrome of the prior's own hard decision, which
    converges in iteration 0 (every message of a satisfied check has the sign of its Q); all zero."""
    rng = np.random.default_rng([SEED, c.seed, 7])
    deg = np.diff(c.indptr)
    live = np.flatnonzero(np.bincount(c.indices, minlength=c.n))
    S = np.zeros((B, c.m), np.int8)
    S[0] = rng.random(c.m) < 0.5
    if live.size:
        for b in (1, 2, 3, 5):
            e = np.zeros(c.n, np.int64)
            w = c.light[b - 1] if b <= 2 else int(rng.integers(c.err_weight, 2 * c.err_weight + 1))
            e[rng.choice(live, size=min(live.size, w), replace=False)] = 1
            S[b] = syndrome_of(c, e ^ (np.asarray(prior) < 0) if b == 1 else e)
        S[4, rng.choice(np.flatnonzero(deg > 0))] = 1
    else:
        S[1:5] = rng.random((4, c.m)) < 0.3
        S[1, 0] = 1
    if (deg == 0).any():
        S[5] = 0
        S[5, rng.choice(np.flatnonzero(deg == 0))] = 1
    S[6] = syndrome_of(c, np.asarray(prior) < 0)
    return S


# ---------------------------------------------------------------------------------------- the families
def _case(name, ip, ix, n, row_layer, claims, flags=(), max_iter=5, err_weight=3, light=(1, 2)):
    ip, ix = np.asarray(ip, np.int32), np.asarray(ix, np.int32)
    c = SimpleNamespace(name=name, seed=zlib.crc32(name.encode()), indptr=ip, indices=ix, n=int(n), m=len(ip) - 1, nnz=len(ix), row_layer=row_layer,
                        flags=tuple(flags), claims=claims, max_iter=max_iter, err_weight=err_weight, light=tuple(light))
    # "uniform": every |Q| of the first pass is equal, so minimum and second minimum tie in every check and across every lane of a check
    c.priors = {"normal": rng_of(name + "/prior").normal(2.5, 1.0, c.n), "uniform": np.full(c.n, 4.0)}
    return c


def core300():
    """m = 300, 3000 columns of degree 4 and 2, a first row of degree 56 (the vglobal_* recipe of tests/graph_shapes.py)"""
    cd = GS.blocks(rng_of("core300/cd"), (4, 1500), (2, 1500))
    return GS.deal(rng_of("core300/graph"), 300, cd, fixed={0: np.arange(56)}, row_cap=ROW_DEG)


def queue_graph():
    """the graph of the second-shot and last-pass tests: 60 rows of degree 15 on 300 columns of degree 3 and a row without entries"""
    ip, ix = GS.deal(rng_of("queue/graph"), 61, np.full(300, 3), fixed={60: []})
    return _case("queue", ip, ix, 300, None, dict(form="V+idx", block=256, lgs={4}), max_iter=9, err_weight=2)


# max_iter at which one of these shots first satisfies its syndrome in the last pass and another is one iteration short (found with the model by
# tests/test_layered_domain_cpu.py::test_the_last_pass_pair_exists, which also keeps it true): errors of the given weight, seeded by the index
LAST_PASS = dict(max_iter=4, weight=3, pool=64)


def last_pass_pool(c, weight, count):
    """`count` syndromes of random errors of one weight"""
    rng = np.random.default_rng([SEED, c.seed, 11])
    S = np.zeros((count, c.m), np.int8)
    for b in range(count):
        e = np.zeros(c.n, np.int64)
        e[rng.choice(c.n, weight, replace=False)] = 1
        S[b] = syndrome_of(c, e)
    return S


def last_pass_pair(decode, pool, T):
    """decode(syndromes, max_iter) -> the four outputs.  -> (the shots that converge in iteration T - 1, the last of max_iter = T; the shots that
    converge in iteration T, which max_iter = T cuts one iteration short)"""
    at, beyond = decode(pool, T), decode(pool, T + 1)
    hit = np.flatnonzero((at[1] == 1) & (at[3] == T - 1))
    short = np.flatnonzero((beyond[1] == 1) & (beyond[3] == T))
    assert np.all(at[1][short] == 0) and np.all(at[3][short] == T - 1)
    return hit, short


def last_pass_batch(hit, short, count):
    """-> (B = 8 shots of the pool: up to three that converge in the last pass, up to three that are one iteration short, the rest the first others;
    where the first and the second kind stand in it)"""
    h, s = [int(b) for b in hit[:3]], [int(b) for b in short[:3]]
    pick = h + s + [b for b in range(count) if b not in h + s][:B - len(h) - len(s)]
    return np.array(pick), np.arange(len(h)), len(h) + np.arange(len(s))


def families():
    out = []
    # ---- posteriors in LDS | in HBM/L2 (forms V | VG+idx): n grown at m = 300; the two graphs differ in one column of degree 0
    ip, ix = core300()
    _, lay = structure(ip, ix, 3000)
    ns, nl, nnz = sum(t[0] for t in lay), len(lay), len(ix)
    out.append(_case("core300", ip, ix, 3000, None, dict(form="V+idx", block=256, lgs={3, 4, 5}), max_iter=6))
    n_v = _last(lambda n: lds_bytes(n, ns, nl, nnz, False, False) <= LDS_BYTES, 10000, 30000)
    for name, n, f in (("v_last", n_v, "V"), ("vg_first", n_v + 1, "VG+idx")):
        out.append(_case(name, ip, spread(rng_of("v_line"), ix, 3000, n_v), n, None, dict(form=f, block=256, lgs={3, 4, 5}, line="V | VG")))
    # ---- n = 65535 | 65536: the last n with u16 indices and the first without
    for n, f in ((65535, "VG+idx"), (65536, "VG")):
        out.append(_case(f"n{n}", ip, spread(rng_of("n16"), ix, 3000, 65535), n, None, dict(form=f, block=1024, lgs={5}, line="u16 | i32 indices"),
                         flags=("BLOCK_1024",), max_iter=4))
    # ---- indices in LDS | in HBM/L2 beside posteriors in LDS (V+idx | V): nnz grown at n = 16000, 300 rows in two layers of the caller's
    n, R = 16000, 300
    z = _last(lambda z: lds_bytes(n, R, 2, z, False, True) <= LDS_BYTES, R, ROW_DEG * R)
    for name, nnz_, f in (("idx_last", z, "V+idx"), ("idx_global_first", z + 1, "V")):
        d = even_degrees(nnz_, R)
        ip_, ix_, lay_ = layered_rows(rng_of("idx_line"), n, [d[0::2], d[1::2]])
        out.append(_case(name, ip_, ix_, n, lay_, dict(form=f, block=1024, lgs={3}, line="V+idx | V"), max_iter=4, light=(2, 2)))
    # ---- the same beside posteriors in HBM/L2 (VG+idx | VG): nnz grown at n = 24000, 1300 rows in four layers
    n, R = 24000, 1300
    z = _last(lambda z: lds_bytes(n, R, 4, z, True, True) <= LDS_BYTES, R, ROW_DEG * R)
    for name, nnz_, f in (("vg_idx_last", z, "VG+idx"), ("vg_only_first", z + 1, "VG")):
        d = even_degrees(nnz_, R)
        ip_, ix_, lay_ = layered_rows(rng_of("vg_idx_line"), n, [d[k::4] for k in range(4)])
        out.append(_case(name, ip_, ix_, n, lay_, dict(form=f, block=1024, lgs={3}, line="VG+idx | VG"), max_iter=3, err_weight=6))
    # ---- rows at n = 64: rows of degree 2, 32 to a layer (the greedy colouring finds exactly these layers), every 150th row empty.  The last count
    # whose posteriors stay in LDS, the first that moves them out (V | VG), the last accepted and the first refused
    n = 64

    def rows_case(name, rows_, claims):
        degs = [[2] * min(32, rows_ - 32 * L) for L in range(-(-rows_ // 32))]
        ip_, ix_, _ = layered_rows(rng_of("rows_line"), n, degs, empty_at=tuple(range(7, rows_, 150)))
        return _case(name, ip_, ix_, n, None, claims, max_iter=3, err_weight=1)
    bytes_of = lambda r, vg: lds_bytes(n, r, -(-r // 32), 2 * r, vg, False)   # noqa: E731
    r_v = _last(lambda r: bytes_of(r, False) <= LDS_BYTES, 4000, 7000)
    r_vg = _last(lambda r: bytes_of(r, True) <= LDS_BYTES, 4000, 7000)
    for name, r, f in (("rows_v_last", r_v, "V"), ("rows_vg_first", r_v + 1, "VG"), ("rows_vg_last", r_vg, "VG"), ("rows_refused", r_vg + 1, None)):
        out.append(rows_case(name, r, dict(form=f, block=256, lgs={1}, line="V | VG at n = 64" if "v_" in name or "first" in name else "VG | refused")))
    # ---- the workgroup size: one layer of disjoint rows with 512, 513, 1024 and 1025 edges
    for nnz_, blk, lgs in ((512, 256, {2}), (513, 512, {3}), (1024, 512, {2}), (1025, 1024, {3})):
        degs = [8] * (nnz_ // 8 - 1) + [8 + nnz_ % 8]
        ip_, ix_, lay_ = layered_rows(rng_of(f"block{nnz_}"), 1100, [degs])
        out.append(_case(f"block_nnz{nnz_}", ip_, ix_, 1100, None, dict(form="V+idx", block=blk, lgs=lgs, line="block")))
    # ---- more lanes than threads: 40 rows of degree 56 with eight lanes each at 256 threads (a second trip of eight checks: one full wave, three idle),
    # 5 such rows (widened to 32 lanes each), 37 such rows (the second trip is five groups of eight in one wave, its other lanes idle in the shuffles)
    ip_, ix_, lay_ = layered_rows(rng_of("lanes_wrap"), 2240, [[56] * 40, [56] * 5, [56] * 37])
    out.append(_case("lanes_wrap", ip_, ix_, 2240, lay_, dict(form="V+idx", block=256, lgs={3, 5}, wraps=[True, False, True]), flags=("BLOCK_256",)))
    # ---- one layer with rows of degree 1, 2, 8, 9, 33 and 56: idle lanes carry (inf, 127) into the combine; once six rows, once four of each
    mixed = [1, 2, 8, 9, 33, 56]
    ip_, ix_, lay_ = layered_rows(rng_of("lanes_mixed"), 500, [mixed, mixed * 4], empty_at=(3,))
    out.append(_case("lanes_mixed", ip_, ix_, 500, lay_, dict(form="V+idx", block=256, lgs={3, 5})))
    # ---- every lg: a whole wave per check (1, 2 and 4 rows of degree 33 .. 56), and one layer per other value, stopped by "edge" and by "fit" (the
    # two conditions a graph can separate, see lane_bits)
    degs = [[56], [33, 40], [34, 47, 56, 50],       # lg 6, "edge" (and the cap with it)
            [1] * 9,                                # lg 0, "edge" at once
            [2, 2, 1],                              # lg 1, "edge"
            [8] * 40,                               # lg 2, "fit": 40 << 2 is 160, 40 << 3 is 320
            [4, 3, 4],                              # lg 2, "edge"
            [8, 7, 5],                              # lg 3, "edge"
            [56] * 10,                              # lg 4, "fit"
            [20, 17]]                               # lg 5, "edge"
    ip_, ix_, lay_ = layered_rows(rng_of("lanes_whole_wave"), 600, degs, empty_at=(0, 20))
    out.append(_case("lanes_whole_wave", ip_, ix_, 600, lay_, dict(form="V+idx", block=256, lgs={0, 1, 2, 3, 4, 5, 6},
                                                                 stops={(6, "edge"), (0, "edge"), (1, "edge"), (2, "fit"), (2, "edge"), (3, "edge"), (4, "fit"),
                                                                        (5, "edge")})))
    # ---- no edges at all: creation accepts it (nothing is read through a table of length 0, no layer runs); a shot converges iff its syndrome is 0
    out.append(_case("no_edges", np.zeros(6, np.int32), np.zeros(0, np.int32), 7, None, dict(form="V+idx", block=256, lgs=set())))
    out.append(queue_graph())
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


_CASES, _REF = [], {}


def all_cases():
    if not _CASES:
        _CASES.extend(families())
    return _CASES


def shots(c):
    """the family's eight syndromes, the same for both priors (shots 1 and 6 belong to the "normal" one)"""
    return syndromes(c, c.priors["normal"])


def reference(c, prior_name, max_iter=None):
    """the model's decode of the family's eight shots (alpha 'dynamical', clip 20); computed once, shared, never changed"""
    key = (c.name, prior_name, max_iter or c.max_iter)
    if key not in _REF:
        ref = LM.LayeredModel(c.indptr, c.indices, c.n, c.priors[prior_name], row_layer=c.row_layer).decode(shots(c), max_iter=key[2])
        for a in ref:
            a.setflags(write=False)
        _REF[key] = ref
    return _REF[key]
