"""Seeded generator of layered Tanner graphs for sliding-window decoding (csrc/window.hip, qldpc_window_decoder_create in include/qldpc_hip.h).

The packaged circuit-level matrices are structurally one layered matrix: 36 or 72 rows per layer, every interior layer identical, one empty column,
windows that are WG2 graphs (or WG for the whole matrix).  Every family here straddles one line of the window decoder's host code or of the kernels it
hands its windows to that those matrices never reach; the comment beside a family names the line.  A family claims a structure (`claims`), the (W, C)
configurations to run (`configs`), the ones creation must refuse (`refused` {(W, C): layer the refusal names}) and the argument axes it varies (`axes`);
tests/test_window_shapes_cpu.py checks the claims against tests/window_model.py and an independent restatement, tests/test_window_shapes_gpu.py checks the
library against the model.  Plain module (no pytest hooks); deterministic from the seed; CSR rows sorted, no repeated edges.

The decode path a window graph takes is graph_shapes.rule_path (the restatement of the selection rules that tests/test_wg_shapes_gpu.py pins to the
library on both sides of every limit); expected_paths() applies it to the model's window graphs and states no rule of its own.
"""
import zlib
from types import SimpleNamespace

import numpy as np

import graph_shapes as GS
import window_model as WM

MAX_ITER = 20            # of the sweep: small enough that min-sum fails in some windows, large enough that it converges in others
SHOTS = 24


# ---------------------------------------------------------------------------------------- the builder
def _regular42(rng, lr):
    """A (4, 2)-regular block of lr rows and 2 lr columns: column c meets rows c, c + 1 and column lr + c rows c, c + 2 (mod lr), rows permuted."""
    assert lr >= 5
    perm = rng.permutation(lr)
    rows = [set() for _ in range(lr)]
    for c in range(lr):
        for col, other in ((c, c + 1), (lr + c, c + 2)):
            rows[perm[c]].add(col)
            rows[perm[other % lr]].add(col)
    ip = np.concatenate([[0], np.cumsum([len(s) for s in rows])]).astype(np.int32)
    return ip, np.array([c for s in rows for c in sorted(s)], np.int32)


def layered(rng, layer_rows, layers, born, own=(2,), nxt=(1,), own_cap=None, next_cap=None, heavy=None, twins=(), empty_rows=(), empty_cols=0,
            periodic=False, regular42=False):
    """A layered matrix: for every layer t, born[t] columns (an int: the same number everywhere) that are "born" in t, each with a number of rows in
    layer t drawn from `own` (>= 1) and a number of rows in layer t + 1 drawn from `nxt` (0: the column lives in one layer; none in the last layer).
    The columns of a layer are dealt over its rows by graph_shapes.deal with at most own_cap / next_cap entries per row and block.
    heavy {row: D}: that row meets exactly D of its layer's own columns and none of the layer before; twins [(row, row)]: two rows of one layer with the
    same three own columns and nothing else; empty_rows: rows without entries; empty_cols: trailing columns without rows; periodic: one layer pattern
    repeated (the last layer keeps its own block only); regular42: every own block is _regular42 (born = 2 layer_rows).
    -> (indptr int32, indices int32, n, start: first column born in layer t, start[layers] = the first empty column)."""
    lr, heavy = layer_rows, dict(heavy or {})
    born = [born] * layers if np.isscalar(born) else list(born)
    assert len(born) == layers and not (periodic and (heavy or twins or len(empty_rows) or len(set(born)) > 1))
    empty_rows = set(int(r) for r in empty_rows)
    start = np.concatenate([[0], np.cumsum(born)]).astype(np.int64)
    own_blocks, next_blocks = [], []
    for t in range(layers):
        if periodic and t:
            own_blocks.append(own_blocks[0])
            next_blocks.append(next_blocks[0] if t + 1 < layers else None)
            continue
        nb = born[t]
        local = lambda rows: {r - t * lr for r in rows if t * lr <= r < (t + 1) * lr}      # noqa: E731
        if regular42:
            assert nb == 2 * lr
            own_blocks.append(_regular42(rng, lr))
        else:
            d_own = np.minimum(rng.choice(np.asarray(own), nb), lr).astype(np.int64) if nb else np.zeros(0, np.int64)
            fixed = {i: [] for i in local(empty_rows)}
            for r, D in heavy.items():
                if r // lr == t:
                    fixed[r - t * lr] = np.sort(rng.choice(nb, D, replace=False))
            for a, b in twins:
                if a // lr == t:
                    assert b // lr == t
                    cols = np.sort(rng.choice(nb, 3, replace=False))
                    d_own[cols] = np.maximum(d_own[cols], min(3, lr))              # two rows here and a third elsewhere
                    fixed[a - t * lr] = fixed[b - t * lr] = cols
            own_blocks.append(GS.deal(rng, lr, d_own, fixed=fixed, row_cap=own_cap) if nb else (np.zeros(lr + 1, np.int32), np.zeros(0, np.int32)))
        if t + 1 == layers:
            next_blocks.append(None)
            continue
        up = lambda rows: {r - (t + 1) * lr for r in rows if (t + 1) * lr <= r < (t + 2) * lr}      # noqa: E731
        d_next = np.minimum(rng.choice(np.asarray(nxt), nb), lr).astype(np.int64) if nb else np.zeros(0, np.int64)
        fixed = {i: [] for i in up(empty_rows) | up(heavy) | up([r for pair in twins for r in pair])}
        next_blocks.append(GS.deal(rng, lr, d_next, fixed=fixed, row_cap=next_cap) if nb else (np.zeros(lr + 1, np.int32), np.zeros(0, np.int32)))
    indptr, indices = [0], []
    for t in range(layers):
        for i in range(lr):
            if t and next_blocks[t - 1] is not None:
                ip, ix = next_blocks[t - 1]
                indices.extend((start[t - 1] + ix[ip[i]:ip[i + 1]]).tolist())
            ip, ix = own_blocks[t]
            indices.extend((start[t] + ix[ip[i]:ip[i + 1]]).tolist())
            indptr.append(len(indices))
    n = int(start[-1]) + empty_cols
    ip, ix = np.asarray(indptr, np.int32), np.asarray(indices, np.int32)
    # a column is born where the builder says: every one has a row in its own layer (a stub graph_shapes.deal had to drop could leave it without)
    first = np.full(n, layers * lr, np.int64)
    np.minimum.at(first, ix, np.repeat(np.arange(layers * lr), np.diff(ip)))
    for t in range(layers):
        assert (first[start[t]:start[t + 1]] // lr == t).all(), f"a column born in layer {t} has no row there"
    return ip, ix, n, start


# ---------------------------------------------------------------------------------------- cases
def standard_configs(layers, extra=()):
    """The (W, C) pairs every family runs (those that are arguments at all: W >= 1, 1 <= C <= W), without repeats, then `extra`."""
    out = []
    for wc in ((1, 1), (2, 1), (2, 2), (3, 2), (4, 3), (layers, layers), (layers + 3, 2), (layers - 1, layers - 1)) + tuple(extra):
        if wc[0] >= 1 and 1 <= wc[1] <= wc[0] and wc not in out:
            out.append(wc)
    return out


def model(case, prior, W, C):
    return WM.WindowModel(case.indptr, case.indices, case.n, case.priors[prior] if isinstance(prior, str) else prior, case.layer_rows, W, C)


def expected_paths(case, prior, W, C, max_iter=MAX_ITER, clip=20.0):
    """The set of decode paths of the model's window graphs under graph_shapes.rule_path (a host prior: the window decoder keeps one per handle)."""
    return {GS.rule_path(st["indptr"], st["indices"], st["cols"].size, st["prior"], host_prior=True, max_iter=max_iter, clip=clip)
            for st in model(case, prior, W, C).stages}


def syndromes(case, B, salt=0, weight=None):
    """B syndromes of a family, as graph_shapes.syndromes has them: those of random errors of weight w .. 2 w (w = case.err_weight), then (B >= 2) an
    all-zero one last and (B >= 3) a random (unrealisable) one first."""
    rng = np.random.default_rng([case.seed, 11, salt, B])
    w = case.err_weight if weight is None else weight
    E = np.zeros((B, case.n), np.int8)
    for b in range(B):
        E[b, rng.choice(case.n, size=min(case.n, int(rng.integers(w, 2 * w + 1))), replace=False)] = 1
    S = WM.Matrix(case.indptr, case.indices, case.n).parity(E)
    if B >= 3:
        S[0] = rng.random(case.m) < 0.5
    if B >= 2:
        S[-1] = 0
    return S


def big_batch(fams=None):
    """-> (case, prior name, (W, C), 8200 syndromes, max_iter): more shots than the 8192 workgroups the gather and commit kernels launch, so their
    grid-stride loops take a second trip, at a max_iter that leaves more than 2048 shots unconverged in one window (the list the one-wave OSD-0
    kernel works off with tickets)."""
    case = {c.name: c for c in (fams or families())}["lr1"]
    return case, "three values", (3, 2), syndromes(case, 8200, salt=1, weight=3), 2


def _case(name, ip, ix, n, start, layer_rows, priors, **kw):
    m = len(ip) - 1
    layers = m // layer_rows
    c = SimpleNamespace(name=name, seed=zlib.crc32(name.encode()), indptr=ip, indices=ix, n=int(n), m=m, layer_rows=layer_rows, layers=layers, start=start,
                        priors=priors, configs=standard_configs(layers), claims={}, refused={}, axes=(), err_weight=3)
    for k, v in kw.items():
        assert hasattr(c, k), k
        setattr(c, k, v)
    assert set(c.refused) <= set(c.configs)
    return c


# "flags": the selectors every graph accepts; "generic": QLDPC_FLAG_KERNEL_GENERIC, which asks for the resident family and is refused (as by
# qldpc_minsum_decode_batch) on a graph that family does not take, so it goes to families whose windows are all REGULAR or RESIDENT graphs
AXES = ("iter0", "iter1", "iter9", "const", "seq", "clip6.5", "flags", "generic", "big")


def families(seed=20261019):
    """-> list of cases (SimpleNamespace): name, seed, indptr, indices, n, m, layer_rows, layers, start (first column born in every layer), priors
    {name: array}, configs [(W, C)], claims (structure the CPU suite verifies), refused {(W, C): layer}, axes (subset of AXES), err_weight."""
    out = []

    def rng_of(name):
        return np.random.default_rng([seed, zlib.crc32(name.encode())])

    def add(name, lr, layers, born, priors, **kw):
        case_kw = {k: kw.pop(k) for k in ("claims", "refused", "axes", "err_weight", "configs") if k in kw}
        ip, ix, n, start = layered(rng_of(name + "/graph"), lr, layers, born, **kw)
        out.append(_case(name, ip, ix, n, start, lr, {k: np.asarray(v(n), np.float64) for k, v in priors.items()}, **case_kw))
        return out[-1]

    uniform = lambda v=3.0: (lambda n: np.full(n, v))                                 # noqa: E731
    classes = lambda tag, values: (lambda n: GS.by_class(rng_of(tag), n, values))      # noqa: E731

    # layer_rows = 1: windows of one to three rows (and the whole graph, eleven), one word of commit flips, one-wave OSD-0, the resident kernel
    add("lr1", 1, 11, [3, 2, 4, 3, 2, 4, 4, 2, 3, 4, 2], {"uniform": uniform(), "three values": classes("lr1p", [2.5, -1.5, 6.25])},
        own=(1,), nxt=(1, 1, 1, 0), claims=dict(max_row=8, born_range=(2, 4), spans=True), axes=("iter0", "iter1", "big"), err_weight=1)
    # periodic, every own block (4, 2)-regular and every column with a row in the next layer: W = 1 drops those rows and leaves REGULAR graphs, one
    # handle for all of them; the whole matrix and every W >= 2 window are not regular
    add("periodic_r42", 12, 8, 24, {"uniform": uniform()}, nxt=(1,), periodic=True, regular42=True,
        claims=dict(periodic=True, own_regular=(4, 2), all_span=True), axes=("const", "seq", "generic"), err_weight=2)
    # small irregular layers with trailing empty columns, some of them in a negative prior class: committed once, in window 0, with decision 1
    def negative(n):
        p = GS.by_class(rng_of("sip"), n, [3.25, 2.5, -1.5], sizes=[n - 20, 12, 8])
        p[[n - 1, n - 3, n - 4]] = -1.5
        return p
    add("small_irregular", 6, 7, 8, {"uniform": uniform(), "negative class": negative}, own=(1, 2), nxt=(0, 1), own_cap=4, next_cap=3, empty_cols=6,
        claims=dict(max_row=8, max_col=3, empty_cols=6, spans=True), axes=("iter9", "const", "generic"), err_weight=2)
    # layer_rows = 33: a commit region of 66 rows (a ragged third word of flips); row degree above 8 and one column degree class per layer position,
    # so the windows are WG2 graphs; 99 rows are the last window of the one-wave OSD-0, 132 the first of the workgroup elimination
    add("mid_lr33", 33, 6, 150, {"uniform": uniform(4.0), "two classes": classes("midp", [2.5, 7.25])}, own=(2,), nxt=(1,),
        claims=dict(min_max_row=9, all_span=True), axes=("flags", "clip6.5"), err_weight=4)
    # layer_rows = 130: commit regions of 260 and 390 rows (the commit kernel's inner stride), windows wider than 1024 columns, and with W = 8 a window
    # of 1040 rows: the 1024-thread table kernel and the OSD-0 form for m > 1024
    add("wide_lr130", 130, 10, 700, {"uniform": uniform(4.0)}, own=(2,), nxt=(1,), configs=standard_configs(10, extra=((8, 2),)),
        claims=dict(all_span=True), err_weight=10)
    # one own-layer row of degree 48 in layer 1 and one of degree 60 in layer 4: WG, STREAM and lighter window graphs inside one decoder
    add("heavy_rows", 16, 7, 80, {"uniform": uniform(), "normal": lambda n: rng_of("hrp").normal(2.5, 1.0, n)}, own=(1, 2), nxt=(0, 1), own_cap=20,
        heavy={16 + 3: 48, 4 * 16 + 5: 60}, claims=dict(heavy={16 + 3: 48, 4 * 16 + 5: 60}, spans=True), axes=("flags",), err_weight=3)
    # no column born in layer 3 nor in the last layer, every 5th row empty, rows 11 and 12 twins: W = 1 has no columns at layer 3, (7, 7) ends with a
    # window that starts in the last layer; an unrealisable syndrome stays unsatisfied in final rows
    add("gaps", 10, 8, [14, 14, 14, 0, 14, 14, 14, 0], {"uniform": uniform(), "two classes": classes("gapp", [2.5, 6.25])}, own=(1, 2), nxt=(0, 1, 1),
        empty_rows=range(4, 80, 5), twins=[(11, 12)], refused={(1, 1): 3, (7, 7): 7},
        claims=dict(empty_rows=16, twin_rows=(11, 12), unborn_layers=(3, 7), spans=True), axes=("iter0", "iter1"), err_weight=2)
    # one layer: whatever (W, C), one window = the whole graph (rule 7 of the header)
    add("one_layer", 14, 1, 40, {"uniform": uniform(), "three values": classes("olp", [2.5, -1.5, 6.25])}, own=(1, 2, 3), own_cap=8,
        claims=dict(one_layer=True), axes=("iter9",), err_weight=2)
    # sharing is decided by the prior slice: the periodic graph of mid_lr33's kind at three full chunks per layer, with priors that differ in one
    # column by one ulp, in every column, in one sign of zero, and with a class above clip_llr
    def one_ulp(n):
        p = np.full(n, 4.0)
        p[3 * 192 + 17] = np.nextafter(4.0, 5.0)
        return p
    add("prior_variants", 33, 7, 192, {"uniform": uniform(4.0), "one ulp": one_ulp, "all distinct": lambda n: 3.0 + np.arange(n) * 1e-3,
                                       "one -0.0": lambda n: np.concatenate([np.full(3 * 192 + 17, 4.0), [-0.0], np.full(n - 3 * 192 - 18, 4.0)]),
                                       "above clip": lambda n: GS.by_class(rng_of("pvp"), n, [27.0, 4.0], sizes=[n // 8, n - n // 8])},
        own=(2,), nxt=(1,), periodic=True, claims=dict(periodic=True, all_span=True), axes=("const", "seq", "clip6.5"), err_weight=4)
    names = [c.name for c in out]
    assert len(set(names)) == len(names) and all(set(c.axes) <= set(AXES) for c in out)
    return out
