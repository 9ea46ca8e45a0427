"""The workgroup BP kernels (csrc/minsum_wg2.hip, csrc/minsum_wg.hip), their hand-overs and Relay-BP on the structured Tanner graphs of
tests/graph_shapes.py: for every family and prior the library must report the decoder form the family is about (qldpc_minsum_decode_path, which
shares its selection function with the launchers) and every decode must be bit-identical to the CPU checker."""
import os
import sys
import threading

import numpy as np
import pytest

try:
    import torch  # noqa: F401   (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)
except ImportError:
    torch = None

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_shapes as GS  # noqa: E402
import relay_model as RM  # noqa: E402
from conftest import GOLDEN, experiments_lib  # noqa: E402
from test_relay_gpu import PARAM_SETS  # noqa: E402

RELAY_SCALED = PARAM_SETS["scaled"]

pytestmark = pytest.mark.gpu

FAMILIES = GS.families()
BY_NAME = {c.name: c for c in FAMILIES}
# kernel variants that exist in the experiments build only (include/qldpc_hip.h), as in tests/test_gpu_parity.py
XFLAGS = 0x2 | 0x40000 | 0x100000
DETAIL_NAMES = ("LEAN", "REG_INDICES", "VGLOBAL", "DAMPING", "BLOCK_1024", "DEG1", "NAN_DEG1_ONLY")


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        import __graft_entry__
        __graft_entry__.build()
    _lib.require_device()
    return _lib


@pytest.fixture(scope="module")
def LX(L):
    X = experiments_lib()
    if not os.path.exists(X.SO_PATH):
        import __graft_entry__
        __graft_entry__.build()
    X.require_device()
    return X


@pytest.fixture(params=["product", "experiments"])
def Lb(request, L):
    return L if request.param == "product" else request.getfixturevalue("LX")


def for_build(L, variants):
    x = L.BUILD == "experiments"
    return [v for v in variants if bool(v & XFLAGS) == x]


def path_of(L, name):
    return getattr(L, "PATH_" + name)


def detail_names(L, detail):
    return {k for k in DETAIL_NAMES if detail & getattr(L, "DETAIL_" + k)}


def same(got, ref, ctx):
    for x, y, what in zip(got, ref, ("err", "conv", "llr", "iter")):
        x, y = np.asarray(x), np.asarray(y)
        if what == "conv":
            x, y = x.astype(bool), y.astype(bool)
        assert np.array_equal(x, y, equal_nan=(what == "llr")), ctx + (what, int((x != y).sum()))


AXES = {"B1": dict(B=1), "B700": dict(B=700), "iter1": dict(max_iter=1), "iter9": dict(max_iter=9), "const": dict(alpha_mode="alvarado", alpha=0.8),
        "seq": dict(alpha_mode="alvarado-autoregressive", alpha=np.array([0.55, 0.7, 0.9])), "clip6.5": dict(clip_llr=6.5)}
_GRAPHS, _REFS = {}, {}


def graph_of(L, c):
    """one handle per (build, family) for the whole module"""
    key = (L.BUILD, c.name)
    if key not in _GRAPHS:
        _GRAPHS[key] = L.Graph(c.indptr, c.indices, c.n)
    return _GRAPHS[key]


def reference(oracle, c, pn, kw):
    """the checker's answer for one run, computed once for both builds"""
    key = (c.name, pn, kw["B"], kw["max_iter"], kw["alpha_mode"], kw["clip_llr"])
    if key not in _REFS:
        synd = GS.syndromes(c, kw["B"])
        _REFS[key] = (synd, oracle.minsum_decode_batch(c.indptr, c.indices, c.n, synd, c.priors[pn], max_iter=kw["max_iter"], alpha=kw["alpha"],
                                                       alpha_mode=kw["alpha_mode"], damping=c.damping, clip_llr=kw["clip_llr"]))
    return _REFS[key]


@pytest.mark.parametrize("name", [c.name for c in FAMILIES])
def test_family(Lb, oracle, name):
    """Variants per family (trimmed to keep the module short; every family and every prior still runs): the first prior takes the base run (B = 37,
    max_iter = 30) with the automatic form, fixed-work, QLDPC_FLAG_WG_TABLES, the streaming kernel and the family's own flag variants, plus the family's
    axis runs (B = 1 / 700, max_iter = 1 / 9, constant / sequence alpha, clip 6.5) with the automatic form only; later priors take the base run with the
    automatic form and fixed-work.  The experiments build runs its two kernels on the base run of the first prior."""
    L, c = Lb, BY_NAME[name]
    graph = graph_of(L, c)
    product = L.BUILD != "experiments"
    base = dict(B=37, max_iter=30, alpha_mode="dynamical", alpha=1.0, clip_llr=20.0)
    conv = unconv = late = 0
    for pi, (pn, prior) in enumerate(c.priors.items()):
        if pi and not product:
            break
        runs = [dict(base)] + ([dict(base, **AXES[a]) for a in c.axes] if pi == 0 and product else [])
        for ri, kw in enumerate(runs):
            # 1. the library takes the decoder form this family is about, with this run's own arguments (a mismatch is a failure: the case would
            #    test something else)
            args = (kw["max_iter"], kw["alpha_mode"], kw["alpha"])
            path, detail = L.minsum_decode_path(graph, prior, *args, damping=c.damping, clip_llr=kw["clip_llr"])
            assert path == path_of(L, c.expected[pn]), (name, pn, ri, path, c.expected[pn])
            have = detail_names(L, detail)
            assert set(c.detail_set.get(pn, ())) <= have and not (set(c.detail_clear.get(pn, ())) & have), (name, pn, ri, sorted(have))
            if ri == 0 and product:
                if c.expected[pn] == "WG2":               # a flag that asks for the table kernel, and the entry point that has no host prior, get it
                    assert L.minsum_decode_path(graph, prior, *args, flags=L.FLAG_WG_TABLES)[0] == L.PATH_WG
                    assert L.minsum_decode_path(graph, None, *args)[0] == L.PATH_WG
                if c.dev_query:
                    want = GS.rule_path(c.indptr, c.indices, c.n, prior, host_prior=False, damping=c.damping)
                    assert L.minsum_decode_path(graph, None, *args, damping=c.damping)[0] == path_of(L, want), (name, pn)
                assert L.minsum_decode_path(graph, prior, *args, damping=c.damping, flags=L.FLAG_KERNEL_STREAM)[0] == L.PATH_STREAM
            # 2. every variant, bit for bit
            synd, ref = reference(oracle, c, pn, kw)
            if ri == 0:
                cv = np.asarray(ref[1]).astype(bool)
                conv += int(cv.sum()); unconv += int((~cv).sum()); late += int((np.asarray(ref[3]) >= 3).sum())
                if c.claims.get("nan"):
                    assert np.isnan(ref[2]).any(), name
            if not product:
                variants = [L.FLAG_WG_EDGE_LANES, L.FLAG_WG_IDXLOAD]
            elif ri == 0 and pi == 0:
                variants = [0, L.FLAG_FIXED_ITERS, L.FLAG_WG_TABLES, L.FLAG_KERNEL_STREAM] + [getattr(L, "FLAG_" + v) for v in c.variants]
            elif ri == 0:
                variants = [0, L.FLAG_FIXED_ITERS]
            else:
                variants = [0]
            for fl in variants:
                got = L.minsum_decode_batch(graph, synd, prior, kw["max_iter"], kw["alpha_mode"], kw["alpha"], damping=c.damping, clip_llr=kw["clip_llr"], flags=fl)
                same(got, ref, (name, pn, L.BUILD, hex(fl), ri))
    if product:
        assert conv >= 1 and unconv >= 1 and late >= 1, (name, conv, unconv, late)   # the comparison above had something to compare


def test_product_build_query_refuses_the_experiment_flags(L):
    """the query answers as the decode call does: the product library has no kernel for the two experiment selectors"""
    c = BY_NAME["rowdeg41"]
    for fl in (L.FLAG_WG_EDGE_LANES, L.FLAG_WG_IDXLOAD):
        with pytest.raises(L.QldpcError, match="error -4"):
            L.minsum_decode_path(graph_of(L, c), c.priors["uniform"], 30, "dynamical", 1.0, flags=fl)
        with pytest.raises(L.QldpcError, match="error -4"):
            L.minsum_decode_batch(graph_of(L, c), GS.syndromes(c, 3), c.priors["uniform"], 30, "dynamical", 1.0, flags=fl)


def test_six_families_against_the_reference_fixture(L):
    """tests/golden/wg_shapes.npz holds what the reference's own decoder computed on six of the families: the GPU against it directly."""
    with np.load(os.path.join(GOLDEN, "wg_shapes.npz")) as d:
        G = {k: d[k] for k in d.files}
    names = [str(x) for x in G["families"]]
    assert len(names) == 6
    for name in names:
        g = lambda k: G[f"{name}__{k}"]          # noqa: E731
        graph = L.Graph(g("indptr"), g("indices"), int(g("n")))
        for fl in (0, L.FLAG_WG_TABLES, L.FLAG_KERNEL_STREAM):
            got = L.minsum_decode_batch(graph, g("syndromes"), g("prior"), int(g("max_iter")), "dynamical", 1.0, flags=fl)
            same(got, (g("err"), g("conv"), g("llr"), g("iter")), (name, hex(fl)))


def test_every_path_and_every_detail_bit_is_reached(L, LX):
    """Counted like `ran[...]` elsewhere in the suite: over the families, the query reports every QLDPC_PATH_* and every QLDPC_DETAIL_* bit at
    least once (QLDPC_PATH_WAVE exists in the experiments build only, behind its option)."""
    paths, bits = {}, {}
    for c in FAMILIES:
        graph = graph_of(L, c)
        for pn, prior in c.priors.items():
            p, d = L.minsum_decode_path(graph, prior, 30, "dynamical", 1.0, damping=c.damping)
            paths[p] = paths.get(p, 0) + 1
            for k in detail_names(L, d):
                bits[k] = bits.get(k, 0) + 1
            if p in (L.PATH_WG2, L.PATH_WG):               # both states of every bit, not only "set"
                for k in set(DETAIL_NAMES) - detail_names(L, d):
                    bits["not " + k] = bits.get("not " + k, 0) + 1
    print("paths", {k: paths.get(getattr(L, "PATH_" + k), 0) for k in ("REGULAR", "RESIDENT", "WG2", "WG", "STREAM")}, "detail bits", bits)
    for k in ("REGULAR", "RESIDENT", "WG2", "WG", "STREAM"):
        assert paths.get(getattr(L, "PATH_" + k), 0) >= 1, k
    for k in DETAIL_NAMES:
        assert bits.get(k, 0) >= 1 and bits.get("not " + k, 0) >= 1, (k, bits)
    from qldpc_amd.data import load_code
    code = load_code("bb72")
    gx, pr = LX.Graph(code["Hx_indptr"], code["Hx_indices"], code["n"]), np.full(code["n"], 3.0)
    assert LX.minsum_decode_path(gx, pr, 30, "dynamical", 1.0)[0] == LX.PATH_REGULAR
    LX.set_option("regular_kernel", 2)
    try:
        assert LX.minsum_decode_path(gx, pr, 30, "dynamical", 1.0)[0] == LX.PATH_WAVE
    finally:
        LX.set_option("regular_kernel", 0)


_RELAY_SEEN = {"legs": 0, "conv": 0, "unconv": 0, "families": 0}
RELAY_FAMILIES = [c.name for c in FAMILIES if c.relay]


@pytest.mark.parametrize("name", RELAY_FAMILIES)
def test_relay_bp_on_the_wg2_families(L, name):
    """Relay-BP (csrc/relay_bp.hip) keeps the same compressed check state: one parameter set with memory, bit for bit against tests/relay_model.py, on
    every family of the LDS-resident form (an unrealisable syndrome, one of a random error, an all-zero one).  deg1_shared is among them: the NaN that
    two disagreeing degree-1 checks make enters the memory term as 0."""
    c = BY_NAME[name]
    assert c.row_deg.max() <= 56
    graph = graph_of(L, c)
    prior = next(iter(c.priors.values()))
    synd = GS.syndromes(c, 3)
    got = L.relay_decode_batch(graph, synd, prior, 20261016, 3, 1, **RELAY_SCALED)
    ref = RM.relay_decode(c.indptr, c.indices, c.n, synd, prior, 20261016, 3, 1, **RELAY_SCALED)
    for a, b, what in zip(got, ref, ("err", "conv", "legs", "iters", "solutions")):
        assert np.array_equal(a, b), (name, what)
    _RELAY_SEEN["legs"] += int((ref[2] > 1).any()); _RELAY_SEEN["conv"] += int(ref[1].any()); _RELAY_SEEN["unconv"] += int((ref[1] == 0).any())
    _RELAY_SEEN["families"] += 1
    if _RELAY_SEEN["families"] == len(RELAY_FAMILIES):
        # the comparison was about Relay-BP: on most families a relay leg beyond the first ran and both outcomes occurred
        assert min(_RELAY_SEEN["legs"], _RELAY_SEEN["conv"], _RELAY_SEEN["unconv"]) >= len(RELAY_FAMILIES) // 2, _RELAY_SEEN
    assert {c.name for c in FAMILIES if "WG2" in c.expected.values() and c.row_deg.max() <= 56} == set(RELAY_FAMILIES) - {"rowdeg41", "coldeg9", "m1025"}


def test_relay_bp_refuses_row_degree_57(L):
    c = BY_NAME["rowdeg57"]
    graph = L.Graph(c.indptr, c.indices, c.n)
    with pytest.raises(L.QldpcError, match="error -4"):                       # QLDPC_ERR_UNSUPPORTED
        L.relay_decode_batch(graph, GS.syndromes(c, 3), c.priors["class"], 1, **RELAY_SCALED)
    ok = BY_NAME["rowdeg56"]
    L.relay_decode_batch(L.Graph(ok.indptr, ok.indices, ok.n), GS.syndromes(ok, 3), ok.priors["class"], 1, **RELAY_SCALED)


def test_table_cache_across_evictions(L, oracle):
    """One handle, six class-valued priors, three times round (a p-sweep): wg2_prepare keeps four tables and starts over on the fifth distinct
    prior, so this evicts a dozen times.  Every call stays bit-identical to the checker and on the LDS-resident form; then the same from two host
    threads with three priors each, interleaved."""
    c = BY_NAME["nch17"]
    graph = L.Graph(c.indptr, c.indices, c.n)
    synd = GS.syndromes(c, 9)
    priors = [np.where(c.priors["class per chunk"] > 3.0 + 0.25 * k, 2.0 + 0.5 * k, 5.0 + 0.125 * k) for k in range(6)]
    refs = [oracle.minsum_decode_batch(c.indptr, c.indices, c.n, synd, p, max_iter=12) for p in priors]
    assert len({p.tobytes() for p in priors}) == 6

    def one(k):              # the decode call comes first: it is the one that misses, evicts and rebuilds; the query then finds its tables
        same(L.minsum_decode_batch(graph, synd, priors[k], 12, "dynamical", 1.0), refs[k], ("cache", k))
        assert L.minsum_decode_path(graph, priors[k], 12, "dynamical", 1.0)[0] == L.PATH_WG2, k

    for _ in range(3):
        for k in range(6):
            one(k)
    errors = []

    def worker(ks):
        try:
            for _ in range(3):
                for k in ks:
                    one(k)
        except BaseException as e:          # noqa: BLE001  (reported by the parent thread)
            errors.append(e)

    ts = [threading.Thread(target=worker, args=(ks,)) for ks in ((0, 2, 4), (1, 3, 5))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
