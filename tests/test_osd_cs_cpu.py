"""OSD-CS without a GPU: the numpy model (tests/osd_cs_model.py) against the reference's OSD-0 and against a brute-force enumeration that
solves every candidate on its own; argument checks of the Python layer and run_simulation; the binding."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import osd_cs_model as M  # noqa: E402


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    return _lib


def _graph(H):
    H = np.asarray(H, np.int8)
    rows, cols = np.nonzero(H)
    indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=H.shape[0]))])
    return M.Graph(indptr, cols, H.shape[1])


def _solve(H, rhs, cols):
    """the unique x on `cols` (independent columns) with H[:, cols] x = rhs over GF(2), or None when there is none"""
    A = np.concatenate([H[:, cols] % 2, rhs[:, None] % 2], axis=1).astype(np.uint8)
    m, k = A.shape[0], len(cols)
    r = 0
    where = []
    for c in range(k):
        piv = next((i for i in range(r, m) if A[i, c]), None)
        if piv is None:
            return None
        A[[r, piv]] = A[[piv, r]]
        for i in range(m):
            if i != r and A[i, c]:
                A[i] ^= A[r]
        where.append(r)
        r += 1
    if A[r:, k].any():
        return None
    return np.array([A[where[c], k] for c in range(k)], np.uint8)


def brute_force(H, synd, llr, hard, w, order):
    """(solution, flips) by the definition: pivots by a rank test in the column order, every candidate solved from scratch."""
    H = np.asarray(H, np.int64) % 2
    seq = M.column_order(llr)
    S = []
    for j in seq:
        if _indep(H, S, int(j)):
            S.append(int(j))
    Tn = [int(j) for j in seq if int(j) not in S]
    q = M.quantise(w)
    b = (synd.astype(np.int64) + H @ hard.astype(np.int64)) % 2
    cands = [()] + [(t,) for t in Tn] + [(Tn[a], Tn[c]) for a in range(min(order, len(Tn))) for c in range(a + 1, min(order, len(Tn)))]
    best = None
    for t in cands:
        ct = np.zeros(H.shape[1], np.int64)
        ct[list(t)] = 1
        xs = _solve(H, (b + H @ ct) % 2, S)
        if xs is None:
            return None
        ct[S] = xs
        x = (hard.astype(np.int64) + ct) % 2
        cost = int(q[x == 1].sum())
        if best is None or cost < best[0]:
            best = (cost, x.astype(np.int8), (list(t) + [-1, -1])[:2])
    return best


def _indep(H, S, j):
    if not H[:, j].any():
        return False
    A = H[:, S + [j]].copy() % 2
    m = A.shape[0]
    r = 0
    for c in range(A.shape[1]):
        piv = next((i for i in range(r, m) if A[i, c]), None)
        if piv is None:
            if c == A.shape[1] - 1:
                return False
            continue
        A[[r, piv]] = A[[piv, r]]
        for i in range(m):
            if i != r and A[i, c]:
                A[i] ^= A[r]
        r += 1
    return True


@pytest.mark.parametrize("case", ["circ144_Z", "circ144_X", "circ72_Z", "circ72_X"])
def test_candidate0_is_the_reference_osd0(golden, case):
    tag, s = case.split("_")
    from qldpc_amd.data import load_circuit_matrices
    d = load_circuit_matrices(tag)
    f = golden(f"{tag}_decode")
    G = M.Graph(d[f"Hdec{s}_indptr"], d[f"Hdec{s}_indices"], int(d[f"Hdec{s}_shape"][1]))
    for ci, shot in enumerate(f[f"{s}_osd_cases"]):
        r = M.osd_cs(G, f[f"{s}_syndromes"][shot], f[f"{s}_llr"][shot], f[f"{s}_err"][shot], f[f"llrs_{s}"], 7, ordering=f[f"{s}_osd_ordering"][ci])
        assert not r["outside"]
        assert np.array_equal(r["osd0"], f[f"{s}_osd_solution"][ci])
        assert np.array_equal(G.parity(r["solution"]), f[f"{s}_syndromes"][shot] & 1)
        assert r["cost"] <= int(M.quantise(f[f"llrs_{s}"])[r["osd0"] == 1].sum())


def _small_cases(golden):
    f = golden("osdw")
    rng = np.random.default_rng(3)
    for case in f["cases"]:
        H = f[f"graph__{str(f[f'{case}__graph'])}"]
        yield H, f[f"{case}__syndrome"], f[f"{case}__llr"], f[f"{case}__hard"], rng.uniform(-1.0, 4.0, H.shape[1])
    for _ in range(25):
        m, n = int(rng.integers(2, 9)), int(rng.integers(3, 13))
        H = (rng.random((m, n)) < 0.3).astype(np.int8)
        H[:, rng.integers(0, n)] = 0
        e = (rng.random(n) < 0.3).astype(np.int64)
        synd = (H.astype(np.int64) @ e % 2).astype(np.int8)
        llr = np.round(rng.normal(0, 1.5, n))
        llr[rng.integers(0, n)] = rng.choice([np.inf, -np.inf, np.nan])
        w = np.where(rng.random(n) < 0.5, 1.0, rng.uniform(0.2, 2.0, n))
        yield H, synd, llr, (rng.random(n) < 0.3).astype(np.int8), w


@pytest.mark.parametrize("order", [0, 1, 3, 64])
def test_model_is_the_brute_force_enumeration(golden, order):
    inside = 0
    for H, synd, llr, hard, w in _small_cases(golden):
        r = M.osd_cs(_graph(H), synd, llr, hard, w, order)
        bf = brute_force(H, synd, llr, hard, w, order)
        if r["outside"]:
            assert bf is None
            continue
        inside += 1
        assert bf is not None
        assert r["cost"] == bf[0]
        assert np.array_equal(r["solution"], bf[1]) and list(r["flips"]) == bf[2]
        assert np.array_equal(_graph(H).parity(r["solution"]), synd & 1)
        if order <= 1:
            assert r["flips"][1] == -1
    assert inside > 20


def test_equal_weights_give_minimum_hamming_weight_over_the_candidates(golden):
    for H, synd, llr, hard, _ in _small_cases(golden):
        n = H.shape[1]
        r = M.osd_cs(_graph(H), synd, llr, hard, np.ones(n), 7)
        if r["outside"]:
            continue
        G = _graph(H)
        assert int(r["solution"].sum()) == int(r["osd0"].sum()) + int(r["deltas"].min()) // 1048576    # (q = 2^20 per one)
        assert np.array_equal(G.parity(r["solution"]), synd & 1)


def test_model_is_fast_on_the_circuit_matrices():
    import time
    from qldpc_amd.data import load_circuit_matrices
    d = load_circuit_matrices("circ144")
    G = M.Graph(d["HdecX_indptr"], d["HdecX_indices"], int(d["HdecX_shape"][1]))
    rng = np.random.default_rng(1)
    llr = rng.normal(3, 2, G.n)
    t0 = time.perf_counter()
    r = M.osd_cs(G, np.zeros(G.m, np.int8), llr, np.zeros(G.n, np.int8), np.abs(llr), 20)
    assert time.perf_counter() - t0 < 5.0
    assert not r["outside"] and r["flips"] == (-1, -1)                       # nothing lighter than the zero vector with positive weights


def test_weights_quantise_like_relay_bp():
    q = M.quantise(np.array([0.0, 1.0, -1.0, 0.5 / 1048576.0, 1e300, -1e300]))
    assert q.tolist() == [0, 1048576, -1048576, 1, 2 ** 40, -(2 ** 40)]


@pytest.mark.parametrize("kw", [dict(osd_order=65), dict(relay_params=dict(t0=3)), dict(osd_order=-1)])
def test_run_simulation_rejects_bad_arguments(L, kw, monkeypatch):
    from qldpc_amd.simulation import engine

    def no_gpu(*a, **k):
        raise AssertionError("GPU work started before the arguments were checked")
    monkeypatch.setattr(engine, "BBCodeCircuit", no_gpu)
    monkeypatch.setattr(L, "Graph", no_gpu)
    with pytest.raises(ValueError):
        engine.run_simulation(None, None, None, None, 0.005, num_trials=10, decoder="bp_osd_cs", devices=[0], **kw)


@pytest.mark.parametrize("bad", [dict(order=65), dict(order=-1), dict(weights_nan=True), dict(weights_len=True)])
def test_python_validation_before_any_graph(L, bad, monkeypatch):
    from qldpc_amd.decoding import osd_cs

    def no_graph(*a, **k):
        raise AssertionError("a graph was created before the arguments were checked")
    monkeypatch.setattr(L, "Graph", no_graph)
    H = np.array([[1, 1, 0], [0, 1, 1]], np.uint8)
    w = np.array([1.0, 2.0, 3.0])
    kw = dict(bad)
    if kw.pop("weights_nan", False):
        w[1] = np.nan
    if kw.pop("weights_len", False):
        w = w[:2]
    with pytest.raises(ValueError):
        osd_cs.OsdCsDecoder(H, w, **kw)
    with pytest.raises(ValueError):
        osd_cs.osd_cs_decode(H, np.zeros((1, 2), np.int8), np.ones((1, 3)), np.zeros((1, 3), np.int8), w, **kw)


def test_binding_follows_the_header(L):
    names = L.exports()
    for fn in ("qldpc_osdcs_batch", "qldpc_osdcs_batch_dev", "qldpc_circuit_plan_use_osd_cs"):
        assert fn in names
        getattr(L.lib(), fn)
    assert L.lib().qldpc_version() == 101
    assert L.lib().qldpc_osdcs_batch(None, 1, None, None, None, None, 7, None, None) == -1
    assert L.lib().qldpc_circuit_plan_use_osd_cs(None, 7) == -1
