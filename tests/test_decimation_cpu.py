"""BP with guided decimation without a GPU: the numpy model against a scalar loop over Python floats, the link to Relay-BP's model, the tie rule,
monotonicity, frozen decisions, running out of columns, argument checks and the binding."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decimation_model as DM  # noqa: E402
import relay_model as RM  # noqa: E402

NAMES = ("err", "llr", "conv", "iters", "rounds", "fixed")


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    return _lib


def _circ72(sector):
    from qldpc_amd.data import load_circuit_matrices
    d = load_circuit_matrices("circ72")
    return d[f"Hdec{sector}_indptr"], d[f"Hdec{sector}_indices"], int(d[f"Hdec{sector}_shape"][1])


def _bb72(golden, H="Hx", p="p080"):
    g = golden("bb72_minsum")
    return g[f"{H}_indptr"], g[f"{H}_indices"], int(g[f"{H}_shape"][1]), g[f"{H}_{p}_syndromes"], g[f"{H}_{p}_prior"]


def _clip_nan(x, clip):
    if x != x:
        return 0.0
    return clip if x > clip else (-clip if x < -clip else x)


def scalar_decode(indptr, indices, n, syndrome, prior, alpha, clip, T, max_rounds, per_round, fix):
    """The steps of qldpc_decim_decode_batch in include/qldpc_hip.h for one shot, on Python floats and lists."""
    m = len(indptr) - 1
    rows = [[int(j) for j in indices[indptr[i]:indptr[i + 1]]] for i in range(m)]
    col_edges = [[] for _ in range(n)]
    for i, row in enumerate(rows):                                 # ascending check order per column
        for k, j in enumerate(row):
            col_edges[j].append((i, k))
    syn = [bool(int(s) & 1) for s in syndrome]
    V = [float(p) for p in prior]
    bias = list(V)
    fixed = [False] * n
    iters = rounds = 0
    conv = False
    for r in range(max_rounds + 1):
        R = [[0.0] * len(row) for row in rows]
        itc = T
        for it in range(T + 1):
            unsat = False
            Rn = []
            for i, row in enumerate(rows):
                par = sp = syn[i]
                min1 = min2 = math.inf
                arg = -1
                negs = []
                for k, j in enumerate(row):
                    v = V[j]
                    par ^= v < 0.0
                    x = v if it == 0 else _clip_nan(v - R[i][k], clip)
                    neg = not x >= 0.0
                    sp ^= neg
                    negs.append(neg)
                    a = abs(x)
                    if a < min1:
                        min2, min1, arg = min1, a, k
                    elif a < min2:
                        min2 = a
                unsat |= par
                m1a, m2a = alpha * min1, alpha * min2
                Rn.append([(-1.0 if sp != negs[k] else 1.0) * (m2a if k == arg else m1a) for k in range(len(row))])
            if it >= 1 and not unsat:
                conv, itc = True, it
                break
            if it == T:
                break
            R = Rn
            for j in range(n):
                s = 0.0
                for i, k in col_edges[j]:
                    s += R[i][k]
                V[j] = s + bias[j]
        iters += itc
        rounds = r + 1
        if conv or r == max_rounds or all(fixed):
            break
        free = [j for j in range(n) if not fixed[j]]
        free.sort(key=lambda j: (-(0.0 if V[j] != V[j] else abs(V[j])), j))
        for j in free[:per_round]:
            bias[j] = -fix if V[j] < 0.0 else fix
            V[j] = bias[j]
            fixed[j] = True
    return [1 if v < 0.0 else 0 for v in V], V, int(conv), iters, rounds, sum(fixed)


def _assert_scalar(ip, ix, n, synd, prior, **kw):
    got = DM.decim_decode(ip, ix, n, synd, prior, **kw)
    for b in range(synd.shape[0]):
        ref = scalar_decode(ip, ix, n, synd[b], prior, kw["alpha"], kw["clip_llr"], kw["t_round"], kw["max_rounds"], kw["per_round"], kw["fix_llr"])
        assert np.array_equal(got[0][b], np.array(ref[0], np.int8)), f"shot {b}: err"
        assert np.array_equal(got[1][b], np.array(ref[1]), equal_nan=True), f"shot {b}: llr"
        assert (int(got[2][b]), int(got[3][b]), int(got[4][b]), int(got[5][b])) == ref[2:], f"shot {b}: conv / iters / rounds / fixed"
    return got


def test_model_equals_the_scalar_loop_steane(golden):
    g = golden("steane_minsum")
    for prior in (g["prior"], g["prior2"]):
        for kw in (dict(t_round=1, max_rounds=3, per_round=2), dict(t_round=2, max_rounds=7, per_round=1), dict(t_round=5, max_rounds=0, per_round=64)):
            _assert_scalar(g["indptr"], g["indices"], int(g["n"]), g["syndromes"], prior, alpha=0.75, clip_llr=20.0, fix_llr=35.0, **kw)


@pytest.mark.parametrize("sector", ["Z", "X"])
def test_model_equals_the_scalar_loop_circ72(golden, sector):
    """sector X has degree-1 checks: their +-inf messages make +-inf marginals, which the key rule puts first"""
    ip, ix, n = _circ72(sector)
    g = golden("circ72_decode")
    synd, prior = g[f"{sector}_syndromes"], g[f"llrs_{sector}"]
    got = _assert_scalar(ip, ix, n, synd, prior, alpha=0.875, clip_llr=20.0, t_round=3, max_rounds=4, per_round=16, fix_llr=50.0)
    assert got[4].max() > 1 and got[5].max() >= 16                 # decimation ran
    if sector == "X":
        assert (np.diff(ip) == 1).any() and np.isinf(got[1]).any()


def test_key_rule_for_nan_and_inf():
    v = np.array([1.0, np.nan, -np.inf, 3.0, np.inf, -3.0, 0.0, np.nan])
    fixed = np.zeros(8, bool)
    assert DM.select(v, fixed, 8).tolist() == [2, 4, 3, 5, 0, 1, 6, 7]   # inf first (lowest column first), the NaNs tie with 0.0
    fixed[[2, 3]] = True
    assert DM.select(v, fixed, 3).tolist() == [4, 5, 0]
    assert DM.select(v, fixed, 64).size == 6


@pytest.mark.parametrize("case", ["steane", "circ72_Z", "circ72_X", "bb72"])
def test_no_rounds_is_relay_without_memory(golden, case):
    if case == "steane":
        g = golden("steane_minsum")
        ip, ix, n, synd, prior = g["indptr"], g["indices"], int(g["n"]), g["syndromes"], g["prior"]
    elif case == "bb72":
        ip, ix, n, synd, prior = _bb72(golden)
        synd = synd[:16]
    else:
        ip, ix, n = _circ72(case[-1])
        g = golden("circ72_decode")
        synd, prior = g[f"{case[-1]}_syndromes"], g[f"llrs_{case[-1]}"]
    err, llr, conv, iters, rounds, fixed = DM.decim_decode(ip, ix, n, synd, prior, alpha=0.8125, clip_llr=20.0, t_round=9, max_rounds=0, per_round=8,
                                                           fix_llr=50.0)
    rerr, rconv, rlegs, riters, _ = RM.relay_decode(ip, ix, n, synd, prior, seed=1, alpha=0.8125, clip_llr=20.0, gamma0=0.0, t0=9, max_legs=0, stop_after=1)
    assert err.tobytes() == rerr.tobytes() and conv.tobytes() == rconv.tobytes() and iters.tobytes() == riters.tobytes()
    assert np.array_equal(rounds, rlegs) and not fixed.any()
    assert np.array_equal(err, (llr < 0.0).astype(np.int8))


def test_ties_go_to_the_lowest_column(golden):
    """uniform prior on the [[72,12,6]] code-capacity matrix: exact ties in |V| occur, also across the cut of the first decimation"""
    ip, ix, n, synd, prior = _bb72(golden)
    assert np.unique(prior).size == 1
    trace = []
    out = DM.decim_decode(ip, ix, n, synd[:16], prior, alpha=1.0, clip_llr=20.0, t_round=2, max_rounds=2, per_round=8, fix_llr=50.0, trace=trace)
    first = [t for t in trace if t[1] == 0]
    assert len(first) >= 4 and (out[4] > 1).sum() == len(first)
    cut_ties = 0
    for b, r, cols, before in first:
        a = np.abs(before)
        assert cols.size == 8
        assert all((a[cols[i]], -cols[i]) >= (a[cols[i + 1]], -cols[i + 1]) for i in range(7))        # the stated order
        rest = np.setdiff1d(np.arange(n), cols)
        assert a[rest].max() <= a[cols].min()
        tied_out = rest[a[rest] == a[cols].min()]                  # left out although as reliable as the last one taken ...
        if tied_out.size:
            cut_ties += 1
            assert tied_out.min() > cols[a[cols] == a[cols].min()].max()                               # ... then they are the higher columns
    assert cut_ties >= 1


def test_converged_shots_do_not_change_with_more_rounds(golden):
    for ip, ix, n, synd, prior in (_bb72(golden), _bb72(golden, "Hz", "p030")):
        kw = dict(alpha=1.0, clip_llr=20.0, t_round=4, per_round=4, fix_llr=50.0)
        base = DM.decim_decode(ip, ix, n, synd[:32], prior, max_rounds=0, **kw)
        more = DM.decim_decode(ip, ix, n, synd[:32], prior, max_rounds=8, **kw)
        ok = base[2] == 1
        assert ok.any() and not ok.all()
        assert np.array_equal(base[0][ok], more[0][ok]) and np.array_equal(base[3][ok], more[3][ok])
        assert (more[4][ok] == 1).all() and (more[5][ok] == 0).all()
        assert more[2].sum() >= base[2].sum()


def test_frozen_decisions_stay(golden):
    """no degree-1 checks and fix_llr > cdeg * alpha * clip_llr: |s_j| <= cdeg * alpha * clip_llr can never outweigh the frozen prior"""
    ip, ix, n, synd, prior = _bb72(golden)
    cdeg = int(np.bincount(ix, minlength=n).max())
    assert np.diff(ip).min() > 1
    alpha, clip = 1.0, 20.0
    fix = cdeg * alpha * clip + 1.0
    trace = []
    out = DM.decim_decode(ip, ix, n, synd[:16], prior, alpha=alpha, clip_llr=clip, t_round=3, max_rounds=6, per_round=5, fix_llr=fix, trace=trace)
    assert len(trace) > 16
    frozen = {}                                                    # shot -> {column: sign it was frozen with}
    for b, r, cols, before in trace:
        for j, neg in frozen.get(b, {}).items():
            assert (before[j] < 0.0) == neg, f"shot {b}: column {j} changed its decision by round {r}"
        frozen.setdefault(b, {}).update({int(j): bool(before[j] < 0.0) for j in cols})
    for b, d in frozen.items():
        for j, neg in d.items():
            assert bool(out[0][b, j]) == neg


def test_running_out_of_columns(golden):
    """Steane, per_round = 4: two decimations freeze all 7 columns; a syndrome the frozen pattern does not satisfy ends at round 3, not at 1 + max_rounds"""
    g = golden("steane_minsum")
    ip, ix, n = g["indptr"], g["indices"], int(g["n"])
    prior = np.full(n, 100.0)                                      # far above clip_llr: one iteration per round cannot flip a column
    synd = np.array([[1, 0, 0], [0, 0, 0]], np.int8)
    err, llr, conv, iters, rounds, fixed = DM.decim_decode(ip, ix, n, synd, prior, alpha=1.0, clip_llr=20.0, t_round=1, max_rounds=3, per_round=4,
                                                           fix_llr=1000.0)
    assert (int(fixed[0]), int(conv[0]), int(rounds[0]), int(iters[0])) == (7, 0, 3, 3)
    assert not err[0].any()                                        # H 0 = 0 is not the syndrome
    assert (int(fixed[1]), int(conv[1]), int(rounds[1]), int(iters[1])) == (0, 1, 1, 1)
    _assert_scalar(ip, ix, n, synd, prior, alpha=1.0, clip_llr=20.0, t_round=1, max_rounds=3, per_round=4, fix_llr=1000.0)


@pytest.mark.parametrize("bad", [
    dict(prior_nan=True), dict(alpha=0.0), dict(alpha=float("nan")), dict(clip_llr=-1.0), dict(fix_llr=0.0), dict(fix_llr=float("inf")), dict(t_round=0),
    dict(max_rounds=-1), dict(max_rounds=2 ** 20), dict(per_round=0), dict(per_round=65), dict(t_round=2.5), dict(bogus=1)])
def test_python_validation_before_any_graph(L, bad, monkeypatch):
    from qldpc_amd.decoding import decimation

    def no_graph(*a, **k):
        raise AssertionError("a graph was created before the arguments were checked")
    monkeypatch.setattr(L, "Graph", no_graph)
    H = np.array([[1, 1, 0], [0, 1, 1]], np.uint8)
    prior = np.array([1.0, 2.0, 3.0])
    kw = dict(alpha=1.0, t_round=4, max_rounds=2, per_round=1, fix_llr=30.0, clip_llr=20.0)
    kw.update(bad)
    if kw.pop("prior_nan", False):
        prior[1] = np.nan
    with pytest.raises(ValueError):
        decimation.DecimationDecoder(H, prior, **kw)
    with pytest.raises(ValueError):
        decimation.decimation_decode(H, np.zeros((1, 2), np.int8), prior, **kw)


def test_null_graph_is_invalid_and_binding_follows_the_header(L):
    names = L.exports()
    for fn in ("qldpc_decim_decode_batch", "qldpc_decim_decode_batch_dev", "qldpc_circuit_plan_use_decimation"):
        assert fn in names
        getattr(L.lib(), fn)
    assert L.lib().qldpc_version() == 101
    argtypes = L.signatures()["qldpc_decim_decode_batch_dev"][1]
    assert argtypes[2] is C.c_void_p and argtypes[-2] is C.c_void_p and len(argtypes) == 17
    assert len(L.signatures()["qldpc_decim_decode_batch"][1]) == 16
    synd, prior = np.zeros(3, np.int8), np.ones(3)
    e, c, i = np.zeros(3, np.int8), np.zeros(1, np.uint8), np.zeros(1, np.int32)
    rc = L.lib().qldpc_decim_decode_batch(None, 1, L.ptr(synd, C.c_int8), L.ptr(prior, C.c_double), 1.0, 20.0, 4, 2, 1, 50.0, L.ptr(e, C.c_int8), None,
                                          L.ptr(c, C.c_uint8), L.ptr(i, C.c_int32), None, None)
    assert rc == -1 and b"graph is NULL" in L.lib().qldpc_last_error()
    assert L.lib().qldpc_decim_decode_batch_dev(None, 1, None, None, 1.0, 20.0, 4, 2, 1, 50.0, None, None, None, None, None, None, None) == -1
    assert L.lib().qldpc_circuit_plan_use_decimation(None, 1.0, 4, 2, 1, 50.0) == -1
    assert "Relay-BP: legs; decimation: rounds" in open(L.HEADER_PATH).read()


DECIM = dict(alpha=1.0, t_round=4, max_rounds=2, per_round=8, fix_llr=50.0)


@pytest.mark.parametrize("kw", [
    dict(decoder="relay_bp"), dict(window=(4, 2)), dict(schedule="layered"), dict(osd_order=2), dict(alpha_mode="dynamical"), dict(alpha_mode="alvarado"),
    dict(alpha_mode="alvarado-autoregressive"), dict(alvarado_alpha=0.8), dict(use_dynamic_alpha=False), dict(scopt=True),
    dict(decimation=dict(DECIM, t_round=0)), dict(decimation=dict(DECIM, per_round=65)), dict(decimation=dict(DECIM, clip_llr=5.0)),
    dict(decimation=dict(DECIM, bogus=1)), dict(decimation=[4, 2])])
def test_run_simulation_rejects_bad_combinations(L, kw, monkeypatch):
    from qldpc_amd.simulation import engine

    def no_gpu(*a, **k):
        raise AssertionError("GPU work started before the arguments were checked")
    monkeypatch.setattr(engine, "BBCodeCircuit", no_gpu)
    monkeypatch.setattr(L, "Graph", no_gpu)
    monkeypatch.setattr(L, "device_count", no_gpu)
    args = dict(decimation=DECIM)
    args.update(kw)
    with pytest.raises(ValueError):
        engine.run_simulation(None, None, None, None, 0.005, num_trials=10, devices=[0], **args)
