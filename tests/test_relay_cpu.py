"""Relay-BP without a GPU: the numpy model against the min-sum checker, the memory-strength stream, argument checks and the binding."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import relay_model as RM  # noqa: E402


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    return _lib


def _circ72(sector="Z"):
    from qldpc_amd.data import load_circuit_matrices
    d = load_circuit_matrices("circ72")
    return d[f"Hdec{sector}_indptr"], d[f"Hdec{sector}_indices"], int(d[f"Hdec{sector}_shape"][1])


@pytest.mark.parametrize("case", ["bb72_x_p030", "bb72_z_p080", "circ72_z", "circ72_x"])
def test_model_without_memory_is_minsum(case, golden, oracle):
    """gamma0 = 0, no relay legs, t0 = max_iter: the model is the constant-alpha min-sum decoder bit for bit (err, conv, iterations)."""
    if case.startswith("bb72"):
        g = golden("bb72_minsum")
        H, p = case.split("_")[1].capitalize(), case.split("_")[2]
        ip, ix, n = g[f"H{H.lower()}_indptr"], g[f"H{H.lower()}_indices"], int(g[f"H{H.lower()}_shape"][1])
        synd, prior, max_iter = g[f"H{H.lower()}_{p}_syndromes"], g[f"H{H.lower()}_{p}_prior"], 30
    else:
        s = case[-1].upper()
        ip, ix, n = _circ72(s)
        g = golden("circ72_decode")
        synd, prior, max_iter = g[f"{s}_syndromes"], g[f"llrs_{s}"], int(g["max_iter"])
    alpha = 0.8125
    err, conv, legs, iters, sols = RM.relay_decode(ip, ix, n, synd, prior, seed=7, alpha=alpha, gamma0=0.0, t0=max_iter, max_legs=0, stop_after=1)
    rerr, rconv, _, riters = oracle.minsum_decode_batch(ip, ix, n, synd, prior, max_iter=max_iter, alpha=alpha, alpha_mode="alvarado")
    assert np.array_equal(err, rerr)
    assert np.array_equal(conv, rconv)
    assert np.array_equal(iters, riters + 1)
    assert np.array_equal(legs, np.ones_like(legs)) and np.array_equal(sols, conv.astype(np.int32))


def test_gamma_stream_is_the_library_philox(L):
    seed, tag, n = 0x123456789ABCDEF, 5, 23
    shots = [0, 1, 2 ** 33 + 7]
    for leg in (1, 2, 299):
        w = RM.gamma_draws(shots, n, leg, seed, tag)
        for bi, shot in enumerate(shots):
            for j in range(n):
                ctr = (C.c_uint32 * 4)(shot & 0xFFFFFFFF, shot >> 32, j >> 2, 0x52000000 | (tag << 20) | leg)
                key = (C.c_uint32 * 2)(seed & 0xFFFFFFFF, seed >> 32)
                out = (C.c_uint32 * 4)()
                L.lib().qldpc_philox4x32_10(ctr, key, out)
                assert w[bi, j] == out[j & 3] >> 16
    g = RM.gammas([3], 8, 1, seed, tag, -0.24, 0.66)
    w = RM.gamma_draws([3], 8, 1, seed, tag).astype(np.float64)
    assert np.array_equal(g, -0.24 + (0.66 - -0.24) * (w / 65536.0))
    assert (g >= -0.24).all() and (g < 0.66).all()


def test_model_relay_legs_only_add_solutions(golden):
    """The model with relay legs: a shot the first leg solves keeps its answer with stop_after = 1; every solution reproduces the syndrome."""
    ip, ix, n = _circ72("Z")
    g = golden("circ72_decode")
    synd, prior = g["Z_syndromes"], g["llrs_Z"]
    base = RM.relay_decode(ip, ix, n, synd, prior, seed=3, gamma0=0.0, t0=20, max_legs=0, stop_after=1)
    err, conv, legs, iters, sols = RM.relay_decode(ip, ix, n, synd, prior, seed=3, gamma0=0.0, t0=20, tr=10, max_legs=6, stop_after=1)
    solved = base[1] == 1
    assert np.array_equal(err[solved], base[0][solved]) and conv[solved].all()
    assert (legs >= 1).all() and (legs <= 7).all() and (sols <= legs).all()
    H = np.zeros((len(ip) - 1, n), np.int64)
    for i in range(len(ip) - 1):
        H[i, ix[ip[i]:ip[i + 1]]] = 1
    for b in np.flatnonzero(conv):
        assert np.array_equal((H @ err[b].astype(np.int64)) % 2, synd[b] & 1)


def test_weights_are_rounded_fixed_point():
    q = RM.weights(np.array([0.0, 1.0, -1.0, 0.5 / 1048576.0, 1e300, -1e300]))
    assert q.tolist() == [0, 1048576, -1048576, 1, 2 ** 40, -(2 ** 40)]


@pytest.mark.parametrize("bad", [
    dict(prior_nan=True), dict(gamma_min=0.5, gamma_max=0.1), dict(t0=0), dict(stop_after=0), dict(tag=16), dict(max_legs=2 ** 20),
    dict(tr=0), dict(alpha=0.0), dict(bogus=1)])
def test_python_validation_before_any_graph(L, bad, monkeypatch):
    from qldpc_amd.decoding import relay

    def no_graph(*a, **k):
        raise AssertionError("a graph was created before the arguments were checked")
    monkeypatch.setattr(L, "Graph", no_graph)
    H = np.array([[1, 1, 0], [0, 1, 1]], np.uint8)
    prior = np.array([1.0, 2.0, 3.0])
    kw = dict(bad)
    if kw.pop("prior_nan", False):
        prior[1] = np.nan
    with pytest.raises(ValueError):
        relay.RelayBPDecoder(H, prior, **kw)
    with pytest.raises(ValueError):
        relay.relay_bp_decode(H, np.zeros((1, 2), np.int8), prior, **kw)


def test_no_cpu_fallback(L):
    if L.device_count() > 0:
        pytest.skip("GPU present")
    from qldpc_amd.decoding.relay import relay_bp_decode
    with pytest.raises(L.QldpcError, match="no CPU fallback"):
        relay_bp_decode(np.eye(3), np.zeros((1, 3), np.int8), [1.0, 1.0, 1.0])


def test_null_graph_is_invalid(L):
    synd, prior = np.zeros(3, np.int8), np.ones(3)
    out8, outu8, o1, o2, o3 = np.zeros(3, np.int8), np.zeros(1, np.uint8), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32)
    rc = L.lib().qldpc_relay_decode_batch(None, 1, L.ptr(synd, C.c_int8), L.ptr(prior, C.c_double), 1.0, 20.0, 0.125, -0.24, 0.66, 80, 60, 300, 5,
                                          C.c_uint64(0), 0, 0, L.ptr(out8, C.c_int8), L.ptr(outu8, C.c_uint8), L.ptr(o1, C.c_int32),
                                          L.ptr(o2, C.c_int32), L.ptr(o3, C.c_int32))
    assert rc == -1 and b"graph is NULL" in L.lib().qldpc_last_error()
    rc = L.lib().qldpc_relay_decode_batch_dev(None, 1, None, None, 1.0, 20.0, 0.125, -0.24, 0.66, 80, 60, 300, 5, C.c_uint64(0), 0, 0,
                                              None, None, None, None, None, None)
    assert rc == -1
    assert L.lib().qldpc_circuit_plan_use_relay(None, 1.0, 0.125, -0.24, 0.66, 80, 60, 300, 5) == -1


def test_binding_follows_the_header(L):
    names = L.exports()
    for fn in ("qldpc_relay_decode_batch", "qldpc_relay_decode_batch_dev", "qldpc_circuit_plan_use_relay"):
        assert fn in names
        getattr(L.lib(), fn)
    assert L.lib().qldpc_version() == 101
    assert L.TALLY["legs_z"] == 14 and L.TALLY["legs_x"] == 15
    hdr = open(L.HEADER_PATH).read()
    assert "#define QLDPC_TALLY_LEGS_Z 14" in hdr and "#define QLDPC_TALLY_LEGS_X 15" in hdr
    argtypes = L.signatures()["qldpc_relay_decode_batch_dev"][1]
    assert argtypes[2] is C.c_void_p and argtypes[-2] is C.c_void_p         # d_syndromes, d_solutions: addresses


@pytest.mark.parametrize("kw", [dict(osd_order=2), dict(alpha_mode="alvarado"), dict(alvarado_alpha=0.8), dict(scopt=True),
                                dict(relay_params=dict(t0=0)), dict(relay_params=dict(clip_llr=5.0))])
def test_run_simulation_rejects_bad_combinations(L, kw, monkeypatch):
    from qldpc_amd.simulation import engine

    def no_gpu(*a, **k):
        raise AssertionError("GPU work started before the arguments were checked")
    monkeypatch.setattr(engine, "BBCodeCircuit", no_gpu)
    monkeypatch.setattr(L, "Graph", no_gpu)
    with pytest.raises(ValueError):
        engine.run_simulation(None, None, None, None, 0.005, num_trials=10, decoder="relay_bp", devices=[0], **kw)


def test_run_simulation_rejects_unknown_decoder(L, monkeypatch):
    from qldpc_amd.simulation import engine
    monkeypatch.setattr(engine, "BBCodeCircuit", lambda *a, **k: (_ for _ in ()).throw(AssertionError("GPU work started")))
    with pytest.raises(ValueError, match="decoder"):
        engine.run_simulation(None, None, None, None, 0.005, num_trials=10, decoder="bogus", devices=[0])
    with pytest.raises(ValueError):
        engine.run_simulation(None, None, None, None, 0.005, num_trials=10, relay_params=dict(t0=3), devices=[0])
