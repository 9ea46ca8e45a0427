"""Sliding-window decoding without a GPU: the layer structure of the packaged matrices, the numpy model (tests/window_model.py) against the
oracle's whole-graph min-sum + OSD-0 and against direct decodes of its own windows, the running-syndrome bookkeeping, argument checks of the
Python layer and run_simulation, and the binding."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import window_model as WM  # noqa: E402

# rows per layer, columns per interior layer of the packaged matrix sets
SETS = {"circ72": (36, 360), "circ144": (72, 720), "circ288": (144, 1440)}


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    return _lib


def _sector(tag, s):
    from qldpc_amd.data import load_circuit_matrices
    d = load_circuit_matrices(tag)
    return d[f"Hdec{s}_indptr"], d[f"Hdec{s}_indices"], int(d[f"Hdec{s}_shape"][1]), int(d["num_cycles"])


@pytest.mark.parametrize("tag", sorted(SETS))
def test_layer_structure_of_the_packaged_matrices(L, tag):
    from qldpc_amd.decoding.window import column_layers
    mc, per_layer = SETS[tag]
    for s in "ZX":
        ip, ix, n, cycles = _sector(tag, s)
        m = len(ip) - 1
        assert m == mc * (cycles + 2)
        tau, span = column_layers((ip, ix, n), mc)
        assert set(np.unique(span)) <= {0, 1} and span.max() == 1
        deg = np.bincount(ix, minlength=n)
        assert (deg == 0).sum() == 1 and tau[deg == 0][0] == 0
        counts = np.bincount(tau[deg > 0], minlength=cycles + 2)
        assert (counts[1:cycles] == per_layer).all(), counts                # periodic in the first layer
        mt, ms = WM.column_layers(WM.Matrix(ip, ix, n), mc)
        assert np.array_equal(mt, tau) and np.array_equal(ms, span)


def _golden_sets(golden):
    f = golden("circ72_decode")
    out = []
    for s in "ZX":
        ip, ix, n, cycles = _sector("circ72", s)
        out.append((s, ip, ix, n, cycles, f[f"llrs_{s}"], f[f"{s}_syndromes"], int(f["max_iter"])))
    return out


def test_one_window_is_the_whole_graph_decode(L, golden, oracle):
    for s, ip, ix, n, cycles, prior, synd, max_iter in _golden_sets(golden):
        for W, C in ((cycles + 2, cycles + 2), (cycles + 5, 3)):
            model = WM.WindowModel(ip, ix, n, prior, 36, W, C)
            assert len(model.stages) == 1 and model.distinct_graphs() == 1
            err, conv, iters, osd, unsat = model.decode(oracle, synd, max_iter=max_iter)
            det, cv, llr, it = oracle.minsum_decode_batch(ip, ix, n, synd, prior, max_iter=max_iter)
            for b in np.flatnonzero(cv == 0):
                det[b] = oracle.osd0(ip, ix, n, synd[b], llr[b], det[b])
            assert np.array_equal(err, det)
            assert np.array_equal(conv, cv.astype(np.int32)) and np.array_equal(osd, 1 - cv.astype(np.int32)) and np.array_equal(iters, it + 1)
            assert not unsat.any()


@pytest.mark.parametrize("WC", [(4, 2), (3, 1)])
def test_windows_commit_direct_decodes_and_keep_the_books(L, golden, oracle, WC):
    W, C = WC
    for s, ip, ix, n, cycles, prior, synd, max_iter in _golden_sets(golden):
        model = WM.WindowModel(ip, ix, n, prior, 36, W, C)
        layers = cycles + 2
        assert [st["a"] for st in model.stages] == list(range(0, layers - W + C, C))[:len(model.stages)] and model.stages[-1]["end"] == layers
        interior = [st for st in model.stages if st["a"] >= 1 and st["end"] <= layers - 2]   # clear of the first layer and of the two closing ones
        assert model.distinct_graphs() == len(model.stages) - max(len(interior) - 1, 0)     # they are ONE graph; every other window is its own
        if WC == (3, 1):
            assert len(interior) == 3
        trace = []
        err, conv, iters, osd, unsat = model.decode(oracle, synd, max_iter=max_iter, trace=trace)
        M = model.M
        assert np.array_equal(model.r_final, (synd & 1) ^ M.parity(err))    # r_final = s ^ H err
        assert np.array_equal(unsat, model.r_final.any(axis=1).astype(np.uint8))
        assert np.array_equal(conv + osd, np.full(len(synd), len(model.stages), np.int32))
        done = np.zeros(n, bool)
        r = synd & 1
        for st, ws, det, cv in trace:
            # the window's syndrome is the running syndrome of what was committed before it
            assert np.array_equal(ws, r[:, st["r0"]:st["r1"]])
            H = np.zeros((st["r1"] - st["r0"], st["cols"].size), np.int8)
            rows = np.repeat(np.arange(len(st["indptr"]) - 1), np.diff(st["indptr"]))
            H[rows, st["indices"]] = 1
            full = np.zeros((M.m, n), np.int8)
            full[M.rows, M.indices] = 1
            assert np.array_equal(H, full[st["r0"]:st["r1"]][:, st["cols"]])  # the window graph is the block of H
            direct, dcv, dllr, _ = oracle.minsum_decode_batch(st["indptr"], st["indices"], st["cols"].size, ws, st["prior"], max_iter=max_iter)
            for b in np.flatnonzero(dcv == 0):
                direct[b] = oracle.osd0(st["indptr"], st["indices"], st["cols"].size, ws[b], dllr[b], direct[b])
            cc = st["cols"][st["committed"]]
            assert np.array_equal(err[:, cc], direct[:, st["committed"]])
            assert not done[cc].any()
            done[cc] = True
            e = np.zeros_like(err)
            e[:, cc] = err[:, cc]
            r = r ^ M.parity(e)
        assert done.all()                                                   # every column is committed exactly once


def test_span_two_column_is_rejected(L):
    from qldpc_amd.decoding.window import SlidingWindowDecoder, column_layers
    H = np.zeros((6, 5), np.int8)
    H[[0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 0]] = 1
    H[2, 1] = 1                                                              # column 1: layers 0 and 1 (fine); column 0: rows 0 and 5 = layers 0 and 2
    tau, span = column_layers(H, 2)
    assert span.tolist() == [2, 1, 0, 0, 0]
    ip, ix, shape = L.canonical_csr(H)
    with pytest.raises(ValueError, match="layers"):
        WM.WindowModel(ip, ix, 5, np.ones(5), 2, 2, 1)

    def no_graph(*a, **k):
        raise AssertionError("a graph was created before the arguments were checked")
    import unittest.mock as mock
    with mock.patch.object(L, "Graph", no_graph):
        with pytest.raises(ValueError, match="layers"):
            SlidingWindowDecoder(H, np.ones(5), 2, 2, 1)


@pytest.mark.parametrize("bad", [dict(layer_rows=5), dict(window=0), dict(commit=0), dict(commit=4), dict(prior_inf=True), dict(prior_len=True),
                                 dict(alpha_mode="bogus")])
def test_python_validation_before_any_graph(L, bad, monkeypatch):
    from qldpc_amd.decoding.window import SlidingWindowDecoder

    def no_graph(*a, **k):
        raise AssertionError("a graph was created before the arguments were checked")
    monkeypatch.setattr(L, "Graph", no_graph)
    H = np.eye(6, dtype=np.int8)
    kw = dict(layer_rows=2, window=3, commit=1)
    kw.update(bad)
    prior = np.ones(6)
    if kw.pop("prior_inf", False):
        prior[2] = np.inf
    if kw.pop("prior_len", False):
        prior = prior[:5]
    with pytest.raises(ValueError):
        SlidingWindowDecoder(H, prior, **kw)


@pytest.mark.parametrize("kw", [dict(decoder="relay_bp"), dict(decoder="bp_osd_cs", osd_order=7), dict(osd_order=2), dict(window=(2, 3)),
                                dict(window=(0, 0)), dict(window=4), dict(window=(4, 2, 1))])
def test_run_simulation_rejects_bad_combinations(L, kw, monkeypatch):
    from qldpc_amd.simulation import engine

    def no_gpu(*a, **k):
        raise AssertionError("GPU work started before the arguments were checked")
    monkeypatch.setattr(engine, "BBCodeCircuit", no_gpu)
    monkeypatch.setattr(L, "Graph", no_gpu)
    kw = dict(dict(window=(4, 2)), **kw)
    with pytest.raises(ValueError):
        engine.run_simulation(None, None, None, None, 0.005, num_trials=10, devices=[0], **kw)


def test_binding_follows_the_header(L):
    names = L.exports()
    for fn in ("qldpc_window_decoder_create", "qldpc_window_decoder_destroy", "qldpc_window_decoder_info", "qldpc_window_decode_batch",
               "qldpc_window_decode_batch_dev", "qldpc_circuit_plan_use_window"):
        assert fn in names
        getattr(L.lib(), fn)
    import ctypes as C
    argtypes = L.signatures()["qldpc_window_decode_batch_dev"][1]
    assert argtypes[2] is C.c_void_p and argtypes[-2] is C.c_void_p          # d_syndromes, d_unsat: addresses
    assert L.lib().qldpc_circuit_plan_use_window(None, 4, 2) == -1
    assert L.lib().qldpc_window_decoder_info(None, None, None, None, None, None) == -1
    out = C.c_void_p()
    prior = np.ones(3)
    assert L.lib().qldpc_window_decoder_create(None, 1, 1, 1, L.ptr(prior, C.c_double), 10, 1, 1.0, None, 0, 20.0, 0, C.byref(out)) == -1
    assert not out.value
