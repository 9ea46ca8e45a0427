"""OSD-CS on the MI355X: C-level checks, bit-exactness against tests/osd_cs_model.py, the link to OSD-0, the device entry point, batch splits,
concurrent streams, the circuit plan switch and run_simulation."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import osd_cs_model as M  # noqa: E402
from test_relay_gpu import _bb_params, circuit_setup, sampled  # noqa: E402

pytestmark = pytest.mark.gpu

ORDERS = (0, 7, 20)


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


def _model_graph(g):
    return M.Graph(g.indptr, g.indices, g.n)


def _cs_call(L, g, synd, llr, hard, w, order):
    synd = np.ascontiguousarray(synd, np.int8).reshape(-1, g.m)
    B = synd.shape[0]
    llr = np.ascontiguousarray(llr, np.float64).reshape(B, g.n)
    hard = np.ascontiguousarray(hard, np.int8).reshape(B, g.n)
    w = np.ascontiguousarray(w, np.float64)
    sol, fl = np.zeros((max(B, 1), g.n), np.int8), np.zeros((max(B, 1), 2), np.int32)
    return L.lib().qldpc_osdcs_batch(g.handle, B, L.ptr(synd, C.c_int8), L.ptr(llr, C.c_double), L.ptr(hard, C.c_int8), L.ptr(w, C.c_double),
                                     int(order), L.ptr(sol, C.c_int8), L.ptr(fl, C.c_int32))


def _cost(x, w):
    q = M.quantise(w)
    return (x.astype(np.int64) * q[None, :]).sum(axis=1)


def _check(L, g, synd, llr, hard, w, order, G=None):
    """library == model on every shot (OSD-0's answer where s + H hard is outside the column space) -> (solution, flips, outside)"""
    sol, fl = L.osdcs_batch(g, synd, llr, hard, w, order)
    msol, mfl, outside, _ = M.osd_cs_batch(G or _model_graph(g), synd, llr, hard, w, order)
    o0 = L.osd0_batch(g, synd, llr, hard)
    for i in range(len(synd)):
        if outside[i]:
            assert np.array_equal(sol[i], o0[i]) and tuple(fl[i]) == (-1, -1), f"shot {i}: outside the column space"
        else:
            assert np.array_equal(sol[i], msol[i]), f"order {order} shot {i}: solution differs from the model"
            assert np.array_equal(fl[i], mfl[i]), f"order {order} shot {i}: flips {fl[i]} vs model {mfl[i]}"
    return sol, fl, outside, o0


def _circ144(L, s):
    from qldpc_amd.data import load_circuit_matrices
    d = load_circuit_matrices("circ144")
    g = L.Graph(d[f"Hdec{s}_indptr"], d[f"Hdec{s}_indices"], int(d[f"Hdec{s}_shape"][1]))
    return g


def test_c_level_validation(L):
    c, compiled, Mx, graphs, priors, masks, plan = circuit_setup(L, "circ72")
    g, w = graphs[0], priors[0]
    synd, llr, hard = np.zeros((2, g.m), np.int8), np.ones((2, g.n)), np.zeros((2, g.n), np.int8)
    assert _cs_call(L, g, synd, llr, hard, w, 65) == -1
    assert _cs_call(L, g, synd, llr, hard, w, -1) == -1
    bad = w.copy()
    bad[3] = np.nan
    assert _cs_call(L, g, synd, llr, hard, bad, 7) == -1
    bad[3] = np.inf
    assert _cs_call(L, g, synd, llr, hard, bad, 7) == -1
    assert _cs_call(L, g, synd[:0], llr[:0], hard[:0], w, 7) == 0
    assert L.lib().qldpc_osdcs_batch(None, 1, None, None, None, None, 7, None, None) == -1
    with pytest.raises(ValueError):
        L.osdcs_batch(g, synd, llr, hard, w, 65)


def test_circ288_is_unsupported(L):
    from qldpc_amd.data import load_circuit_matrices
    d = load_circuit_matrices("circ288")
    g = L.Graph(d["HdecZ_indptr"], d["HdecZ_indices"], int(d["HdecZ_shape"][1]))
    assert g.m > 1024
    n = g.n
    assert _cs_call(L, g, np.zeros((1, g.m), np.int8), np.ones((1, n)), np.zeros((1, n), np.int8), np.ones(n), 7) == -4
    with pytest.raises(L.QldpcError, match="1024"):
        L.osdcs_batch(g, np.zeros((1, g.m), np.int8), np.ones((1, n)), np.zeros((1, n), np.int8), np.ones(n), 7)


@pytest.mark.parametrize("order", ORDERS)
def test_bit_exact_circ144(L, golden, order):
    f = golden("circ144_decode")
    lighter = 0
    for s in "ZX":
        g = _circ144(L, s)
        synd, llr, hard, w = f[f"{s}_syndromes"], f[f"{s}_llr"], f[f"{s}_err"], f[f"llrs_{s}"]
        sol, fl, outside, o0 = _check(L, g, synd, llr, hard, w, order)
        assert not outside.any()
        assert np.array_equal(L.gf2_spmv_batch(g, sol), synd & 1)
        c_cs, c_0 = _cost(sol, w), _cost(o0, w)
        assert (c_cs <= c_0).all()
        lighter += int((c_cs < c_0).sum())
        if order <= 1:
            assert (fl[:, 1] == -1).all()
        if order == 0:
            assert (fl[:, 0] >= 0).any()                                     # singles are swept at every order
    assert lighter > 0


@pytest.mark.parametrize("order", ORDERS)
def test_bit_exact_circ72(L, golden, order):
    f = golden("circ72_decode")
    from qldpc_amd.data import load_circuit_matrices
    d = load_circuit_matrices("circ72")
    for s in "ZX":
        g = L.Graph(d[f"Hdec{s}_indptr"], d[f"Hdec{s}_indices"], int(d[f"Hdec{s}_shape"][1]))
        _check(L, g, f[f"{s}_syndromes"], f[f"{s}_llr"], f[f"{s}_err"], f[f"llrs_{s}"], order)


@pytest.mark.parametrize("order", ORDERS)
def test_bit_exact_bb72_bp_failures(L, golden, order):
    g0 = golden("bb72_minsum")
    for H, p in (("Hx", "p080"), ("Hz", "p030"), ("Hx", "p030")):
        ip, ix, n = g0[f"{H}_indptr"], g0[f"{H}_indices"], int(g0[f"{H}_shape"][1])
        synd, prior = g0[f"{H}_{p}_syndromes"], g0[f"{H}_{p}_prior"]
        g = L.Graph(ip, ix, n)
        err, conv, llr, _ = L.minsum_decode_batch(g, synd, prior, 30, "dynamical", 1.0)
        bad = np.flatnonzero(conv == 0)
        if bad.size:
            _check(L, g, synd[bad], llr[bad], err[bad], prior, order)


@pytest.mark.parametrize("order", ORDERS)
def test_bit_exact_small_graphs(L, golden, order):
    f = golden("osdw")
    graphs = {}
    nout = 0
    rng = np.random.default_rng(order)
    for case in f["cases"]:
        name = str(f[f"{case}__graph"])
        if name not in graphs:
            H = f[f"graph__{name}"]
            ip, ix, shape = L.canonical_csr(H)
            graphs[name] = (L.Graph(ip, ix, shape[1]), H)
        g, H = graphs[name]
        w = rng.uniform(-2.0, 5.0, g.n)
        out = _check(L, g, f[f"{case}__syndrome"][None], f[f"{case}__llr"][None], f[f"{case}__hard"][None], w, order)[2]
        nout += int(out.sum())
    assert nout > 0                                                          # the fixtures hold foreign, unsatisfiable syndromes


def test_random_small_matrices(L):
    rng = np.random.default_rng(5)
    for trial in range(12):
        m, n = int(rng.integers(3, 40)), int(rng.integers(5, 90))
        H = (rng.random((m, n)) < 0.15).astype(np.int8)
        H[:, rng.integers(0, n)] = 0                                         # a zero column
        ip, ix, shape = L.canonical_csr(H)
        g = L.Graph(ip, ix, n)
        B = 6
        hard = (rng.random((B, n)) < 0.2).astype(np.int8)
        e = (rng.random((B, n)) < 0.2).astype(np.int8)
        synd = (e.astype(np.int64) @ H.T.astype(np.int64) % 2).astype(np.int8)
        llr = np.round(rng.normal(0, 2, (B, n)), 0)                          # many ties
        llr[0, :3] = [np.inf, -np.inf, np.nan]
        w = np.where(rng.random(n) < 0.5, 1.0, rng.uniform(0.1, 3.0, n))
        for order in (0, 1, 7, 64):
            _check(L, g, synd, llr, hard, w, order)


def test_batch_splits_and_select_list(L, golden):
    f = golden("circ144_decode")
    s = "X"
    g = _circ144(L, s)
    synd, llr, hard, w = f[f"{s}_syndromes"], f[f"{s}_llr"], f[f"{s}_err"], f[f"llrs_{s}"]
    whole = L.osdcs_batch(g, synd, llr, hard, w, 7)
    for lo, hi in ((0, 1), (1, 9), (9, 16)):
        part = L.osdcs_batch(g, synd[lo:hi], llr[lo:hi], hard[lo:hi], w, 7)
        assert np.array_equal(part[0], whole[0][lo:hi]) and np.array_equal(part[1], whole[1][lo:hi])
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)        # noqa: E731
    ds, dl, dh, dw = t(synd), t(llr), t(hard), t(np.asarray(w, np.float64))
    sel = np.array([3, 0, 11, 7], np.int32)
    dsel, dcnt = t(sel), t(np.array([sel.size], np.int32))
    dsol = torch.full((16, g.n), 5, dtype=torch.int8, device=dev)
    dfl = torch.full((16, 2), -7, dtype=torch.int32, device=dev)
    rc = L.lib().qldpc_osdcs_batch_dev(g.handle, 16, C.c_void_p(ds.data_ptr()), C.c_void_p(dl.data_ptr()), C.c_void_p(dh.data_ptr()),
                                       C.c_void_p(dw.data_ptr()), 7, C.c_void_p(dsel.data_ptr()), C.c_void_p(dcnt.data_ptr()),
                                       C.c_void_p(dsol.data_ptr()), C.c_void_p(dfl.data_ptr()), C.c_void_p(0))
    assert rc == 0
    torch.cuda.synchronize()
    sol, fl = dsol.cpu().numpy(), dfl.cpu().numpy()
    for i in range(16):
        if i in sel:
            assert np.array_equal(sol[i], whole[0][i]) and np.array_equal(fl[i], whole[1][i])
        else:
            assert (sol[i] == 5).all() and (fl[i] == -7).all()


def test_two_streams_on_one_graph(L, golden):
    f = golden("circ144_decode")
    g = _circ144(L, "Z")
    synd, llr, hard, w = f["Z_syndromes"], f["Z_llr"], f["Z_err"], f["llrs_Z"]
    alone = L.osdcs_batch(g, synd, llr, hard, w, 7)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)        # noqa: E731
    ds, dl, dh, dw = t(synd), t(llr), t(hard), t(np.asarray(w, np.float64))
    outs = [(torch.zeros((16, g.n), dtype=torch.int8, device=dev), torch.zeros((16, 2), dtype=torch.int32, device=dev)) for _ in range(2)]
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    torch.cuda.synchronize()
    for (dsol, dfl), st in zip(outs, streams):
        rc = L.lib().qldpc_osdcs_batch_dev(g.handle, 16, C.c_void_p(ds.data_ptr()), C.c_void_p(dl.data_ptr()), C.c_void_p(dh.data_ptr()),
                                           C.c_void_p(dw.data_ptr()), 7, None, None, C.c_void_p(dsol.data_ptr()), C.c_void_p(dfl.data_ptr()),
                                           C.c_void_p(st.cuda_stream))
        assert rc == 0
    torch.cuda.synchronize()
    for dsol, dfl in outs:
        assert np.array_equal(dsol.cpu().numpy(), alone[0]) and np.array_equal(dfl.cpu().numpy(), alone[1])
    res = {}

    def host(k):
        res[k] = L.osdcs_batch(g, synd, llr, hard, w, 7)
    ts = [threading.Thread(target=host, args=(k,)) for k in range(2)]
    for th in ts:
        th.start()
    for th in ts:
        th.join()
    for k in range(2):
        assert np.array_equal(res[k][0], alone[0]) and np.array_equal(res[k][1], alone[1])


def _host_verdicts(L, tag, seed, count, order):
    """sampler -> BP -> (OSD-CS of `order`, or OSD-0 when order is None) on the unconverged shots -> numpy judge."""
    c, compiled, Mx, graphs, priors, masks, plan = circuit_setup(L, tag)
    p = plan(batch=count)
    spz, tz, spx, tx = p.sample(seed, 0, count)
    p.close()
    verdict = np.zeros(count, np.uint8)
    conv_sum, osd_sum, unsat = [], [], []
    for sec, (g, prior, mask, synd, true) in enumerate(((graphs[0], priors[0], masks[0], spz, tz), (graphs[1], priors[1], masks[1], spx, tx))):
        det, conv, llr, iters = L.minsum_decode_batch(g, synd, prior, 50, "dynamical", 1.0)
        bad = np.flatnonzero(conv == 0)
        if bad.size:
            if order is None:
                det[bad] = L.osd0_batch(g, synd[bad], llr[bad], det[bad])
            else:
                det[bad] = L.osdcs_batch(g, synd[bad], llr[bad], det[bad], prior, order)[0]
        k = true.shape[1]
        rows = np.stack([(mask >> np.uint64(r)) & np.uint64(1) for r in range(k)]).astype(np.int64)
        dec = (det.astype(np.int64) @ rows.T) % 2
        verdict |= (np.any(dec != true.astype(np.int64), axis=1).astype(np.uint8) << sec)
        conv_sum.append(int(conv.sum())); osd_sum.append(int(bad.size))
        unsat.append(int((L.gf2_spmv_batch(g, det) != (synd & 1)).any(axis=1).sum()))
    return verdict, conv_sum, osd_sum, unsat


@pytest.mark.parametrize("order", [None, 7])
def test_circuit_plan_matches_the_pieces(L, order):
    count, seed = 2048, 9876
    verdict, conv, osd, unsat = _host_verdicts(L, "circ72", seed, count, order)
    c, compiled, Mx, graphs, priors, masks, plan = circuit_setup(L, "circ72")
    p = plan(batch=1024)
    if order is not None:
        p.use_osd_cs(order)
    got = p.run_outcomes(seed, 0, count)
    tally = p.read(clear=True)
    ph, _ = p.phase_times()
    p.close()
    T = L.TALLY
    assert np.array_equal(got, verdict)
    assert tally[T["trials"]] == count and tally[T["total_err"]] == np.count_nonzero(verdict)
    assert tally[T["z_err"]] == np.count_nonzero(verdict & 1) and tally[T["x_err"]] == np.count_nonzero(verdict & 2)
    assert [tally[T["bp_conv_z"]], tally[T["bp_conv_x"]]] == conv
    assert [tally[T["osd_z"]], tally[T["osd_x"]]] == osd
    assert [tally[T["unsat_z"]], tally[T["unsat_x"]]] == unsat == [0, 0]
    assert tally[T["legs_z"]] == 0 and tally[T["legs_x"]] == 0
    assert ph["osd_z"] > 0 and ph["osd_x"] > 0


def test_plan_switch_rules(L):
    c, compiled, Mx, graphs, priors, masks, plan = circuit_setup(L, "circ72")
    p = plan(batch=256, use_osd=False)
    with pytest.raises(L.QldpcError):
        p.use_osd_cs(7)
    p.close()
    p = plan(batch=256)
    p.use_relay()
    with pytest.raises(L.QldpcError):
        p.use_osd_cs(7)
    p.close()
    p = plan(batch=256)
    with pytest.raises(ValueError):
        p.use_osd_cs(65)
    p.use_osd_cs(7)
    with pytest.raises(L.QldpcError):
        p.use_relay()
    p.close()

    # the switches that stay open: the same decoder again replaces its parameters, and Relay-BP needs no OSD stage
    def tally(p):
        p.run(11, 0, 512)
        t = p.read()
        p.close()
        return t

    one_leg = dict(max_legs=1, stop_after=1)
    p, q, r = plan(batch=256), plan(batch=256), plan(batch=256)
    p.use_relay(**one_leg)
    p.use_relay()
    q.use_relay()
    r.use_relay(**one_leg)
    relay = tally(q)
    assert np.array_equal(tally(p), relay) and not np.array_equal(tally(r), relay)
    p = plan(batch=256, use_osd=False)
    p.use_relay()
    assert np.array_equal(tally(p), relay)
    p, q = plan(batch=256), plan(batch=256)
    p.use_osd_cs(0)
    p.use_osd_cs(7)
    q.use_osd_cs(7)
    assert np.array_equal(tally(p), tally(q))


def test_run_simulation_lowers_the_logical_error_count(L):
    from qldpc_amd.data import load_code, load_precomputed_matrices
    from qldpc_amd.simulation.engine import run_simulation
    c = load_code("bb72")
    kw = dict(num_cycles=6, precomputed_matrices=load_precomputed_matrices("circ72"), base_seed=2026, batch=4096, **_bb_params(c))
    r0 = run_simulation(c["Hx"], c["Hz"], c["Lx"], c["Lz"], 0.005, num_trials=8192, devices=[0], **kw)
    r1 = run_simulation(c["Hx"], c["Hz"], c["Lx"], c["Lz"], 0.005, num_trials=8192, devices=[0], decoder="bp_osd_cs", osd_order=7, **kw)
    r2 = run_simulation(c["Hx"], c["Hz"], c["Lx"], c["Lz"], 0.005, num_trials=8192, devices=[0, 0], decoder="bp_osd_cs", osd_order=7, **kw)
    print("bp_osd", r0["tally"][L.TALLY["total_err"]], "bp_osd_cs", r1["tally"][L.TALLY["total_err"]])
    assert r1["decoder"] == "bp_osd_cs" and r1["osd_order"] == 7
    assert np.array_equal(r1["tally"], r2["tally"])
    T = L.TALLY
    assert r1["tally"][T["osd_z"]] == r0["tally"][T["osd_z"]] and r1["tally"][T["osd_x"]] == r0["tally"][T["osd_x"]]
    assert r1["tally"][T["total_err"]] < r0["tally"][T["total_err"]]
