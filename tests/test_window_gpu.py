"""Sliding-window decoding on the MI355X: bit-exactness against tests/window_model.py on every shot, the link to the whole-graph min-sum + OSD-0,
shared window graphs, batch splits, the device entry point, two host threads on one decoder, the circuit plan switch, run_simulation and an
experiment longer than the LDS-resident forms hold."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import window_model as WM  # noqa: E402
from test_relay_gpu import _bb_params, circuit_setup, sampled  # noqa: E402

pytestmark = pytest.mark.gpu

LAYER_ROWS = {"circ72": 36, "circ144": 72}
NAMES = ("err", "conv", "iters", "osd", "unsat")


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


def _configs(layers):
    return ((layers, layers), (4, 2), (3, 1), (5, 5))


def _inputs(L, golden, tag):
    """per sector: (graph, prior, syndromes = the golden ones followed by 512 plan-sampled trials)"""
    c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, tag)
    f = golden(f"{tag}_decode")
    (spz, _), (spx, _) = sampled(L, tag, 512, seed=77)
    return [(graphs[0], priors[0], np.concatenate([f["Z_syndromes"], spz])), (graphs[1], priors[1], np.concatenate([f["X_syndromes"], spx]))]


def _assert_equal(got, want, what):
    for name, a, b in zip(NAMES, got, want):
        bad = np.flatnonzero((a != b).reshape(len(a), -1).any(axis=1))
        assert bad.size == 0, f"{what}: {name} differs from the model on shots {bad[:8].tolist()} ({bad.size} of {len(a)})"


@pytest.mark.parametrize("tag", ["circ72", "circ144"])
def test_library_equals_model_on_every_shot(L, golden, oracle, tag):
    lr = LAYER_ROWS[tag]
    for sec, (g, prior, synd) in enumerate(_inputs(L, golden, tag)):
        layers = g.m // lr
        for W, Cm in _configs(layers):
            dec = L.WindowDecoder(g, lr, W, Cm, prior, max_iter=50)
            model = WM.WindowModel(g.indptr, g.indices, g.n, prior, lr, W, Cm)
            info = dec.info()
            got = dec.decode(synd)
            dec.close()
            want = model.decode(oracle, synd, max_iter=50)
            print(f"{tag} sector {sec} (W, C) = ({W}, {Cm}): {info}; shots {len(synd)}, osd windows {int(want[3].sum())}, unsat {int(want[4].sum())}")
            _assert_equal(got, want, f"{tag} sector {sec} ({W}, {Cm})")
            assert info["windows"] == len(model.stages) and info["graphs"] == model.distinct_graphs()
            assert info["max_rows"] == max(s["r1"] - s["r0"] for s in model.stages) and info["max_cols"] == max(s["cols"].size for s in model.stages)
            assert np.array_equal((L.gf2_spmv_batch(g, got[0]) != (synd & 1)).any(axis=1), got[4] != 0)   # unsat is exactly H err != s


@pytest.mark.parametrize("tag", ["circ72", "circ144"])
def test_one_window_is_minsum_plus_osd0(L, golden, tag):
    lr = LAYER_ROWS[tag]
    for g, prior, synd in _inputs(L, golden, tag):
        layers = g.m // lr
        for W, Cm in ((layers, layers), (layers + 3, 2)):
            dec = L.WindowDecoder(g, lr, W, Cm, prior, max_iter=50)
            assert dec.info()["windows"] == 1 and dec.info()["graphs"] == 1
            err, conv, iters, osd, unsat = dec.decode(synd)
            dec.close()
            det, cv, llr, it = L.minsum_decode_batch(g, synd, prior, 50, "dynamical", 1.0)
            bad = np.flatnonzero(cv == 0)
            if bad.size:
                det[bad] = L.osd0_batch(g, synd[bad], llr[bad], det[bad])
            assert np.array_equal(err, det)
            assert np.array_equal(conv, cv.astype(np.int32)) and np.array_equal(iters, it + 1) and np.array_equal(osd, 1 - cv.astype(np.int32))


@pytest.mark.parametrize("tag", ["circ72", "circ144"])
def test_interior_windows_share_one_graph(L, tag):
    c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, tag)
    lr = LAYER_ROWS[tag]
    for g, prior in zip(graphs, priors):
        layers = g.m // lr
        for W, Cm in ((3, 1), (2, 1), (4, 2)):
            dec = L.WindowDecoder(g, lr, W, Cm, prior)
            info = dec.info()
            dec.close()
            starts = [a for a, _, _ in WM.windows(layers, W, Cm)]
            interior = [a for a in starts if a >= 1 and a + W <= layers - 2]
            assert info["windows"] == len(starts)
            assert info["graphs"] == len(starts) - max(len(interior) - 1, 0), (info, starts, interior)
            assert info["max_rows"] == W * lr
            # every window takes the decoder form a host-prior decode of its graph takes: the LDS-resident workgroup form where it is eligible
            model = WM.WindowModel(g.indptr, g.indices, g.n, prior, lr, W, Cm)
            paths = {}
            for gid, st in zip(model.graph_ids(), model.stages):
                if gid not in paths:
                    wg = L.Graph(st["indptr"], st["indices"], st["cols"].size)
                    paths[gid] = L.minsum_decode_path(wg, st["prior"], 50, "dynamical", 1.0)[0]
            assert info["wg2_windows"] == sum(paths[gid] == L.PATH_WG2 for gid in model.graph_ids()), (info, paths)
            if tag == "circ144" and (W, Cm) == (4, 2):
                assert paths[model.graph_ids()[1]] == L.PATH_WG2 and info["wg2_windows"] >= len(interior)      # the shared interior graph


def test_c_level_validation(L):
    c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, "circ72")
    g, prior = graphs[0], priors[0]

    def create(lr, W, Cm, pr=prior, mode=1):
        out = C.c_void_p()
        pr = np.ascontiguousarray(pr, np.float64)
        rc = L.lib().qldpc_window_decoder_create(g.handle, lr, W, Cm, L.ptr(pr, C.c_double), 50, mode, 1.0, None, 0, 20.0, 0, C.byref(out))
        if rc == 0:
            L.lib().qldpc_window_decoder_destroy(out)
        return rc
    assert create(36, 4, 2) == 0
    for args in ((35, 4, 2), (0, 4, 2), (36, 0, 0), (36, 4, 0), (36, 4, 5), (36, -1, 1)):
        assert create(*args) == -1, args
    bad = prior.copy()
    bad[7] = np.inf
    assert create(36, 4, 2, bad) == -1
    assert create(36, 4, 2, prior, mode=9) == -1
    assert create(12, 4, 2) == -1 and b"layers" in L.lib().qldpc_last_error()          # thirds of a cycle: columns span more than two layers
    dec = L.WindowDecoder(g, 36, 4, 2, prior)
    assert L.lib().qldpc_window_decode_batch(dec.handle, 0, None, None, None, None, None, None) == 0     # B = 0: a no-op
    assert L.lib().qldpc_window_decode_batch(dec.handle, 1, None, None, None, None, None, None) == -1
    assert L.lib().qldpc_window_decode_batch(None, 0, None, None, None, None, None, None) == -1
    dec.close()


def test_python_decoder_matches_the_wrapper(L, golden):
    from qldpc_amd.decoding.window import SlidingWindowDecoder
    g, prior, synd = _inputs(L, golden, "circ72")[0]
    d1 = SlidingWindowDecoder((g.indptr, g.indices, g.n), prior, 36, 4, 2)
    err, info = d1.decode(synd[:32])
    dec = L.WindowDecoder(g, 36, 4, 2, prior)
    want = dec.decode(synd[:32])
    dec.close()
    assert np.array_equal(err, want[0]) and info["windows"] == 3
    for k, w in zip(NAMES[1:], want[1:]):
        assert np.array_equal(info[k], w)
    e1, i1 = d1.decode(synd[5])
    assert np.array_equal(e1, want[0][5]) and i1["iters"] == want[2][5] and i1["osd"] == want[3][5]


def test_batch_splits_dev_call_and_two_threads(L, golden):
    g, prior, synd = _inputs(L, golden, "circ144")[1]
    synd = synd[:200]
    dec = L.WindowDecoder(g, 72, 4, 2, prior)
    whole = dec.decode(synd)
    assert whole[3].sum() > 0                                               # some windows went through OSD-0
    for lo, hi in ((0, 1), (1, 77), (77, 200)):
        part = dec.decode(synd[lo:hi])
        for a, b in zip(part, whole):
            assert np.array_equal(a, b[lo:hi])
    dev = torch.device("cuda:0")
    B = len(synd)
    ds = torch.from_numpy(np.ascontiguousarray(synd)).to(dev)
    derr = torch.full((B, g.n), 5, dtype=torch.int8, device=dev)
    dconv, dit, dosd = (torch.full((B,), -3, dtype=torch.int32, device=dev) for _ in range(3))
    dun = torch.full((B,), 9, dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    rc = L.lib().qldpc_window_decode_batch_dev(dec.handle, B, C.c_void_p(ds.data_ptr()), C.c_void_p(derr.data_ptr()), C.c_void_p(dconv.data_ptr()),
                                               C.c_void_p(dit.data_ptr()), C.c_void_p(dosd.data_ptr()), C.c_void_p(dun.data_ptr()), C.c_void_p(st.cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    for a, b in zip((derr, dconv, dit, dosd, dun), whole):
        assert np.array_equal(a.cpu().numpy(), b)
    res = {}

    def host(k):
        res[k] = dec.decode(synd)
    ts = [threading.Thread(target=host, args=(k,)) for k in range(2)]
    for th in ts:
        th.start()
    for th in ts:
        th.join()
    for k in range(2):
        for a, b in zip(res[k], whole):
            assert np.array_equal(a, b)
    dec.close()


def _host_verdicts(L, setup, layer_rows, seed, count, WC):
    """sampler -> SlidingWindowDecoder per sector -> numpy judge (as test_osd_cs_gpu._host_verdicts does for OSD-CS)."""
    c, compiled, Mx, graphs, priors, masks, plan = setup
    p = plan(batch=count)
    spz, tz, spx, tx = p.sample(seed, 0, count)
    p.close()
    verdict = np.zeros(count, np.uint8)
    out = dict(conv=[], osd=[], unsat=[], iters=[], err=[], synd=[spz, spx])
    for sec, (g, prior, mask, synd, true) in enumerate(((graphs[0], priors[0], masks[0], spz, tz), (graphs[1], priors[1], masks[1], spx, tx))):
        dec = L.WindowDecoder(g, layer_rows, WC[0], WC[1], prior, max_iter=50)
        det, conv, iters, osd, unsat = dec.decode(synd)
        nwin = dec.info()["windows"]
        dec.close()
        k = true.shape[1]
        rows = np.stack([(mask >> np.uint64(r)) & np.uint64(1) for r in range(k)]).astype(np.int64)
        dd = (det.astype(np.int64) @ rows.T) % 2
        verdict |= (np.any(dd != true.astype(np.int64), axis=1).astype(np.uint8) << sec)
        out["conv"].append(int((conv == nwin).sum())); out["osd"].append(int((osd > 0).sum())); out["unsat"].append(int(unsat.sum()))
        out["iters"].append(int(iters.sum())); out["err"].append(det)
    return verdict, out


@pytest.mark.parametrize("WC", [(4, 2), (3, 1)])
def test_circuit_plan_matches_the_pieces(L, WC):
    count, seed = 2048, 4321
    setup = circuit_setup(L, "circ72")
    verdict, h = _host_verdicts(L, setup, 36, seed, count, WC)
    p = setup[6](batch=1024)
    p.use_window(*WC)
    got = p.run_outcomes(seed, 0, count)
    tally = p.read(clear=True)
    ph, _ = p.phase_times()
    p.close()
    T = L.TALLY
    assert np.array_equal(got, verdict)
    assert tally[T["trials"]] == count and tally[T["total_err"]] == np.count_nonzero(verdict)
    assert tally[T["z_err"]] == np.count_nonzero(verdict & 1) and tally[T["x_err"]] == np.count_nonzero(verdict & 2)
    assert [tally[T["bp_conv_z"]], tally[T["bp_conv_x"]]] == h["conv"]
    assert [tally[T["osd_z"]], tally[T["osd_x"]]] == h["osd"]
    assert [tally[T["iters_z"]], tally[T["iters_x"]]] == h["iters"]
    assert [tally[T["unsat_z"]], tally[T["unsat_x"]]] == h["unsat"]
    assert tally[T["legs_z"]] == 0 and tally[T["legs_x"]] == 0
    assert ph["bp_z"] > 0 and ph["osd_z"] > 0 and ph["bp_x"] > 0 and ph["osd_x"] > 0


def test_unswitched_plan_is_unchanged(L):
    """an unswitched plan's tally for a fixed seed: the same before and after windowed plans ran, and equal to the one-window plan's"""
    setup = circuit_setup(L, "circ72")
    p = setup[6](batch=1024)
    p.run(99, 0, 3000)
    t0 = p.read(clear=True)
    p.close()
    w = setup[6](batch=1024)
    w.use_window(8, 8)
    w.run(99, 0, 3000)
    tw = w.read(clear=True)
    w.close()
    p = setup[6](batch=1024)
    p.run(99, 0, 3000)
    t1 = p.read(clear=True)
    p.close()
    assert np.array_equal(t0, t1)
    assert np.array_equal(t0, tw)                                           # one window = the whole graph: every slot agrees


def test_plan_switch_rules(L):
    plan = circuit_setup(L, "circ72")[6]
    p = plan(batch=256, use_osd=False)
    with pytest.raises(L.QldpcError):
        p.use_window(4, 2)
    p.close()
    p = plan(batch=256)
    p.use_relay()
    with pytest.raises(L.QldpcError):
        p.use_window(4, 2)
    p.close()
    p = plan(batch=256)
    p.use_osd_cs(7)
    with pytest.raises(L.QldpcError):
        p.use_window(4, 2)
    p.close()
    p = plan(batch=256, damping=0.5)
    with pytest.raises(L.QldpcError):
        p.use_window(4, 2)
    p.close()
    p = plan(batch=256)
    with pytest.raises(ValueError):
        p.use_window(2, 3)
    p.use_window(4, 2)
    for again in (lambda: p.use_window(4, 2), lambda: p.use_relay(), lambda: p.use_osd_cs(7)):
        with pytest.raises(L.QldpcError):
            again()
    p.close()


def test_run_simulation_window(L):
    from qldpc_amd.data import load_code, load_precomputed_matrices
    from qldpc_amd.simulation.engine import run_simulation
    c = load_code("bb72")
    kw = dict(num_cycles=6, precomputed_matrices=load_precomputed_matrices("circ72"), base_seed=2027, batch=2048, **_bb_params(c))
    r1 = run_simulation(c["Hx"], c["Hz"], c["Lx"], c["Lz"], 0.005, num_trials=6000, devices=[0], window=(4, 2), **kw)
    r2 = run_simulation(c["Hx"], c["Hz"], c["Lx"], c["Lz"], 0.005, num_trials=6000, devices=[0, 0], window=(4, 2), **kw)
    assert r1["window"] == (4, 2) and r1["tally"][L.TALLY["trials"]] == 6000
    assert np.array_equal(r1["tally"], r2["tally"])
    for bad in (dict(decoder="relay_bp"), dict(decoder="bp_osd_cs", osd_order=7), dict(osd_order=1)):
        with pytest.raises(ValueError):
            run_simulation(c["Hx"], c["Hz"], c["Lx"], c["Lz"], 0.005, num_trials=100, devices=[0], window=(4, 2), **dict(kw, **bad))


def test_long_experiment_end_to_end(L, oracle):
    """[[72,12,6]] x 30 cycles: m = 1152 rows, beyond the LDS-resident forms; the windows are 216-row graphs whatever the length."""
    from qldpc_amd.data import load_code
    from qldpc_amd.codes.bb_code import BBCodeCircuit
    from qldpc_amd.noise.compiled import CompiledCircuit
    from qldpc_amd.noise.builder import build_decoding_matrices
    from qldpc_amd.simulation.engine import prior_llrs, run_simulation
    c = load_code("bb72")
    cycles, p_err, WC = 30, 0.005, (6, 3)
    cb = BBCodeCircuit(c["Hx"], c["Hz"], num_cycles=cycles, **_bb_params(c))
    Mx = build_decoding_matrices(cb, c["Lx"], c["Lz"], p_err, verbose=False)
    r = run_simulation(c["Hx"], c["Hz"], c["Lx"], c["Lz"], p_err, num_trials=4096, num_cycles=cycles, precomputed_matrices=Mx, base_seed=31, batch=2048,
                       devices=[0], window=WC, **_bb_params(c))
    T = L.TALLY
    assert r["tally"][T["trials"]] == 4096 and r["window"] == WC
    compiled = CompiledCircuit(base_circuit=cb.get_full_circuit(), noiseless_suffix=cb.cycle * 2, lin_order=cb.lin_order, data_qubits=cb.data_qubits,
                               Xchecks=cb.Xchecks, Zchecks=cb.Zchecks)
    k = np.asarray(c["Lx"]).shape[0]
    graphs, priors, masks = [], [], []
    for s in ("Z", "X"):
        ip, ix, shape = L.canonical_csr(Mx[f"Hdec{s}"])
        assert shape[0] == 36 * (cycles + 2) == 1152
        graphs.append(L.Graph(ip, ix, shape[1]))
        priors.append(prior_llrs(np.asarray(Mx[f"channel_probs{s}"], dtype=np.float64)))
        if f"H{s}_logical" in Mx:
            masks.append(L.logical_column_masks(Mx[f"H{s}_logical"], shape[1]))
        else:
            flr = int(Mx[f"first_logical_row{s}"])
            masks.append(L.logical_column_masks(np.asarray(Mx[f"H{s}_full"])[flr:flr + k], shape[1]))

    def plan(batch=1024, **kw):
        return L.CircuitPlan(compiled, c["Lx"], c["Lz"], graphs[0], graphs[1], priors[0], priors[1], masks[0], masks[1], p_err, batch=batch, **kw)
    setup = (c, compiled, Mx, graphs, priors, masks, plan)
    count = 256
    verdict, h = _host_verdicts(L, setup, 36, 31, count, WC)
    for sec in range(2):
        g = graphs[sec]
        dec = L.WindowDecoder(g, 36, WC[0], WC[1], priors[sec])
        info = dec.info()
        got = dec.decode(h["synd"][sec])
        dec.close()
        model = WM.WindowModel(g.indptr, g.indices, g.n, priors[sec], 36, *WC)
        want = model.decode(oracle, h["synd"][sec], max_iter=50)
        _assert_equal(got, want, f"30 cycles, sector {sec}")
        assert np.array_equal(got[0], h["err"][sec])
        assert info["windows"] == 10 and info["max_rows"] == 216 and info["graphs"] == model.distinct_graphs() <= 4
    p = plan(batch=256)
    p.use_window(*WC)
    assert np.array_equal(p.run_outcomes(31, 0, count), verdict)            # the first 256 trials of the run above
    t = p.read(clear=True)
    p.close()
    assert [t[T["osd_z"]], t[T["osd_x"]]] == h["osd"] and [t[T["unsat_z"]], t[T["unsat_x"]]] == h["unsat"]
