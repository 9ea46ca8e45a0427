"""Relay-BP on the MI355X: C-level checks, bit-exactness against tests/relay_model.py, the link to the plain min-sum decoder, batch splits,
the circuit plan switch, run_simulation, concurrent use of one graph, and that nothing existing changes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import relay_model as RM  # noqa: E402

pytestmark = pytest.mark.gpu

SCALED = dict(t0=20, tr=10, max_legs=20)
PARAM_SETS = {
    "scaled": dict(SCALED),
    "stop1": dict(SCALED, stop_after=1),
    "stop3": dict(SCALED, stop_after=3),
    "negative": dict(SCALED, gamma0=-0.1, gamma_min=-0.3, gamma_max=-0.05),
    "point": dict(SCALED, gamma_min=0.2, gamma_max=0.2),
}


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


def _bb_params(c):
    return dict(ell=c["ell"], m=c["m_dim"], a_x_powers=c["a_x_powers"], a_y_powers=c["a_y_powers"], b_y_powers=c["b_y_powers"],
                b_x_powers=c["b_x_powers"])


_SETUPS = {}


def circuit_setup(L, tag):
    """(code, compiled circuit, matrices, graphs [Z, X], priors, masks, plan factory) of a bundled circuit-level matrix set."""
    if tag in _SETUPS:
        return _SETUPS[tag]
    from qldpc_amd.data import load_code, load_precomputed_matrices
    from qldpc_amd.codes.bb_code import BBCodeCircuit
    from qldpc_amd.noise.compiled import CompiledCircuit
    from qldpc_amd.simulation.engine import prior_llrs
    code = {"circ72": "bb72", "circ144": "bb144"}[tag]
    c = load_code(code)
    M = load_precomputed_matrices(tag)
    cb = BBCodeCircuit(c["Hx"], c["Hz"], num_cycles=M["num_cycles"], **_bb_params(c))
    compiled = CompiledCircuit(base_circuit=cb.get_full_circuit(), noiseless_suffix=cb.cycle * 2, lin_order=cb.lin_order, data_qubits=cb.data_qubits,
                               Xchecks=cb.Xchecks, Zchecks=cb.Zchecks)
    graphs, priors, masks = [], [], []
    for s in ("Z", "X"):
        ip, ix, shape = L.canonical_csr(M[f"Hdec{s}"])
        graphs.append(L.Graph(ip, ix, shape[1]))
        priors.append(prior_llrs(np.asarray(M[f"channel_probs{s}"], dtype=np.float64)))
        masks.append(L.logical_column_masks(M[f"H{s}_logical"], shape[1]))

    def plan(batch=1024, **kw):
        return L.CircuitPlan(compiled, c["Lx"], c["Lz"], graphs[0], graphs[1], priors[0], priors[1], masks[0], masks[1], 0.005, batch=batch, **kw)
    _SETUPS[tag] = (c, compiled, M, graphs, priors, masks, plan)
    return _SETUPS[tag]


def sampled(L, tag, count, seed=11):
    c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, tag)
    p = plan(batch=max(count, 1))
    spz, tz, spx, tx = p.sample(seed, 0, count)
    p.close()
    return (spz, tz), (spx, tx)


def _relay_call(L, g, synd, prior, seed, shot_begin=0, tag=0, **kw):
    """Raw C call on host arrays -> return code (for the argument checks)."""
    synd = np.ascontiguousarray(synd, np.int8).reshape(-1, g.m)
    prior = np.ascontiguousarray(prior, np.float64)
    B = synd.shape[0]
    p = dict(L.RELAY_DEFAULTS, **kw)
    err, conv = np.zeros((max(B, 1), g.n), np.int8), np.zeros(max(B, 1), np.uint8)
    a, b, s = np.zeros(max(B, 1), np.int32), np.zeros(max(B, 1), np.int32), np.zeros(max(B, 1), np.int32)
    return L.lib().qldpc_relay_decode_batch(g.handle, B, L.ptr(synd, C.c_int8), L.ptr(prior, C.c_double), p["alpha"], p["clip_llr"], p["gamma0"],
                                            p["gamma_min"], p["gamma_max"], p["t0"], p["tr"], p["max_legs"], p["stop_after"], C.c_uint64(seed),
                                            shot_begin, tag, L.ptr(err, C.c_int8), L.ptr(conv, C.c_uint8), L.ptr(a, C.c_int32), L.ptr(b, C.c_int32),
                                            L.ptr(s, C.c_int32))


def test_c_level_validation(L):
    c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, "circ72")
    g, prior = graphs[0], priors[0]
    synd = np.zeros((2, g.m), np.int8)
    bad_prior = prior.copy()
    bad_prior[5] = np.inf
    assert _relay_call(L, g, synd, bad_prior, 1) == -1
    for kw in (dict(gamma_min=0.5, gamma_max=0.1), dict(t0=0), dict(stop_after=0), dict(max_legs=2 ** 20), dict(tr=0), dict(alpha=-1.0),
               dict(clip_llr=float("nan")), dict(gamma0=float("inf"))):
        assert _relay_call(L, g, synd, prior, 1, **kw) == -1, kw
    assert _relay_call(L, g, synd, prior, 1, tag=16) == -1
    assert _relay_call(L, g, synd[:0], prior, 1) == 0                       # B = 0: a no-op


@pytest.mark.parametrize("pset", sorted(PARAM_SETS))
def test_bit_exact_against_the_model_circ72(L, pset):
    c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, "circ72")
    (spz, _), (spx, _) = sampled(L, "circ72", 64)
    for tag, (g, prior, synd) in enumerate(((graphs[0], priors[0], spz), (graphs[1], priors[1], spx))):
        got = L.relay_decode_batch(g, synd, prior, 20260916, 5, tag, **PARAM_SETS[pset])
        ref = RM.relay_decode(g.indptr, g.indices, g.n, synd, prior, 20260916, 5, tag, **PARAM_SETS[pset])
        for a, b, what in zip(got, ref, ("err", "conv", "legs", "iters", "solutions")):
            assert np.array_equal(a, b), f"{pset} sector {'ZX'[tag]}: {what} differs"
        if pset == "scaled":
            assert got[2].max() > 1                                          # relay legs ran


@pytest.mark.parametrize("pset", ["scaled", "stop3", "negative"])
def test_bit_exact_against_the_model_bb72(L, golden, pset):
    g0 = golden("bb72_minsum")
    for H, p in (("hx", "p080"), ("hz", "p030")):
        ip, ix, n = g0[f"{H.capitalize()}_indptr"], g0[f"{H.capitalize()}_indices"], int(g0[f"{H.capitalize()}_shape"][1])
        synd, prior = g0[f"{H.capitalize()}_{p}_syndromes"], g0[f"{H.capitalize()}_{p}_prior"]
        g = L.Graph(ip, ix, n)
        got = L.relay_decode_batch(g, synd, prior, 77, 0, 3, **PARAM_SETS[pset])
        ref = RM.relay_decode(ip, ix, n, synd, prior, 77, 0, 3, **PARAM_SETS[pset])
        for a, b, what in zip(got, ref, ("err", "conv", "legs", "iters", "solutions")):
            assert np.array_equal(a, b), f"{pset} {H} {p}: {what} differs"


def test_leg0_without_memory_is_minsum_circ144(L):
    c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, "circ144")
    (spz, _), (spx, _) = sampled(L, "circ144", 96)
    for tag, (g, prior, synd) in enumerate(((graphs[0], priors[0], spz), (graphs[1], priors[1], spx))):
        err, conv, legs, iters, sols = L.relay_decode_batch(g, synd, prior, 5, 0, tag, alpha=0.875, gamma0=0.0, t0=50, max_legs=0, stop_after=1)
        e2, c2, _, i2 = L.minsum_decode_batch(g, synd, prior, 50, "alvarado", 0.875)
        assert np.array_equal(err, e2) and np.array_equal(conv, c2) and np.array_equal(iters, i2 + 1)
        assert (legs == 1).all() and np.array_equal(sols, conv.astype(np.int32))


def test_leg0_without_memory_is_minsum_circ288_vg(L):
    from qldpc_amd.data import load_circuit_matrices
    d = load_circuit_matrices("circ288")
    from qldpc_amd.simulation.engine import prior_llrs
    for s in ("Z", "X"):
        ip, ix, n = d[f"Hdec{s}_indptr"], d[f"Hdec{s}_indices"], int(d[f"Hdec{s}_shape"][1])
        m = len(ip) - 1
        assert n * 8 + 24 * m > 160 * 1024                                   # V does not fit LDS: the HBM/L2 form runs
        g = L.Graph(ip, ix, n)
        prior = prior_llrs(np.asarray(d[f"channel_probs{s}"], dtype=np.float64))
        rng = np.random.default_rng(3)
        E = (rng.random((6, n)) < 0.0015).astype(np.int8)
        E[0] = 0
        synd = L.gf2_spmv_batch(g, E)
        err, conv, legs, iters, sols = L.relay_decode_batch(g, synd, prior, 9, 0, 0, gamma0=0.0, t0=30, max_legs=0, stop_after=1)
        e2, c2, _, i2 = L.minsum_decode_batch(g, synd, prior, 30, "alvarado", 1.0)
        assert np.array_equal(err, e2) and np.array_equal(conv, c2) and np.array_equal(iters, i2 + 1)
        assert conv[0]
        # with relay legs the HBM/L2 form still equals the model on two shots
        got = L.relay_decode_batch(g, synd[:2], prior, 9, 0, 1, t0=8, tr=4, max_legs=3)
        ref = RM.relay_decode(ip, ix, n, synd[:2], prior, 9, 0, 1, t0=8, tr=4, max_legs=3)
        for a, b in zip(got, ref):
            assert np.array_equal(a, b)


def test_relay_only_adds_solutions(L):
    c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, "circ72")
    (spz, _), (spx, _) = sampled(L, "circ72", 256, seed=23)
    for tag, (g, prior, synd) in enumerate(((graphs[0], priors[0], spz), (graphs[1], priors[1], spx))):
        e0, c0, _, _ = L.minsum_decode_batch(g, synd, prior, 40, "alvarado", 1.0)
        err, conv, legs, iters, sols = L.relay_decode_batch(g, synd, prior, 1, 0, tag, gamma0=0.0, t0=40, tr=20, max_legs=30, stop_after=1)
        ok = c0 == 1
        assert conv[ok].all() and np.array_equal(err[ok], e0[ok])
        assert conv.sum() >= c0.sum()
        s = L.gf2_spmv_batch(g, err)
        assert np.array_equal(s[conv == 1], synd[conv == 1] & 1)


def test_splits_and_device_entry(L):
    c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, "circ72")
    (spz, _), _ = sampled(L, "circ72", 128, seed=5)
    g, prior = graphs[0], priors[0]
    kw = dict(t0=20, tr=10, max_legs=15, stop_after=2)
    whole = L.relay_decode_batch(g, spz, prior, 99, 0, 0, **kw)
    a = L.relay_decode_batch(g, spz[:64], prior, 99, 0, 0, **kw)
    b = L.relay_decode_batch(g, spz[64:], prior, 99, 64, 0, **kw)
    for w, x, y in zip(whole, a, b):
        assert np.array_equal(w, np.concatenate([x, y]))
    dev = torch.device("cuda:0")
    ds = torch.from_numpy(np.ascontiguousarray(spz)).to(dev)
    dp = torch.from_numpy(prior).to(dev)
    B, n = spz.shape[0], g.n
    de = torch.zeros((B, n), dtype=torch.int8, device=dev)
    dc = torch.zeros(B, dtype=torch.uint8, device=dev)
    dl, di, dso = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(3))
    p = dict(L.RELAY_DEFAULTS, **kw)
    stream = torch.cuda.current_stream(dev).cuda_stream
    L.check(L.lib().qldpc_relay_decode_batch_dev(g.handle, B, ds.data_ptr(), dp.data_ptr(), p["alpha"], p["clip_llr"], p["gamma0"], p["gamma_min"],
                                                 p["gamma_max"], p["t0"], p["tr"], p["max_legs"], p["stop_after"], C.c_uint64(99), 0, 0, de.data_ptr(),
                                                 dc.data_ptr(), dl.data_ptr(), di.data_ptr(), dso.data_ptr(), C.c_void_p(stream)))
    torch.cuda.synchronize(dev)
    for w, t in zip(whole, (de, dc, dl, di, dso)):
        assert np.array_equal(w, t.cpu().numpy())


def _host_verdicts(L, tag, seed, count, params):
    c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, tag)
    p = plan(batch=count)
    spz, tz, spx, tx = p.sample(seed, 0, count)
    p.close()
    verdict = np.zeros(count, np.uint8)
    legs_sum, iters_sum, conv_sum, unsat = [], [], [], []
    for sec, (g, prior, mask, synd, true) in enumerate(((graphs[0], priors[0], masks[0], spz, tz), (graphs[1], priors[1], masks[1], spx, tx))):
        err, conv, legs, iters, sols = L.relay_decode_batch(g, synd, prior, seed, 0, sec, **params)
        k = true.shape[1]
        rows = np.stack([(mask >> np.uint64(r)) & np.uint64(1) for r in range(k)]).astype(np.int64)
        dec = (err.astype(np.int64) @ rows.T) % 2
        verdict |= (np.any(dec != true.astype(np.int64), axis=1).astype(np.uint8) << sec)
        legs_sum.append(int(legs.sum())); iters_sum.append(int(iters.sum())); conv_sum.append(int(conv.sum()))
        unsat.append(int((L.gf2_spmv_batch(g, err) != (synd & 1)).any(axis=1).sum()))
    return verdict, legs_sum, iters_sum, conv_sum, unsat


RELAY_SMALL = dict(t0=30, tr=15, max_legs=8, stop_after=2)


def test_circuit_plan_matches_the_pieces(L):
    c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, "circ72")
    count, seed = 2048, 4321
    verdict, legs, iters, conv, unsat = _host_verdicts(L, "circ72", seed, count, RELAY_SMALL)
    p = plan(batch=1024)
    p.use_relay(**RELAY_SMALL)
    got = p.run_outcomes(seed, 0, count)
    tally = p.read(clear=True)
    ph, _ = p.phase_times()
    p.close()
    T = L.TALLY
    assert np.array_equal(got, verdict)
    assert tally[T["trials"]] == count
    assert tally[T["z_err"]] == np.count_nonzero(verdict & 1) and tally[T["x_err"]] == np.count_nonzero(verdict & 2)
    assert tally[T["total_err"]] == np.count_nonzero(verdict)
    assert [tally[T["legs_z"]], tally[T["legs_x"]]] == legs
    assert [tally[T["iters_z"]], tally[T["iters_x"]]] == iters
    assert [tally[T["bp_conv_z"]], tally[T["bp_conv_x"]]] == conv
    assert [tally[T["unsat_z"]], tally[T["unsat_x"]]] == unsat
    assert tally[T["osd_z"]] == 0 and tally[T["osd_x"]] == 0
    assert ph["osd_z"] == 0 and ph["osd_x"] == 0 and ph["bp_z"] > 0


def test_run_simulation_workers_and_early_stop(L):
    from qldpc_amd.data import load_code, load_precomputed_matrices
    from qldpc_amd.simulation.engine import run_simulation
    c = load_code("bb72")
    kw = dict(num_cycles=6, precomputed_matrices=load_precomputed_matrices("circ72"), base_seed=777, batch=512, decoder="relay_bp",
              relay_params=RELAY_SMALL, **_bb_params(c))
    r1 = run_simulation(c["Hx"], c["Hz"], c["Lx"], c["Lz"], 0.005, num_trials=1500, devices=[0], **kw)
    r2 = run_simulation(c["Hx"], c["Hz"], c["Lx"], c["Lz"], 0.005, num_trials=1500, devices=[0, 0], **kw)
    assert np.array_equal(r1["tally"], r2["tally"])
    assert r1["decoder"] == "relay_bp" and r1["relay_params"]["t0"] == 30
    assert r1["mean_legs_z"] >= 1.0 and r1["mean_legs_x"] >= 1.0
    assert r1["tally"][L.TALLY["osd_z"]] == 0
    target = 3
    r3 = run_simulation(c["Hx"], c["Hz"], c["Lx"], c["Lz"], 0.005, num_trials=None, max_trials=20000, target_logical_errors=target, devices=[0], **kw)
    verdict = _host_verdicts(L, "circ72", 777, r3["num_trials"], RELAY_SMALL)[0]
    assert np.count_nonzero(verdict) == target and verdict[-1] != 0       # stops AT the trial of the target-th error
    assert r3["logical_errors"] == target


def test_concurrent_streams_on_one_graph(L):
    c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, "circ72")
    import threading
    (spz, _), _ = sampled(L, "circ72", 256, seed=41)
    g, prior = graphs[0], priors[0]
    kw = dict(t0=20, tr=10, max_legs=10)
    alone_r = L.relay_decode_batch(g, spz, prior, 3, 0, 0, **kw)
    alone_b = L.minsum_decode_batch(g, spz, prior, 50, "dynamical", 1.0)
    out = {}

    def relay():
        out["r"] = L.relay_decode_batch(g, spz, prior, 3, 0, 0, **kw)

    def bp():
        out["b"] = L.minsum_decode_batch(g, spz, prior, 50, "dynamical", 1.0)
    for _ in range(3):
        ts = [threading.Thread(target=relay), threading.Thread(target=bp)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        for a, b in zip(out["r"], alone_r):
            assert np.array_equal(a, b)
        for a, b in zip(out["b"], alone_b):
            assert np.array_equal(a, b)
    # device entry points on two torch streams
    dev = torch.device("cuda:0")
    B, n = spz.shape[0], g.n
    ds, dp = torch.from_numpy(np.ascontiguousarray(spz)).to(dev), torch.from_numpy(prior).to(dev)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    de, dc = torch.zeros((B, n), dtype=torch.int8, device=dev), torch.zeros(B, dtype=torch.uint8, device=dev)
    dl, di, dso = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(3))
    be, bl, bc, bi = (torch.zeros((B, n), dtype=torch.int8, device=dev), torch.zeros((B, n), dtype=torch.float64, device=dev),
                      torch.zeros(B, dtype=torch.uint8, device=dev), torch.zeros(B, dtype=torch.int32, device=dev))
    torch.cuda.synchronize(dev)
    p = dict(L.RELAY_DEFAULTS, **kw)
    one = np.zeros(1)
    L.check(L.lib().qldpc_relay_decode_batch_dev(g.handle, B, ds.data_ptr(), dp.data_ptr(), p["alpha"], p["clip_llr"], p["gamma0"], p["gamma_min"],
                                                 p["gamma_max"], p["t0"], p["tr"], p["max_legs"], p["stop_after"], C.c_uint64(3), 0, 0, de.data_ptr(),
                                                 dc.data_ptr(), dl.data_ptr(), di.data_ptr(), dso.data_ptr(), C.c_void_p(s1.cuda_stream)))
    L.check(L.lib().qldpc_minsum_decode_batch_dev(g.handle, B, ds.data_ptr(), dp.data_ptr(), 50, L.ALPHA_DYNAMIC, 1.0, L.ptr(one, C.c_double), 1, 1.0,
                                                  20.0, 0, be.data_ptr(), bl.data_ptr(), bc.data_ptr(), bi.data_ptr(), C.c_void_p(s2.cuda_stream)))
    torch.cuda.synchronize(dev)
    for a, t in zip(alone_r, (de, dc, dl, di, dso)):
        assert np.array_equal(a, t.cpu().numpy())
    assert np.array_equal(alone_b[0], be.cpu().numpy()) and np.array_equal(alone_b[1], bc.cpu().numpy())


def test_nothing_existing_changes(L):
    c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, "circ72")
    before = plan(batch=512)
    before.run(2024, 0, 3000)
    t_before = before.read(clear=True)
    before.close()
    (spz, _), (spx, _) = sampled(L, "circ72", 64, seed=8)
    L.relay_decode_batch(graphs[0], spz, priors[0], 1, 0, 0, **SCALED)
    L.relay_decode_batch(graphs[1], spx, priors[1], 1, 0, 1, **SCALED)
    switched = plan(batch=512)
    switched.use_relay(**RELAY_SMALL)
    switched.run(2024, 0, 1000)
    switched.read(clear=True)
    after = plan(batch=512)
    after.run(2024, 0, 3000)
    t_after = after.read(clear=True)
    after.close()
    switched.close()
    assert np.array_equal(t_before, t_after)
    assert t_before[L.TALLY["legs_z"]] == 0 and t_before[L.TALLY["legs_x"]] == 0
    assert t_before[L.TALLY["osd_z"]] + t_before[L.TALLY["osd_x"]] > 0
