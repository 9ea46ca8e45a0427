"""BP with guided decimation on the MI355X: C-level checks, bit-exactness against tests/decimation_model.py, the link to Relay-BP, the HBM/L2 form,
batch splits and the device entry, concurrent use of one graph, the circuit plan switch and its refusals, run_simulation, and that nothing
existing changes."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import decimation_model as DM  # noqa: E402
from test_relay_gpu import _bb_params, circuit_setup, sampled  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("err", "llr", "conv", "iters", "rounds", "fixed")
BASE = dict(alpha=1.0, clip_llr=20.0, fix_llr=50.0)
PARAM_SETS = {"8x6x1": dict(t_round=8, max_rounds=6, per_round=1), "4x12x16": dict(t_round=4, max_rounds=12, per_round=16),
              "3x40x64": dict(t_round=3, max_rounds=40, per_round=64)}
PLAN = dict(alpha=1.0, t_round=6, max_rounds=10, per_round=8, fix_llr=50.0)


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


def assert_same(got, ref, what):
    for a, b, name in zip(got, ref, NAMES):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {name} has another type or shape"
        if name == "llr":
            assert np.array_equal(a, b, equal_nan=True), f"{what}: llr differs"         # bytes, NaN payloads aside
            assert np.array_equal(np.signbit(a[~np.isnan(a)]), np.signbit(b[~np.isnan(b)])), f"{what}: a zero of llr has another sign"
        else:
            assert a.tobytes() == b.tobytes(), f"{what}: {name} differs"


def _call(L, g, synd, prior, null_outputs=False, **kw):
    """Raw C call on host arrays -> return code (for the argument checks)."""
    synd = np.ascontiguousarray(synd, np.int8).reshape(-1, g.m)
    prior = np.ascontiguousarray(prior, np.float64)
    B = synd.shape[0]
    p = dict(BASE, t_round=4, max_rounds=2, per_round=8)
    p.update(kw)
    err, llr, conv = np.zeros((max(B, 1), g.n), np.int8), np.zeros((max(B, 1), g.n)), np.zeros(max(B, 1), np.uint8)
    a, b, c = (np.zeros(max(B, 1), np.int32) for _ in range(3))
    return L.lib().qldpc_decim_decode_batch(g.handle, B, L.ptr(synd, C.c_int8), L.ptr(prior, C.c_double), p["alpha"], p["clip_llr"], p["t_round"],
                                            p["max_rounds"], p["per_round"], p["fix_llr"], L.ptr(err, C.c_int8), None if null_outputs else L.ptr(llr, C.c_double),
                                            L.ptr(conv, C.c_uint8), L.ptr(a, C.c_int32), None if null_outputs else L.ptr(b, C.c_int32),
                                            None if null_outputs else L.ptr(c, C.c_int32))


def test_c_level_validation(L):
    c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, "circ72")
    g, prior = graphs[0], priors[0]
    synd = np.zeros((2, g.m), np.int8)
    for bad in (np.inf, -np.inf, np.nan):
        bad_prior = prior.copy()
        bad_prior[5] = bad
        assert _call(L, g, synd, bad_prior) == -1
    nan, inf = float("nan"), float("inf")
    for kw in (dict(alpha=0.0), dict(alpha=-1.0), dict(alpha=nan), dict(alpha=inf), dict(clip_llr=0.0), dict(clip_llr=nan), dict(clip_llr=inf),
               dict(fix_llr=0.0), dict(fix_llr=-5.0), dict(fix_llr=nan), dict(fix_llr=inf), dict(t_round=0), dict(t_round=-3), dict(max_rounds=-1),
               dict(max_rounds=2 ** 20), dict(per_round=0), dict(per_round=65)):
        assert _call(L, g, synd, prior, **kw) == -1, kw
    for kw in (dict(t_round=1), dict(max_rounds=0), dict(per_round=1), dict(per_round=64)):                     # the ends of the ranges
        assert _call(L, g, synd, prior, **kw) == 0, kw
    assert _call(L, g, synd, prior, null_outputs=True) == 0                # llr, rounds, fixed may be NULL
    assert _call(L, g, synd[:0], prior) == 0                               # B = 0: a no-op
    assert _call(L, g, synd[:0], prior, alpha=0.0) == -1                   # ... after the argument checks
    wide = L.Graph(np.array([0, 57], np.int32), np.arange(57, dtype=np.int32), 57)                               # row degree 57
    assert _call(L, wide, np.zeros((1, 1), np.int8), np.ones(57)) == -4                                         # QLDPC_ERR_UNSUPPORTED, as Relay-BP
    assert b"row degree" in L.lib().qldpc_last_error()


@pytest.mark.parametrize("pset", sorted(PARAM_SETS))
def test_bit_exact_against_the_model_circ72(L, pset):
    c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, "circ72")
    (spz, _), (spx, _) = sampled(L, "circ72", 16)
    for sec, (g, prior, synd) in enumerate(((graphs[0], priors[0], spz), (graphs[1], priors[1], spx))):
        kw = dict(BASE, **PARAM_SETS[pset])
        got = L.decim_decode_batch(g, synd, prior, **kw)
        ref = DM.decim_decode(g.indptr, g.indices, g.n, synd, prior, **kw)
        print(pset, "ZX"[sec], "conv", ref[2].tolist(), "rounds", ref[4].tolist(), "fixed", ref[5].tolist())
        assert_same(got, ref, f"{pset} sector {'ZX'[sec]}")
        assert ref[4].max() > 1                                            # decimation ran


def test_bit_exact_against_the_model_bb72_ties(L, golden):
    g0 = golden("bb72_minsum")
    ip, ix, n = g0["Hx_indptr"], g0["Hx_indices"], int(g0["Hx_shape"][1])
    synd, prior = g0["Hx_p080_syndromes"][:16], g0["Hx_p080_prior"]
    assert np.unique(prior).size == 1
    g = L.Graph(ip, ix, n)
    for pset in sorted(PARAM_SETS):
        kw = dict(BASE, **PARAM_SETS[pset])
        assert_same(L.decim_decode_batch(g, synd, prior, **kw), DM.decim_decode(ip, ix, n, synd, prior, **kw), f"bb72 {pset}")
    kw = dict(BASE, t_round=2, max_rounds=2, per_round=8)                    # the setting of the CPU tie test: ties across the cut
    assert_same(L.decim_decode_batch(g, synd, prior, **kw), DM.decim_decode(ip, ix, n, synd, prior, **kw), "bb72 ties")


def test_running_out_of_columns_steane(L, golden):
    g0 = golden("steane_minsum")
    ip, ix, n = g0["indptr"], g0["indices"], int(g0["n"])
    g = L.Graph(ip, ix, n)
    prior = np.full(n, 100.0)
    synd = np.array([[1, 0, 0], [0, 0, 0]], np.int8)
    kw = dict(alpha=1.0, clip_llr=20.0, t_round=1, max_rounds=3, per_round=4, fix_llr=1000.0)
    got = L.decim_decode_batch(g, synd, prior, **kw)
    assert_same(got, DM.decim_decode(ip, ix, n, synd, prior, **kw), "steane")
    assert (int(got[5][0]), int(got[2][0]), int(got[4][0])) == (7, 0, 3)
    for prior in (g0["prior"], g0["prior2"]):
        kw = dict(alpha=0.75, clip_llr=20.0, t_round=2, max_rounds=7, per_round=4, fix_llr=35.0)
        assert_same(L.decim_decode_batch(g, g0["syndromes"], prior, **kw), DM.decim_decode(ip, ix, n, g0["syndromes"], prior, **kw), "steane golden")


def test_no_rounds_is_relay_without_memory_circ144(L):
    c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, "circ144")
    (spz, _), (spx, _) = sampled(L, "circ144", 8)
    for sec, (g, prior, synd) in enumerate(((graphs[0], priors[0], spz), (graphs[1], priors[1], spx))):
        err, llr, conv, iters, rounds, fixed = L.decim_decode_batch(g, synd, prior, alpha=0.875, clip_llr=20.0, t_round=30, max_rounds=0, per_round=8,
                                                                    fix_llr=50.0)
        rerr, rconv, rlegs, riters, _ = L.relay_decode_batch(g, synd, prior, 5, 0, sec, alpha=0.875, gamma0=0.0, t0=30, max_legs=0, stop_after=1)
        assert err.tobytes() == rerr.tobytes() and conv.tobytes() == rconv.tobytes() and iters.tobytes() == riters.tobytes()
        assert (rounds == 1).all() and (fixed == 0).all() and np.array_equal(err, (llr < 0.0).astype(np.int8))


def test_slab_form_circ288(L):
    from qldpc_amd.data import load_circuit_matrices
    from qldpc_amd.simulation.engine import prior_llrs
    d = load_circuit_matrices("circ288")
    ip, ix, n = d["HdecZ_indptr"], d["HdecZ_indices"], int(d["HdecZ_shape"][1])
    m = len(ip) - 1
    assert n * 8 + 24 * m > 160 * 1024                                     # V does not fit LDS: the HBM/L2 form runs
    g = L.Graph(ip, ix, n)
    prior = prior_llrs(np.asarray(d["channel_probsZ"], dtype=np.float64))
    E = (np.random.default_rng(3).random((2, n)) < 0.0015).astype(np.int8)
    synd = L.gf2_spmv_batch(g, E)
    kw = dict(BASE, t_round=3, max_rounds=2, per_round=8)
    ref = DM.decim_decode(ip, ix, n, synd, prior, **kw)
    assert_same(L.decim_decode_batch(g, synd, prior, **kw), ref, "circ288")
    assert ref[5].max() == 16


def _dev_call(L, g, ds, dp, B, kw, stream):
    dev = ds.device
    out = (torch.zeros((B, g.n), dtype=torch.int8, device=dev), torch.zeros((B, g.n), dtype=torch.float64, device=dev),
           torch.zeros(B, dtype=torch.uint8, device=dev)) + tuple(torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(3))
    L.check(L.lib().qldpc_decim_decode_batch_dev(g.handle, B, ds.data_ptr(), dp.data_ptr(), kw["alpha"], kw["clip_llr"], kw["t_round"], kw["max_rounds"],
                                                 kw["per_round"], kw["fix_llr"], *[t.data_ptr() for t in out], C.c_void_p(stream)))
    return out


def test_splits_and_device_entry(L):
    c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, "circ72")
    _, (spx, _) = sampled(L, "circ72", 96, seed=5)
    g, prior = graphs[1], priors[1]
    kw = dict(BASE, t_round=5, max_rounds=8, per_round=12)
    whole = L.decim_decode_batch(g, spx, prior, **kw)
    assert whole[4].max() > 1
    a, b, one = L.decim_decode_batch(g, spx[:37], prior, **kw), L.decim_decode_batch(g, spx[37:], prior, **kw), L.decim_decode_batch(g, spx[50:51], prior, **kw)
    assert_same([np.concatenate([x, y]) for x, y in zip(a, b)], whole, "split")
    assert_same(one, [w[50:51] for w in whole], "one shot")
    assert_same([w[::-1] for w in L.decim_decode_batch(g, spx[::-1], prior, **kw)], whole, "reversed order")
    dev = torch.device("cuda:0")
    ds, dp = torch.from_numpy(np.ascontiguousarray(spx)).to(dev), torch.from_numpy(prior).to(dev)
    out = _dev_call(L, g, ds, dp, spx.shape[0], kw, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert_same([t.cpu().numpy() for t in out], whole, "device entry")


def test_concurrent_streams_on_one_graph(L):
    import threading
    c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, "circ72")
    (spz, _), _ = sampled(L, "circ72", 128, seed=41)
    g, prior = graphs[0], priors[0]
    kw = dict(BASE, t_round=5, max_rounds=8, per_round=12)
    alone_d = L.decim_decode_batch(g, spz, prior, **kw)
    alone_b = L.minsum_decode_batch(g, spz, prior, 50, "dynamical", 1.0)
    out = {}

    def decim():
        out["d"] = L.decim_decode_batch(g, spz, prior, **kw)

    def bp():
        out["b"] = L.minsum_decode_batch(g, spz, prior, 50, "dynamical", 1.0)
    for _ in range(3):
        ts = [threading.Thread(target=decim), threading.Thread(target=bp)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert_same(out["d"], alone_d, "host threads")
        for a, b in zip(out["b"], alone_b):
            assert np.array_equal(a, b, equal_nan=True)
    # device entry points on two torch streams
    dev = torch.device("cuda:0")
    B, n = spz.shape[0], g.n
    ds, dp = torch.from_numpy(np.ascontiguousarray(spz)).to(dev), torch.from_numpy(prior).to(dev)
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    be, bl, bc, bi = (torch.zeros((B, n), dtype=torch.int8, device=dev), torch.zeros((B, n), dtype=torch.float64, device=dev),
                      torch.zeros(B, dtype=torch.uint8, device=dev), torch.zeros(B, dtype=torch.int32, device=dev))
    torch.cuda.synchronize(dev)
    one = np.zeros(1)
    d1 = _dev_call(L, g, ds, dp, B, kw, s1.cuda_stream)
    L.check(L.lib().qldpc_minsum_decode_batch_dev(g.handle, B, ds.data_ptr(), dp.data_ptr(), 50, L.ALPHA_DYNAMIC, 1.0, L.ptr(one, C.c_double), 1, 1.0,
                                                  20.0, 0, be.data_ptr(), bl.data_ptr(), bc.data_ptr(), bi.data_ptr(), C.c_void_p(s2.cuda_stream)))
    d2 = _dev_call(L, g, ds, dp, B, kw, s2.cuda_stream)
    torch.cuda.synchronize(dev)
    assert_same([t.cpu().numpy() for t in d1], alone_d, "stream 1")
    assert_same([t.cpu().numpy() for t in d2], alone_d, "stream 2")
    assert np.array_equal(alone_b[0], be.cpu().numpy()) and np.array_equal(alone_b[1], bc.cpu().numpy())


def _pieces(L, setup, seed, count, cs_order, params):
    """plan sampler -> qldpc_decim_decode_batch -> the existing OSD-0 (or OSD-CS) call on the unconverged -> logical comparison"""
    c, compiled, Mx, graphs, priors, masks, plan = setup
    p = plan(batch=count)
    spz, tz, spx, tx = p.sample(seed, 0, count)
    p.close()
    verdict = np.zeros(count, np.uint8)
    out = dict(conv=[], osd=[], unsat=[], iters=[], rounds=[])
    for sec, (g, prior, mask, synd, true) in enumerate(((graphs[0], priors[0], masks[0], spz, tz), (graphs[1], priors[1], masks[1], spx, tx))):
        det, llr, conv, iters, rounds, fixed = L.decim_decode_batch(g, synd, prior, clip_llr=20.0, **params)
        bad = np.flatnonzero(conv == 0)
        if bad.size:
            if cs_order is None:
                det[bad] = L.osd0_batch(g, synd[bad], llr[bad], det[bad])
            else:
                det[bad] = L.osdcs_batch(g, synd[bad], llr[bad], det[bad], prior, cs_order)[0]
        k = true.shape[1]
        rows = np.stack([(mask >> np.uint64(r)) & np.uint64(1) for r in range(k)]).astype(np.int64)
        dd = (det.astype(np.int64) @ rows.T) % 2
        verdict |= (np.any(dd != true.astype(np.int64), axis=1).astype(np.uint8) << sec)
        out["conv"].append(int(conv.sum())); out["osd"].append(int(bad.size)); out["iters"].append(int(iters.astype(np.int64).sum()))
        out["rounds"].append(int(rounds.astype(np.int64).sum()))
        out["unsat"].append(int((L.gf2_spmv_batch(g, det) != (synd & 1)).any(axis=1).sum()))
    return verdict, out


@pytest.mark.parametrize("cs_order", [None, 6])
def test_circuit_plan_matches_the_pieces(L, cs_order):
    count, seed = 256, 4321
    setup = circuit_setup(L, "circ72")
    verdict, h = _pieces(L, setup, seed, count, cs_order, PLAN)
    p = setup[6](batch=128)                                                # two batches
    if cs_order is not None:
        p.use_osd_cs(cs_order)
    p.use_decimation(**PLAN)
    got = p.run_outcomes(seed, 0, count)
    tally = p.read(clear=True)
    ph, _ = p.phase_times()
    p.close()
    T = L.TALLY
    print(cs_order, "tally", tally.tolist(), "pieces", h)
    assert np.array_equal(got, verdict)
    assert tally[T["trials"]] == count and tally[T["total_err"]] == np.count_nonzero(verdict)
    assert tally[T["z_err"]] == np.count_nonzero(verdict & 1) and tally[T["x_err"]] == np.count_nonzero(verdict & 2)
    assert [tally[T["bp_conv_z"]], tally[T["bp_conv_x"]]] == h["conv"]
    assert [tally[T["osd_z"]], tally[T["osd_x"]]] == h["osd"]
    assert [tally[T["iters_z"]], tally[T["iters_x"]]] == h["iters"]
    assert [tally[T["unsat_z"]], tally[T["unsat_x"]]] == h["unsat"]
    assert [tally[T["legs_z"]], tally[T["legs_x"]]] == h["rounds"]         # slots 14 / 15: the summed rounds
    assert h["rounds"][0] > count and h["osd"][0] + h["osd"][1] > 0        # decimation ran, and so did the OSD stage
    assert ph["bp_z"] > 0 and ph["bp_x"] > 0 and ph["osd_z"] > 0


def test_plan_switch_rules(L):
    plan = circuit_setup(L, "circ72")[6]
    for first, name in ((lambda p: p.use_relay(), "Relay-BP"), (lambda p: p.use_window(4, 2), "sliding-window"), (lambda p: p.use_layered(), "layered")):
        p = plan(batch=256)
        first(p)
        with pytest.raises(L.QldpcError, match=f"(?s){name}.*guided decimation"):          # ... then decimation is refused, both sides named
            p.use_decimation(**PLAN)
        p.close()
    for then, name in ((lambda p: p.use_relay(), "Relay-BP"), (lambda p: p.use_window(4, 2), "sliding-window"), (lambda p: p.use_layered(), "layered")):
        p = plan(batch=256)
        p.use_decimation(**PLAN)
        with pytest.raises(L.QldpcError, match=f"(?s)guided decimation.*{name}"):          # ... and the other way round
            then(p)
        p.use_osd_cs(5)                                                    # the OSD stage is independent of the BP stage
        p.use_decimation(**dict(PLAN, per_round=4))                        # new arguments replace the old ones
        p.run(1, 0, 64)
        assert p.read()[L.TALLY["trials"]] == 64
        p.close()
    p = plan(batch=256, damping=0.5)
    with pytest.raises(L.QldpcError, match="damping"):
        p.use_decimation(**PLAN)
    with pytest.raises(ValueError):
        p.use_decimation(**dict(PLAN, per_round=0))
    with pytest.raises(ValueError):
        p.use_decimation(clip_llr=5.0)
    assert L.lib().qldpc_circuit_plan_use_decimation(p._h, 1.0, 0, 2, 8, 50.0) == -1
    p.close()
    p = plan(batch=256, use_osd=False)                                     # BP alone
    p.use_decimation(**PLAN)
    p.run(1, 0, 64)
    t = p.read()
    assert t[L.TALLY["trials"]] == 64 and t[L.TALLY["osd_z"]] == 0 and t[L.TALLY["legs_z"]] >= 64
    p.close()


def test_run_simulation_decimation(L):
    from qldpc_amd.data import load_code, load_precomputed_matrices
    from qldpc_amd.simulation.engine import run_simulation
    c = load_code("bb72")
    kw = dict(num_cycles=6, precomputed_matrices=load_precomputed_matrices("circ72"), base_seed=2028, batch=512, **_bb_params(c))
    args = (c["Hx"], c["Hz"], c["Lx"], c["Lz"], 0.005)
    r1 = run_simulation(*args, num_trials=1500, devices=[0], decimation=PLAN, **kw)
    r2 = run_simulation(*args, num_trials=1500, num_workers=2, devices=[0, 0], decimation=PLAN, **kw)
    assert r1["tally"][L.TALLY["trials"]] == 1500 and np.array_equal(r1["tally"], r2["tally"])        # reproducible, whatever the workers
    assert r2["num_workers"] == 2 and r1["decimation"] == PLAN
    assert r1["mean_rounds_z"] == r1["tally"][L.TALLY["legs_z"]] / 1500 and r1["mean_rounds_z"] >= 1.0 and r1["mean_rounds_x"] >= 1.0
    p = circuit_setup(L, "circ72")[6](batch=512)
    p.use_decimation(**PLAN)
    p.run(2028, 0, 1500)
    assert np.array_equal(p.read(), r1["tally"])                           # ... and equal to the plan run
    p.close()
    r3 = run_simulation(*args, num_trials=700, devices=[0], decimation=PLAN, decoder="bp_osd_cs", osd_order=5, **kw)
    assert r3["decoder"] == "bp_osd_cs" and r3["decimation"] == PLAN and r3["tally"][L.TALLY["trials"]] == 700
    r0 = run_simulation(*args, num_trials=700, devices=[0], **kw)
    assert "decimation" not in r0 and "mean_rounds_z" not in r0 and r0["tally"][L.TALLY["legs_z"]] == 0


def test_nothing_existing_changes(L):
    """an unswitched plan's tally for a fixed seed is the same before and after a different plan on the same graphs was switched to decimation"""
    c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, "circ72")
    before = plan(batch=512)
    before.run(2024, 0, 2000)
    t_before = before.read(clear=True)
    before.close()
    switched = plan(batch=512)
    switched.use_decimation(**PLAN)
    switched.run(2024, 0, 1000)
    t_sw = switched.read(clear=True)
    after = plan(batch=512)
    after.run(2024, 0, 2000)
    t_after = after.read(clear=True)
    after.close()
    switched.close()
    T = L.TALLY
    assert np.array_equal(t_before, t_after)
    assert t_before[T["legs_z"]] == 0 and t_before[T["legs_x"]] == 0 and t_sw[T["legs_z"]] >= 1000
    assert t_before[T["osd_z"]] + t_before[T["osd_x"]] > 0
