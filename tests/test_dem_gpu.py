"""Detector error models on the MI355X: the sampler against the numpy model bit for bit (T1), the fused pipeline against its parts trial by trial
(T2), one-sector plans (T3), every decoder switch on a DEM plan against the batch decoder it stands for (T4), creation errors (T5) and
run_dem_simulation (T6)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dem_model as DM  # noqa: E402

pytestmark = pytest.mark.gpu

RELAY = dict(t0=20, tr=10, max_legs=6)
DECIM = dict(alpha=0.9, t_round=10, max_rounds=6, per_round=8)


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


@pytest.fixture(scope="module")
def DEM():
    from qldpc_amd.simulation.dem import DetectorErrorModel
    return DetectorErrorModel


_MODELS = {}


def model(L, DEM, name):
    """(dem, graphs) of "tiny", "circ72" (layer_rows 36) and their sector-0 halves "tiny_z", "circ72_z"; built once."""
    if name not in _MODELS:
        if name.endswith("_z"):
            dem = model(L, DEM, name[:-2])[0].sector(0)
        else:
            dem = DM.tiny_dem(DEM) if name == "tiny" else DEM.from_decoding_matrices("circ72", layer_rows=36)
        views = [dem.decoder_view(s) for s in range(dem.n_sectors)]
        _MODELS[name] = (dem, [L.Graph(v.indptr, v.indices, v.shape[1]) for v in views])
    return _MODELS[name]


def logical_errors(det, mask, true):
    k = true.shape[1]
    rows = np.stack([(mask >> np.uint64(r)) & np.uint64(1) for r in range(k)]).astype(np.int64) if k else np.zeros((0, det.shape[1]), np.int64)
    return np.any((det.astype(np.int64) @ rows.T) % 2 != true.astype(np.int64), axis=1)


def parts(L, dem, graphs, plan, seed, begin, count, max_iter, decode=None):
    """plan.sample -> a batch decoder per sector (default: minsum_decode_batch -> osd0_batch on the non-converged) -> logical masks against the truth
    -> (verdicts, hand-built tally).  decode(sector, graph, view, syndromes) -> (det, conv, iters + 1 summed, osd calls)."""
    sampled = plan.sample(seed, begin, count)
    T = L.TALLY
    tally, verdict = np.zeros(L.TALLY_SLOTS, np.int64), np.zeros(count, np.uint8)
    tally[T["trials"]] = count
    for s in range(dem.n_sectors):
        g, v, synd, true = graphs[s], dem.decoder_view(s), sampled[2 * s], sampled[2 * s + 1]
        if decode is None:
            det, conv, llr, iters = L.minsum_decode_batch(g, synd, v.prior, max_iter, "dynamical", 1.0)
            bad = np.flatnonzero(conv == 0)
            if bad.size:
                det[bad] = L.osd0_batch(g, synd[bad], llr[bad], det[bad])
            it, osd = int((iters.astype(np.int64) + 1).sum()), int(bad.size)
        else:
            det, conv, it, osd = decode(s, g, v, synd)
        err = logical_errors(det, v.logmask, true)
        verdict |= err.astype(np.uint8) << s
        sfx = "zx"[s]
        tally[T[sfx + "_err"]], tally[T["bp_conv_" + sfx]], tally[T["osd_" + sfx]], tally[T["iters_" + sfx]] = err.sum(), (conv != 0).sum(), osd, it
        tally[T["zero_synd_" + sfx]] = (~synd.any(axis=1)).sum()
        tally[T["unsat_" + sfx]] = (L.gf2_spmv_batch(g, det) != (synd & 1)).any(axis=1).sum()
    tally[T["total_err"]] = np.count_nonzero(verdict)
    return verdict, tally


def assert_tally(L, got, want, slots=None):
    names = sorted(L.TALLY, key=L.TALLY.get)
    diff = {n: (int(got[i]), int(want[i])) for i, n in enumerate(names) if got[i] != want[i] and (slots is None or n in slots)}
    assert not diff, f"tally slots (plan, parts): {diff}"


# ---- T1 ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [20260301, (0x9E3779B9 << 32) | 17])
def test_t1_sampler_is_the_model(L, DEM, seed):
    dem, graphs = model(L, DEM, "tiny")
    begin, count = (1 << 32) - 100, 4096                       # crosses the 32-bit counter word
    plan = dem.plan(graphs, batch=1024)                        # four batches of 1024 workgroups, a trial each (a second trial per workgroup: test_dem_shapes_gpu.py, stride)
    got = plan.sample(seed, begin, count)
    plan.close()
    want = DM.sample(dem, seed, begin, count)
    for s in range(2):
        assert got[2 * s].shape == want[s][0].shape and got[2 * s + 1].shape == want[s][1].shape
        bad = np.flatnonzero((got[2 * s] != want[s][0]).any(axis=1) | (got[2 * s + 1] != want[s][1]).any(axis=1))
        assert bad.size == 0, f"sector {s}: trials {bad[:8].tolist()} differ from the model ({bad.size} of {count})"
    assert want[0][1][:, 63].any() and want[0][0][:, 36].any() and want[1][0].any()      # bit 63, the highest detector and sector 1 are exercised
    other = dem.plan(graphs, batch=4096)                       # another batch size, another grid: the same draws
    again = other.sample(seed, begin, count)
    other.close()
    assert all(np.array_equal(a, b) for a, b in zip(got, again))


# ---- T2 / T3 ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, count, max_iter", [("tiny", 4096, 12), ("circ72", 512, 12), ("tiny_z", 4096, 12), ("circ72_z", 512, 12)])
def test_t2_t3_pipeline_is_its_parts(L, DEM, name, count, max_iter):
    dem, graphs = model(L, DEM, name)
    seed, T = 424242, L.TALLY
    plan = dem.plan(graphs, max_iter=max_iter, batch=128)
    verdict, want = parts(L, dem, graphs, plan, seed, 0, count, max_iter)
    got = plan.run_outcomes(seed, 0, count)
    tally = plan.read(clear=True)
    bad = np.flatnonzero(got != verdict)
    assert bad.size == 0, f"{name}: verdicts of trials {bad[:8].tolist()} differ ({bad.size} of {count})"
    assert_tally(L, tally, want)
    print(f"{name}: tally {tally.tolist()}")
    assert want[T["z_err"]] > 0                                # the logical comparison had something to find ...
    assert want[T["osd_z"]] > 0 or not name.startswith("circ72")      # ... and on circ72 the OSD stage something to do (12 iterations leave BP failures)
    cut = 200 * count // 512                                   # two calls, cut inside a batch: the same tally
    a = plan.run_outcomes(seed, 0, cut)
    b = plan.run_outcomes(seed, cut, count - cut)
    assert np.array_equal(np.concatenate([a, b]), verdict)
    assert np.array_equal(plan.read(clear=True), tally)
    plan.run(seed, 0, count)                                   # and without the verdicts
    assert np.array_equal(plan.read(clear=True), tally)
    if dem.n_sectors == 1:                                     # T3: sector 1 does not exist
        spz, tz, spx, tx = plan.sample(seed, 0, 64)
        assert spx.size == 0 and not tx.any() and spz.any()
        assert not (got & 2).any()
        assert all(tally[T[k + "_x"]] == 0 for k in ("bp_conv", "osd", "iters", "zero_synd", "unsat", "legs")) and tally[T["x_err"]] == 0
        assert tally[T["total_err"]] == tally[T["z_err"]]
        ph, nb = plan.phase_times()
        assert ph["bp_x"] == 0 and ph["osd_x"] == 0 and ph["bp_z"] > 0 and ph["sample"] > 0
        two, two_graphs = model(L, DEM, name[:-2])             # the Z half draws what the two-sector model draws in sector 0
        p2 = two.plan(two_graphs, max_iter=max_iter, batch=128)
        assert np.array_equal(p2.run_outcomes(seed, 0, count) & 1, got)
        p2.close()
    plan.close()


# ---- T4 -----------------------------------------------------------------------------------------------------------------------------------------------
def _bp_then_osd(L, bp, cs_order=None):
    """decode() of `parts` from a BP-stage decoder: bp(sector, graph, view, syndromes) -> (det, conv, llr, iterations per trial)"""
    def decode(s, g, v, synd):
        det, conv, llr, its = bp(s, g, v, synd)
        det = det.copy()
        bad = np.flatnonzero(conv == 0)
        if bad.size:
            det[bad] = L.osd0_batch(g, synd[bad], llr[bad], det[bad]) if cs_order is None else L.osdcs_batch(g, synd[bad], llr[bad], det[bad], v.prior, cs_order)[0]
        return det, conv, int(its.astype(np.int64).sum()), int(bad.size)
    return decode


def _switches(L, seed, begin, max_iter):
    from qldpc_amd.decoding.decimation import DecimationDecoder
    from qldpc_amd.decoding.layered import LayeredMinSumDecoder
    from qldpc_amd.decoding.single import SingleMinSumDecoder
    from qldpc_amd.decoding.window import SlidingWindowDecoder
    H = lambda g: (g.indptr, g.indices, g.n)      # noqa: E731

    def minsum(s, g, v, synd):
        det, conv, llr, it = L.minsum_decode_batch(g, synd, v.prior, max_iter, "dynamical", 1.0)
        return det, conv, llr, it + 1

    def relay(s, g, v, synd):                     # the run's seed, the global trial index as the shot, the sector as the tag; no OSD stage
        err, conv, legs, iters, _ = L.relay_decode_batch(g, synd, v.prior, seed, begin, s, **RELAY)
        return err, conv, int(iters.astype(np.int64).sum()), 0

    def layered(s, g, v, synd):
        det, conv, llr, it = LayeredMinSumDecoder(H(g), v.prior, maxIter=max_iter).decode(synd)
        return det, conv, llr, it + 1

    def decim(s, g, v, synd):
        det, llr, conv, iters, rounds, fixed = DecimationDecoder(H(g), v.prior, clip_llr=20.0, **DECIM).decode(synd)
        return det, conv, llr, iters

    def single(s, g, v, synd):
        det, conv, llr, it = SingleMinSumDecoder(H(g), v.prior, max_iter=max_iter).decode(synd)
        return det, conv, llr, it + 1

    def window(s, g, v, synd):
        err, info = SlidingWindowDecoder(H(g), v.prior, 36, 3, 1, max_iter=max_iter).decode(synd)
        return err, (info["conv"] == info["windows"]).astype(np.uint8), int(info["iters"].astype(np.int64).sum()), int((info["osd"] > 0).sum())

    return {"relay": (lambda p: p.use_relay(**RELAY), relay),
            "osd_cs": (lambda p: p.use_osd_cs(4), _bp_then_osd(L, minsum, cs_order=4)),
            "layered": (lambda p: p.use_layered(), _bp_then_osd(L, layered)),
            "decimation": (lambda p: p.use_decimation(**DECIM), _bp_then_osd(L, decim)),
            "f32": (lambda p: p.use_f32(), _bp_then_osd(L, single)),
            "window": (lambda p: p.use_window(3, 1), window)}


@pytest.mark.parametrize("name", ["circ72", "circ72_z"])
@pytest.mark.parametrize("switch", ["relay", "osd_cs", "layered", "decimation", "f32", "window"])
def test_t4_switches_ride_along(L, DEM, name, switch):
    dem, graphs = model(L, DEM, name)
    seed, begin, count, max_iter = 777, 1000, 128, 12
    use, decode = _switches(L, seed, begin, max_iter)[switch]
    plan = dem.plan(graphs, max_iter=max_iter, batch=128)
    use(plan)
    verdict, want = parts(L, dem, graphs, plan, seed, begin, count, max_iter, decode)
    got = plan.run_outcomes(seed, begin, count)
    tally = plan.read(clear=True)
    plan.close()
    bad = np.flatnonzero(got != verdict)
    assert bad.size == 0, f"{name} {switch}: verdicts of trials {bad[:8].tolist()} differ ({bad.size} of {count})"
    assert_tally(L, tally, want, slots=set(L.TALLY) - {"legs_z", "legs_x"})      # (legs / rounds: below)
    if dem.n_sectors == 1:
        assert not (got & 2).any() and tally[L.TALLY["legs_x"]] == 0 and tally[L.TALLY["iters_x"]] == 0
    if switch in ("relay", "decimation"):
        assert tally[L.TALLY["legs_z"]] >= count


def test_t4_window_needs_layer_rows(L, DEM):
    dem, graphs = model(L, DEM, "circ72")
    for lr in (0, 35):                                          # none given; not a divisor of 288
        d = DEM.from_decoding_matrices("circ72", layer_rows=lr)
        plan = d.plan(graphs, batch=64)
        assert L.lib().qldpc_circuit_plan_use_window(plan._h, 3, 1) == -1
        assert b"layer_rows" in L.lib().qldpc_last_error() and b"sector 0" in L.lib().qldpc_last_error()
        with pytest.raises(L.QldpcError, match="layer_rows"):
            plan.use_window(3, 1)
        plan.run(1, 0, 64)                                      # the plan is still what it was
        assert plan.read()[L.TALLY["trials"]] == 64
        plan.close()


# ---- T5 -----------------------------------------------------------------------------------------------------------------------------------------------
def _create(L, dem, graphs, mutate=None, nsec=None, drop_g1=False, flags=0, logmask0=None):
    """raw qldpc_circuit_plan_create_dem on (a mutated copy of) the model's tables -> (rc, error text, handle)"""
    views = [dem.decoder_view(s) for s in range(dem.n_sectors)]
    sectors = [list(S) for S in dem.sectors]
    prob = dem.prob.copy()
    for S in sectors:
        S[3], S[4], S[5] = S[3].copy(), S[4].copy(), S[5].copy()
    if mutate:
        mutate(prob, sectors)
    d, keep = L.make_dem_desc(prob, [tuple(S) for S in sectors])
    if nsec is not None:
        d.n_sectors = nsec
    pri = [np.ascontiguousarray(v.prior) for v in views] + [None]
    lms = [np.ascontiguousarray(v.logmask if logmask0 is None or s else logmask0, np.uint64) for s, v in enumerate(views)] + [None]
    g = list(graphs) + [None]
    if drop_g1:
        g[1] = None
    one = np.zeros(1)
    opt = lambda a, t: L.ptr(a, t) if a is not None else None      # noqa: E731
    h = C.c_void_p()
    rc = L.lib().qldpc_circuit_plan_create_dem(C.byref(d), g[0].handle, g[1].handle if g[1] is not None else None, opt(pri[0], C.c_double),
                                               opt(pri[1], C.c_double), opt(lms[0], C.c_uint64), opt(lms[1], C.c_uint64), 12, L.ALPHA_DYNAMIC, 1.0, 1.0,
                                               L.ptr(one, C.c_double), 1, L.ptr(one, C.c_double), 1, 1.0, 20.0, 1, flags, 256, C.byref(h))
    return rc, (L.lib().qldpc_last_error() or b"").decode(), h


def test_t5_creation_errors(L, DEM):
    dem, graphs = model(L, DEM, "tiny")

    def setter(sector, field, index, value):
        def f(prob, sectors):
            if field == "prob":
                prob[index] = value
            else:
                sectors[sector][field][index] = value
        return f

    def null_table(prob, sectors):
        sectors[1][4] = None

    l5 = int(dem.sectors[0].det_ptr[5])                          # mechanism 5 = ([36], bit 63) in sector 0
    l4 = int(dem.sectors[1].det_ptr[4])                          # mechanism 4 = ([1, 4], 4) in sector 1
    cases = [(dict(mutate=setter(0, "prob", 9, 1.0)), "mechanism 9"), (dict(mutate=setter(0, "prob", 11, -0.25)), "mechanism 11"),
             (dict(mutate=setter(0, "prob", 36, float("nan"))), "mechanism 36"),
             (dict(mutate=setter(0, 3, 8, int(dem.sectors[0].det_ptr[7]) - 1)), "sector 0, mechanism 7"),            # det_ptr goes down
             (dict(mutate=setter(0, 4, l5, 37)), "sector 0, mechanism 5"),                                          # detector 37 of 37
             (dict(mutate=setter(1, 4, l4 + 1, 1)), "sector 1, mechanism 4"),                                       # [1, 1]: not ascending
             (dict(mutate=setter(1, 5, 4, 8)), "sector 1, mechanism 4"),                                            # bit 3 with k = 3
             (dict(nsec=0), "n_sectors"), (dict(nsec=3), "n_sectors"),
             (dict(drop_g1=True), "sector 1"),                                                                      # two sectors, one graph
             (dict(logmask0=np.full(graphs[0].n, 1, np.uint64)), None)]                                             # (a valid decoder mask: control)
    for kw, needle in cases:
        rc, text, h = _create(L, dem, graphs, **kw)
        if needle is None:
            assert rc == 0 and h.value
            L.lib().qldpc_circuit_plan_destroy(h)
            continue
        assert rc == -1 and not h.value, (kw, rc, text)          # QLDPC_ERR_INVALID, and no plan came back (nothing to leak)
        assert needle in text, (needle, text)
    # NULL table: make_dem_desc cannot build it, so clear the pointer afterwards
    views = [dem.decoder_view(s) for s in range(2)]
    d, keep = L.make_dem_desc(dem.prob, [tuple(S) for S in dem.sectors])
    d.det_idx[1] = C.POINTER(C.c_uint16)()
    one, h = np.zeros(1), C.c_void_p()
    rc = L.lib().qldpc_circuit_plan_create_dem(C.byref(d), graphs[0].handle, graphs[1].handle, L.ptr(views[0].prior, C.c_double), L.ptr(views[1].prior, C.c_double),
                                               L.ptr(views[0].logmask, C.c_uint64), L.ptr(views[1].logmask, C.c_uint64), 12, L.ALPHA_DYNAMIC, 1.0, 1.0,
                                               L.ptr(one, C.c_double), 1, L.ptr(one, C.c_double), 1, 1.0, 20.0, 1, 0, 256, C.byref(h))
    assert rc == -1 and not h.value and b"sector 1" in L.lib().qldpc_last_error() and b"NULL" in L.lib().qldpc_last_error()
    # g_s->m != n_det[s]: sector 1's graph handed to sector 0
    with pytest.raises(L.QldpcError, match="sector 0.*5 rows.*37 detectors"):
        dem.plan([graphs[1], graphs[1]])
    # a decoder-side logical mask beyond k (sector 1 has k = 3)
    with pytest.raises(L.QldpcError, match="sector 1.*column 2"):
        lm = views[1].logmask.copy()
        lm[2] = 8
        L.DemPlan(dem.prob, [tuple(S) for S in dem.sectors], graphs, [v.prior for v in views], [views[0].logmask, lm])
    # one sector with a second graph
    with pytest.raises(L.QldpcError, match="one sector"):
        z = dem.sector(0)
        d1, keep1 = L.make_dem_desc(z.prob, [tuple(z.sectors[0])])
        L.check(L.lib().qldpc_circuit_plan_create_dem(C.byref(d1), graphs[0].handle, graphs[1].handle, L.ptr(views[0].prior, C.c_double), None,
                                                      L.ptr(views[0].logmask, C.c_uint64), None, 12, L.ALPHA_DYNAMIC, 1.0, 1.0, L.ptr(one, C.c_double), 1,
                                                      L.ptr(one, C.c_double), 1, 1.0, 20.0, 1, 0, 256, C.byref(h)))


def test_t5_count_zero_and_clock_probe(L, DEM):
    dem, graphs = model(L, DEM, "tiny")
    plan = dem.plan(graphs, batch=64, flags=L.FLAG_CLOCK_PROBE)
    plan.run(3, 0, 0)
    assert plan.run_outcomes(3, 5, 0).size == 0
    assert not plan.read().any()
    assert all(x.shape[0] == 0 for x in plan.sample(3, 0, 0))
    plan.run(3, 0, 64)
    mhz = plan.clock()                                          # QLDPC_FLAG_CLOCK_PROBE keeps working on a DEM plan
    assert len(mhz) == 2 and all(np.isfinite(v) and v >= 0 for v in mhz)
    plan.close()
    plain = dem.plan(graphs, batch=64)
    with pytest.raises(L.QldpcError, match="CLOCK_PROBE"):
        plain.clock()
    plain.close()


# ---- T6 -----------------------------------------------------------------------------------------------------------------------------------------------
def test_t6_run_dem_simulation(L, DEM):
    from qldpc_amd.simulation.dem import run_dem_simulation
    dem, graphs = model(L, DEM, "circ72")
    seed, count, T = 2030, 2048, L.TALLY
    plan = dem.plan(graphs, max_iter=12, batch=512)
    verdict, want = parts(L, dem, graphs, plan, seed, 0, count, 12)
    r1 = run_dem_simulation(dem, num_trials=count, maxIter=12, base_seed=seed, batch=512, devices=[0])
    assert_tally(L, r1["tally"], want)
    assert r1["num_trials"] == count and r1["logical_errors"] == np.count_nonzero(verdict) and r1["num_workers"] == 1
    assert r1["z_logical_error_rate"] == np.count_nonzero(verdict & 1) / count and r1["x_logical_error_rate"] == np.count_nonzero(verdict & 2) / count
    assert r1["logical_error_rate"] == np.count_nonzero(verdict) / count and r1["precision"] == "f64"
    # the in-order early stop: exactly the trial a host-side prefix cut of run_outcomes gives
    out = plan.run_outcomes(seed, 0, count)
    plan.close()
    assert np.array_equal(out, verdict)
    stop = int(np.flatnonzero(np.cumsum(out != 0) == 5)[0]) + 1
    r2 = run_dem_simulation(dem, num_trials=count, maxIter=12, base_seed=seed, batch=512, devices=[0], target_logical_errors=5)
    assert r2["num_trials"] == stop and r2["logical_errors"] == 5
    assert r2["z_logical_error_rate"] == np.count_nonzero(out[:stop] & 1) / stop and r2["x_logical_error_rate"] == np.count_nonzero(out[:stop] & 2) / stop
    # two plans on one card give the one-plan result; more workers than GPUs are capped
    r3 = run_dem_simulation(dem, num_trials=count, maxIter=12, base_seed=seed, batch=512, devices=[0, 0])
    assert np.array_equal(r3["tally"], r1["tally"]) and r3["num_workers"] == 2 and r3["devices"] == [0, 0]
    r4 = run_dem_simulation(dem, num_trials=count, maxIter=12, base_seed=seed, batch=512, num_workers=8)
    assert r4["num_workers"] == min(8, L.device_count()) and np.array_equal(r4["tally"], r1["tally"])
    r5 = run_dem_simulation(dem, num_trials=count, maxIter=12, base_seed=seed, batch=512, devices=[0, 0], target_logical_errors=5)
    assert r5["num_trials"] == stop and r5["logical_errors"] == 5
    # one sector: the x keys are 0
    z, _ = model(L, DEM, "circ72_z")
    rz = run_dem_simulation(z, num_trials=count, maxIter=12, base_seed=seed, batch=512, devices=[0])
    assert rz["x_logical_error_rate"] == 0 and rz["z_logical_error_rate"] == r1["z_logical_error_rate"] == rz["logical_error_rate"]
    assert all(rz["tally"][T[k]] == 0 for k in T if k.endswith("_x") or k == "x_err")
    # an extension rides along, with its result keys
    rr = run_dem_simulation(dem, num_trials=256, maxIter=12, base_seed=seed, batch=128, devices=[0], decoder="relay_bp", relay_params=RELAY)
    assert rr["decoder"] == "relay_bp" and rr["mean_legs_z"] >= 1 and rr["num_trials"] == 256
    rw = run_dem_simulation(dem, num_trials=256, maxIter=12, base_seed=seed, batch=128, devices=[0], window=(3, 1))
    assert rw["window"] == (3, 1) and rw["num_trials"] == 256
