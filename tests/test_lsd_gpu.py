"""BP+LSD on the MI355X: the kernel equals tests/lsd_model.py bit for bit in solution and info on the seeded shots of tests/lsd_shapes.py (flag 1 / 2
shots: qldpc_osd0_batch's answer), the device entry point, concurrent streams, C-level refusals, the circuit plan switch and its counters,
run_simulation / DemDecoder, and the recorded circ144 cases against the reference's OSD-0 answers."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lsd_model as M  # noqa: E402
import lsd_shapes as LS  # noqa: E402
import osd_shapes as S  # noqa: E402
from test_relay_gpu import _bb_params, circuit_setup  # noqa: E402

pytestmark = pytest.mark.gpu

_GRAPHS = {}


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


def _graph(L, key):
    if key not in _GRAPHS:
        f, _ = LS.matrix(key)
        _GRAPHS[key] = L.Graph(f.indptr, f.indices, f.n)
    return _GRAPHS[key]


def _held(L, key, name, shots, bps, max_rows):
    """library == model on every shot: solution and info where the flag is 0, info and qldpc_osd0_batch's solution where it is not -> info"""
    g = _graph(L, key)
    want_sol, want_info, _ = LS.answers(key, name, shots, bps, max_rows)
    sol, info = L.lsd_batch(g, shots.synd, shots.llr, shots.hard, bps, max_rows)
    o0 = L.osd0_batch(g, shots.synd, shots.llr, shots.hard)
    for b in range(shots.synd.shape[0]):
        assert tuple(info[b]) == tuple(want_info[b]), f"{key}/{name} bits {bps} cap {max_rows} shot {b}: info {info[b]} vs model {want_info[b]}"
        want = want_sol[b] if want_info[b, 0] == 0 else o0[b]
        assert np.array_equal(sol[b], want), f"{key}/{name} bits {bps} cap {max_rows} shot {b} (flag {info[b, 0]}): solution differs"
    return info


def _raw(L, g, synd, llr, hard, bps, max_rows):
    synd = np.ascontiguousarray(synd, np.int8).reshape(-1, g.m)
    B = synd.shape[0]
    llr, hard = np.ascontiguousarray(llr, np.float64).reshape(B, g.n), np.ascontiguousarray(hard, np.int8).reshape(B, g.n)
    sol, info = np.zeros((max(B, 1), g.n), np.int8), np.zeros((max(B, 1), 4), np.int32)
    return L.lib().qldpc_lsd_batch(g.handle, B, L.ptr(synd, C.c_int8), L.ptr(llr, C.c_double), L.ptr(hard, C.c_int8), int(bps), int(max_rows),
                                   L.ptr(sol, C.c_int8), L.ptr(info, C.c_int32))


@pytest.mark.parametrize("bps", (1, 2, 64))
@pytest.mark.parametrize("key", sorted(LS.MATRICES))
def test_general_shots(L, key, bps):
    """sparse errors, zero residuals, random syndromes, NaN / infinite / tied |llr| on every matrix at bits_per_step 1, 2 and 64"""
    shots = LS.general(key)
    info = _held(L, key, "general", shots, bps, 128)
    zero = ~(shots.synd ^ np.stack([LS.matrix(key)[1].parity(h) for h in shots.hard])).any(axis=1)
    assert zero.sum() >= 3 and (info[zero] == 0).all()                       # zero residual: flag 0, no rounds, nothing added
    assert (info[:, 0] == 0).sum() > 12


@pytest.mark.parametrize("bps", (1, 2))
@pytest.mark.parametrize("name, key", (("single_seed", "ident"), ("merging", "dep"), ("apart", "ident"), ("duplicates", "doubled"), ("empty_rows", "tiny")))
def test_special_shots(L, name, key, bps):
    """a single seed; two clusters that merge and two that stay apart; twin columns; seeds on rows without columns (flag 2)"""
    info = _held(L, key, name, getattr(LS, name)(), bps, 128)
    if name == "empty_rows":
        assert (info[:, 0] == 2).all()


@pytest.mark.parametrize("max_rows", (1, 64, 65))
def test_row_caps(L, max_rows):
    """max_rows 1, 64 and 65 (the row-word boundary): shots the cap stops (by one row among them, tests/test_lsd_cpu.py names them) beside shots it does not"""
    info = np.concatenate([_held(L, "ident", "general", LS.general("ident"), 1, max_rows), _held(L, "ident", "single_seed", LS.single_seed(), 1, max_rows),
                           _held(L, "tiny", "empty_rows", LS.empty_rows(), 1, max_rows)])
    flags = np.bincount(info[:, 0], minlength=3)
    assert flags[0] > 0 and flags[1] > 0 and flags[2] > 0
    assert (info[:, 2] <= max_rows).all()


def test_big_batch(L):
    """600 shots: more than the workgroups of a launch, so the ticket counter hands every workgroup a second shot"""
    shots = LS.general("doubled")
    rep = S.BIG_BATCH // shots.synd.shape[0]
    big = LS._shots(np.tile(shots.synd, (rep, 1)), np.tile(shots.llr, (rep, 1)), np.tile(shots.hard, (rep, 1)))
    assert big.synd.shape[0] == S.BIG_BATCH
    want_sol, want_info, _ = LS.answers("doubled", "general", shots, 2, 128)
    g = _graph(L, "doubled")
    sol, info = L.lsd_batch(g, big.synd, big.llr, big.hard, 2, 128)
    o0 = L.osd0_batch(g, shots.synd, shots.llr, shots.hard)
    want = np.where((want_info[:, :1] == 0), want_sol, o0)
    assert np.array_equal(info, np.tile(want_info, (rep, 1)))
    assert np.array_equal(sol, np.tile(want, (rep, 1)))


def _dev_call(L, g, t, bps, max_rows, dsel, dcnt, dsol, dinfo, stream=0):
    ds, dl, dh = t
    return L.lib().qldpc_lsd_batch_dev(g.handle, ds.shape[0], C.c_void_p(ds.data_ptr()), C.c_void_p(dl.data_ptr()), C.c_void_p(dh.data_ptr()), bps, max_rows,
                                       C.c_void_p(dsel.data_ptr()) if dsel is not None else None, C.c_void_p(dcnt.data_ptr()) if dcnt is not None else None,
                                       C.c_void_p(dsol.data_ptr()), C.c_void_p(dinfo.data_ptr()), C.c_void_p(stream))


def test_dev_entry_select_list_and_alias(L):
    """device pointers, a select list, d_solution aliasing d_hard: listed shots solved in place, the others untouched"""
    shots = LS.general("dep")
    g = _graph(L, "dep")
    whole = L.lsd_batch(g, shots.synd, shots.llr, shots.hard, 1, 64)          # (flags 0, 1 and 2 among them)
    assert set(whole[1][:, 0]) == {0, 1, 2}
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)        # noqa: E731
    ds, dl, dh = t(shots.synd), t(shots.llr), t(shots.hard)
    B = shots.synd.shape[0]
    sel = np.array([5, 0, 3, 11, 19, 7, 2, 23], np.int32)
    dsel, dcnt = t(sel), t(np.array([sel.size], np.int32))
    dinfo = torch.full((B, 4), -7, dtype=torch.int32, device=dev)
    assert _dev_call(L, g, (ds, dl, dh), 1, 64, dsel, dcnt, dh, dinfo) == 0
    torch.cuda.synchronize()
    sol, info = dh.cpu().numpy(), dinfo.cpu().numpy()
    for i in range(B):
        if i in sel:
            assert np.array_equal(sol[i], whole[0][i]) and np.array_equal(info[i], whole[1][i]), i
        else:
            assert np.array_equal(sol[i], shots.hard[i]) and (info[i] == -7).all(), i


def test_two_streams_and_two_threads(L):
    shots = LS.general("ident")
    g = _graph(L, "ident")
    alone = L.lsd_batch(g, shots.synd, shots.llr, shots.hard, 2, 128)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)        # noqa: E731
    tens = (t(shots.synd), t(shots.llr), t(shots.hard))
    B = shots.synd.shape[0]
    outs = [(torch.zeros((B, g.n), dtype=torch.int8, device=dev), torch.zeros((B, 4), dtype=torch.int32, device=dev)) for _ in range(2)]
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    torch.cuda.synchronize()
    rcs = {}

    def enqueue(k):
        rcs[k] = _dev_call(L, g, tens, 2, 128, None, None, outs[k][0], outs[k][1], streams[k].cuda_stream)
    ts = [threading.Thread(target=enqueue, args=(k,)) for k in range(2)]
    for th in ts:
        th.start()
    for th in ts:
        th.join()
    assert rcs == {0: 0, 1: 0}
    torch.cuda.synchronize()
    for dsol, dinfo in outs:
        assert np.array_equal(dsol.cpu().numpy(), alone[0]) and np.array_equal(dinfo.cpu().numpy(), alone[1])


def test_c_level_refusals(L):
    g = _graph(L, "dep")
    f, _ = LS.matrix("dep")
    synd, llr, hard = np.zeros((2, f.m), np.int8), np.ones((2, f.n)), np.zeros((2, f.n), np.int8)
    for bps, rows in ((0, 512), (65, 512), (-1, 512), (1, 0), (1, 1025), (1, -3)):
        assert _raw(L, g, synd, llr, hard, bps, rows) == -1, (bps, rows)
    assert _raw(L, g, synd, llr, hard, 1, 1024) == 0 and _raw(L, g, synd, llr, hard, 64, 1) == 0
    assert _raw(L, g, synd[:0], llr[:0], hard[:0], 1, 512) == 0
    assert L.lib().qldpc_lsd_batch(None, 1, None, None, None, 1, 512, None, None) == -1
    assert L.lib().qldpc_lsd_batch(g.handle, 1, None, None, None, 1, 512, None, None) == -1
    with pytest.raises(ValueError):
        L.lsd_batch(g, synd, llr, hard, 65, 512)
    with pytest.raises(ValueError):
        L.lsd_batch(g, synd, llr, hard, 1, 1025)
    wide = S.build_matrix("lsd_wide", "dep", 129, 65535)                      # n == 65535: beyond the uint16 column tables
    gw = L.Graph(wide.indptr, wide.indices, wide.n)
    assert _raw(L, gw, np.zeros((1, wide.m), np.int8), np.ones((1, wide.n)), np.zeros((1, wide.n), np.int8), 1, 512) == -4
    with pytest.raises(L.QldpcError, match="65535"):
        L.lsd_batch(gw, np.zeros((1, wide.m), np.int8), np.ones((1, wide.n)), np.zeros((1, wide.n), np.int8))
    gw.close()
    assert LS.supported(f.m, f.n, f.max_col_deg, 1024) and not LS.supported(wide.m, wide.n, wide.max_col_deg, 512)


# ---------------------------------------------------------------------------------------------------------------- the circuit plan
def _by_hand(L, tag, seed, count, bps, max_rows):
    """sampler -> BP -> qldpc_lsd_batch on the unconverged shots -> numpy judge, through the C ABI piece by piece"""
    c, compiled, Mx, graphs, priors, masks, plan = circuit_setup(L, tag)
    p = plan(batch=count)
    spz, tz, spx, tx = p.sample(seed, 0, count)
    p.close()
    verdict = np.zeros(count, np.uint8)
    osd, flags = [], []
    for sec, (g, prior, mask, synd, true) in enumerate(((graphs[0], priors[0], masks[0], spz, tz), (graphs[1], priors[1], masks[1], spx, tx))):
        det, conv, llr, iters = L.minsum_decode_batch(g, synd, prior, 50, "dynamical", 1.0)
        bad = np.flatnonzero(conv == 0)
        fl = np.zeros(3, np.int64)
        if bad.size:
            det[bad], info = L.lsd_batch(g, synd[bad], llr[bad], det[bad], bps, max_rows)
            fl = np.bincount(info[:, 0], minlength=3)
        rows = np.stack([(mask >> np.uint64(r)) & np.uint64(1) for r in range(true.shape[1])]).astype(np.int64)
        dec = (det.astype(np.int64) @ rows.T) % 2
        verdict |= (np.any(dec != true.astype(np.int64), axis=1).astype(np.uint8) << sec)
        osd.append(int(bad.size))
        flags.append(fl)
        assert np.array_equal(L.gf2_spmv_batch(g, det), synd & 1)
    return verdict, osd, np.stack(flags)


@pytest.mark.parametrize("bps, max_rows", ((1, 512), (4, 24)))
def test_circuit_plan_matches_the_pieces(L, bps, max_rows):
    count, seed = 2048, 9876
    verdict, osd, flags = _by_hand(L, "circ72", seed, count, bps, max_rows)
    c, compiled, Mx, graphs, priors, masks, plan = circuit_setup(L, "circ72")
    p = plan(batch=1024)
    assert not p.lsd_counts().any()                                          # never switched: zeros
    p.use_lsd(bps, max_rows)
    got = p.run_outcomes(seed, 0, count)
    tally = p.read()
    counts = p.lsd_counts(clear=True)
    assert not p.lsd_counts().any()
    ph, _ = p.phase_times()
    p.close()
    T = L.TALLY
    assert np.array_equal(got, verdict)
    assert tally[T["trials"]] == count and tally[T["total_err"]] == np.count_nonzero(verdict)
    assert [tally[T["osd_z"]], tally[T["osd_x"]]] == osd and min(osd) > 0
    assert np.array_equal(counts, flags) and counts.sum(axis=1).tolist() == osd
    if max_rows == 24:
        assert counts[:, 1].min() > 0                                        # the small cap stops some
    assert tally[T["unsat_z"]] == 0 and tally[T["unsat_x"]] == 0
    assert ph["osd_z"] > 0 and ph["osd_x"] > 0


def test_plan_switch_rules(L):
    c, compiled, Mx, graphs, priors, masks, plan = circuit_setup(L, "circ72")

    def refused(p, call, match):
        with pytest.raises(L.QldpcError, match=match):
            call(p)
        p.close()
    p = plan(batch=256, use_osd=False)
    refused(p, lambda p: p.use_lsd(), "use_osd = 0")
    p = plan(batch=256)
    p.use_relay()
    refused(p, lambda p: p.use_lsd(), "Relay-BP")
    p = plan(batch=256)
    p.use_window(3, 1)
    refused(p, lambda p: p.use_lsd(), "sliding-window")
    p = plan(batch=256)
    p.use_osd_cs(7)
    refused(p, lambda p: p.use_lsd(), "BP \\+ OSD-CS: BP \\+ LSD cannot follow")
    for later, match in ((lambda p: p.use_osd_cs(7), "BP \\+ LSD: BP \\+ OSD-CS cannot follow"), (lambda p: p.use_relay(), "BP \\+ LSD"),
                         (lambda p: p.use_window(3, 1), "BP \\+ LSD")):
        p = plan(batch=256)
        p.use_lsd()
        refused(p, later, match)
    p = plan(batch=256)
    p.use_layered()
    p.use_lsd()
    refused(p, lambda p: p.use_osd_cs(3), "BP \\+ LSD: BP \\+ OSD-CS cannot follow")
    p = plan(batch=256)
    with pytest.raises(ValueError):
        p.use_lsd(0, 512)
    with pytest.raises(ValueError):
        p.use_lsd(1, 2000)
    assert L.lib().qldpc_circuit_plan_use_lsd(p.handle, 65, 512) == -1 and L.lib().qldpc_circuit_plan_use_lsd(p.handle, 1, 1025) == -1
    p.close()

    # what stays open: LSD before or after layered, decimation and f32, and again with new parameters
    def tally(p):
        p.run(11, 0, 512)
        t, cnt = p.read(), p.lsd_counts()
        p.close()
        return t, cnt

    p, q = plan(batch=256), plan(batch=256)
    p.use_lsd(4, 16)
    p.use_lsd(1, 512)
    q.use_lsd(1, 512)
    (tp, cp), (tq, cq) = tally(p), tally(q)
    assert np.array_equal(tp, tq) and np.array_equal(cp, cq) and cp.sum() > 0
    for path in (lambda p: p.use_layered(), lambda p: p.use_decimation(), lambda p: p.use_f32()):
        p, q = plan(batch=256), plan(batch=256)
        p.use_lsd()
        path(p)
        path(q)
        q.use_lsd()
        (tp, cp), (tq, cq) = tally(p), tally(q)
        assert np.array_equal(tp, tq) and np.array_equal(cp, cq)
        assert cp.sum(axis=1).tolist() == [tp[L.TALLY["osd_z"]], tp[L.TALLY["osd_x"]]]


def test_run_simulation_and_dem_decoder(L):
    from qldpc_amd.data import load_code, load_precomputed_matrices
    from qldpc_amd.simulation.dem import DemDecoder, DetectorErrorModel, run_dem_simulation
    from qldpc_amd.simulation.engine import run_simulation
    c = load_code("bb72")
    mats = load_precomputed_matrices("circ72")
    kw = dict(num_cycles=6, precomputed_matrices=mats, base_seed=2026, batch=1024, **_bb_params(c))
    r0 = run_simulation(c["Hx"], c["Hz"], c["Lx"], c["Lz"], 0.005, num_trials=2048, devices=[0], **kw)
    r1 = run_simulation(c["Hx"], c["Hz"], c["Lx"], c["Lz"], 0.005, num_trials=2048, devices=[0], decoder="bp_lsd", **kw)
    r2 = run_simulation(c["Hx"], c["Hz"], c["Lx"], c["Lz"], 0.005, num_trials=2048, devices=[0, 0], decoder="bp_lsd", lsd={"bits_per_step": 1}, **kw)
    T = L.TALLY
    assert r1["decoder"] == "bp_lsd" and r1["lsd"] == {"bits_per_step": 1, "max_rows": 512}
    assert np.array_equal(r1["tally"], r2["tally"]) and np.array_equal(r1["lsd_counts"], r2["lsd_counts"])
    assert r1["tally"][T["osd_z"]] == r0["tally"][T["osd_z"]] and r1["tally"][T["osd_x"]] == r0["tally"][T["osd_x"]]
    assert r1["lsd_counts"].sum(axis=1).tolist() == [r1["tally"][T["osd_z"]], r1["tally"][T["osd_x"]]]
    assert r1["tally"][T["unsat_z"]] == 0 and r1["tally"][T["unsat_x"]] == 0
    for bad in (dict(decoder="bp_lsd", osd_order=2), dict(decoder="bp_osd", lsd={}), dict(decoder="bp_lsd", window=(3, 1)), dict(decoder="bp_lsd", lsd={"rows": 3}),
                dict(decoder="bp_lsd", lsd={"max_rows": 0})):
        with pytest.raises(ValueError):
            run_simulation(c["Hx"], c["Hz"], c["Lx"], c["Lz"], 0.005, num_trials=8, devices=[0], **dict(kw, **bad))
    # the strata runner: the same BP stage under a fixed weight, LSD behind it
    from qldpc_amd.simulation.strata import run_weight_strata
    sk = dict(weights=[6, 14], trials_per_weight=256, num_cycles=6, precomputed_matrices=mats, batch=256, base_seed=3, **_bb_params(c))
    s0 = run_weight_strata(c["Hx"], c["Hz"], c["Lx"], c["Lz"], 0.005, **sk)
    s1 = run_weight_strata(c["Hx"], c["Hz"], c["Lx"], c["Lz"], 0.005, decoder="bp_lsd", lsd={"max_rows": 256}, **sk)
    assert np.array_equal(s0.trials, s1.trials) and np.array_equal(s0.bp_converged, s1.bp_converged) and (s1.bp_converged < 256).any()
    dem = DetectorErrorModel.from_decoding_matrices("circ72", layer_rows=36)
    par = {"bits_per_step": 2, "max_rows": 256}
    rd = run_dem_simulation(dem, num_trials=2048, base_seed=5, batch=1024, devices=[0], decoder="bp_lsd", lsd=par)
    assert rd["decoder"] == "bp_lsd" and rd["lsd"] == par and rd["lsd_counts"].sum() == rd["tally"][T["osd_z"]] + rd["tally"][T["osd_x"]] > 0
    # DemDecoder(decoder="bp_lsd") == a plan switched by hand and fed the same records
    count, seed = 512, 5
    plan = dem.plan([L.Graph(v.indptr, v.indices, v.shape[1]) for v in (dem.decoder_view(0), dem.decoder_view(1))], max_iter=50, batch=128)
    spz, _, spx, _ = plan.sample(seed, 0, count)
    events = np.hstack([spz, spx]).astype(np.uint8)                          # the default layout: sector 0's rows, then sector 1's
    plan.use_lsd(**par)
    want = plan.decode_events(L.pack_events(events), seed, 0)
    assert plan.lsd_counts().sum() > 0
    plan.close()
    dec = DemDecoder(dem, decoder="bp_lsd", lsd=par, batch=256, seed=seed)
    (a0, a1), flags = dec.decode_to_flags(events)
    dec.close()
    bits = lambda v, k: ((v[:, None] >> np.arange(k, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)      # noqa: E731
    assert np.array_equal(a0, bits(want[0], dem.k[0])) and np.array_equal(a1, bits(want[1], dem.k[1])) and np.array_equal(flags, want[2])
    assert not (flags & 0xC).any()                                           # every correction reproduces its syndrome
    with pytest.raises(ValueError):
        DemDecoder(dem, decoder="bp_lsd", osd_order=1)


def test_recorded_circ144_cases_equal_the_reference_osd0(L, golden):
    """the 16 recorded OSD cases of circ144_decode.npz: with bits_per_step = 1 every one resolves in clusters, to the reference's OSD-0 answer bit for bit"""
    from qldpc_amd.data import load_circuit_matrices
    f, d = golden("circ144_decode"), load_circuit_matrices("circ144")
    for s in "ZX":
        g = L.Graph(d[f"Hdec{s}_indptr"], d[f"Hdec{s}_indices"], int(d[f"Hdec{s}_shape"][1]))
        cases = f[f"{s}_osd_cases"]
        sol, info = L.lsd_batch(g, f[f"{s}_syndromes"][cases], f[f"{s}_llr"][cases], f[f"{s}_err"][cases], 1, 512)
        assert (info[:, 0] == 0).all() and info[:, 2].max() <= 255 and info[:, 3].max() <= 387
        assert np.array_equal(sol, f[f"{s}_osd_solution"].astype(np.int8))
        G = M.Graph(g.indptr, g.indices, g.n)
        for i, case in enumerate(cases[:2]):                                 # (and the model's info on two of them per sector)
            assert tuple(info[i]) == M.lsd(G, f[f"{s}_syndromes"][case], f[f"{s}_llr"][case], f[f"{s}_err"][case], 1, 512)[1]
        g.close()
