"""Single-precision min-sum on the MI355X: C-level checks, bit equality with tests/minsum32_model.py (err, conv, final_iter and llr, no tolerance) on the
code-capacity, circuit-level and structured graphs, every form selector, batch splits, the device entry point, two host threads on one decoder, the
anchor to the f64 decoder where no f32 operation rounds, what info() reports, the circuit plan switch against the pipeline assembled from pieces,
and run_simulation(precision="f32")."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_shapes as GS  # noqa: E402
import minsum32_model as MM  # noqa: E402
from minsum32_shapes import lds_bytes  # noqa: E402
from test_relay_gpu import _bb_params, circuit_setup, sampled  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("err", "conv", "llr", "final_iter")
MODEL_ALPHA = {"dynamical": "dynamical", "alvarado": "const", "alvarado-autoregressive": "seq"}
LDS_MAX = 160 * 1024


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


def assert_same(got, want, what):
    for name, a, b in zip(NAMES, got, want):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape, (what, name)
        eq = (a == b) | ((a != a) & (b != b)) if name == "llr" else (a == b)        # equal values, NaN where NaN
        bad = np.flatnonzero(~eq.reshape(len(a), -1).all(axis=1))
        assert bad.size == 0, f"{what}: {name} differs on shots {bad[:8].tolist()} ({bad.size} of {len(a)})"


def check(L, g, prior, synd, what, max_iter=50, alpha_mode="dynamical", alpha=1.0, clip_llr=20.0, flags=0):
    """decode with the library and with the model; -> (library outputs, info)"""
    dec = L.Minsum32Decoder(g, prior, max_iter=max_iter, alpha_mode=alpha_mode, alpha=alpha, clip_llr=clip_llr, flags=flags)
    info = dec.info()
    got = dec.decode(synd)
    dec.close()
    assert info["lds_bytes"] == lds_bytes(g.m, g.n) <= LDS_MAX and info["block"] in (256, 512, 1024) and info["wg_per_cu"] >= 1, (what, info)
    want = MM.Minsum32Model(g.indptr, g.indices, g.n, prior).decode(synd, max_iter=max_iter, alpha_mode=MODEL_ALPHA[alpha_mode], alpha=alpha, clip_llr=clip_llr)
    print(f"{what}: {info}; shots {len(synd)}, converged {int(want[1].sum())}, mean iterations {float((want[3] + 1).mean()):.1f}")
    assert_same(got, want, what)
    return got, info


def circuit_inputs(L, golden, tag, count, seed=77):
    c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, tag)
    f = golden(f"{tag}_decode")
    if not count:
        return [(graphs[0], priors[0], f["Z_syndromes"]), (graphs[1], priors[1], f["X_syndromes"])]
    (spz, _), (spx, _) = sampled(L, tag, count, seed=seed)
    return [(graphs[0], priors[0], np.concatenate([f["Z_syndromes"], spz])), (graphs[1], priors[1], np.concatenate([f["X_syndromes"], spx]))]


def exact_prior(n, seed=72):
    """+-(1..32)/4: with alpha 0.5, clip 20 and 12 iterations every value is a multiple of 2^-14 below 2^7, so no f32 operation rounds"""
    rng = np.random.default_rng(seed)
    return rng.integers(1, 33, n) * 0.25 * rng.choice([-1.0, 1.0], n)


def test_c_level_validation(L):
    c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, "circ72")
    g, prior = graphs[0], priors[0]
    lib = L.lib()

    def create(graph=g, pr=prior, max_iter=50, mode=1, seq=None, clip=20.0, flags=0, out=True):
        h = C.c_void_p()
        pr = None if pr is None else np.ascontiguousarray(pr, np.float64)
        sq = None if seq is None else np.ascontiguousarray(seq, np.float64)
        rc = lib.qldpc_minsum32_decoder_create(graph.handle if graph is not None else None, None if pr is None else L.ptr(pr, C.c_double), max_iter, mode, 1.0,
                                               None if sq is None else L.ptr(sq, C.c_double), 0 if sq is None else sq.size, clip, flags,
                                               C.byref(h) if out else None)
        if rc == 0:
            lib.qldpc_minsum32_decoder_destroy(h)
        return rc
    assert create() == 0
    assert create(mode=2, seq=[0.5, 0.75]) == 0
    for kw in (dict(max_iter=0), dict(max_iter=-3), dict(clip=0.0), dict(clip=-1.0), dict(clip=float("nan")), dict(clip=float("inf")), dict(clip=1e39),
               dict(clip=1e-50), dict(mode=9), dict(mode=2), dict(graph=None), dict(pr=None), dict(out=False),
               dict(flags=L.FLAG_F32_BLOCK_256 | L.FLAG_F32_BLOCK_512)):
        assert create(**kw) == -1, kw
    bad = prior.copy()
    bad[3], bad[4] = np.inf, np.nan
    assert create(pr=bad) == 0                                              # a non-finite prior is allowed, as in the plain decoder
    # unsupported: a row of degree 57, more columns than the u16 tables index, more state than LDS holds
    fam = {c.name: c for c in GS.families()}
    wide = fam["rowdeg57"]
    assert create(graph=L.Graph(wide.indptr, wide.indices, wide.n), pr=np.ones(wide.n)) == -4 and b"row degree <= 56" in lib.qldpc_last_error()
    nbig = 70000
    assert create(graph=L.Graph(np.arange(nbig + 1), np.arange(nbig), nbig), pr=np.ones(nbig)) == -4 and b"n < 65535" in lib.qldpc_last_error()
    mbig = 9000
    assert lds_bytes(mbig, mbig) > LDS_MAX
    assert create(graph=L.Graph(np.arange(mbig + 1), np.arange(mbig), mbig), pr=np.ones(mbig)) == -4 and b"LDS" in lib.qldpc_last_error()
    ok = fam["rowdeg56"]
    assert create(graph=L.Graph(ok.indptr, ok.indices, ok.n), pr=np.ones(ok.n)) == 0
    # decode calls
    dec = L.Minsum32Decoder(g, prior)
    assert lib.qldpc_minsum32_decode_batch(dec.handle, 0, None, None, None, None, None) == 0           # B = 0: a no-op
    assert lib.qldpc_minsum32_decode_batch_dev(dec.handle, 0, None, None, None, None, None, None) == 0
    assert lib.qldpc_minsum32_decode_batch(dec.handle, 1, None, None, None, None, None) == -1
    assert lib.qldpc_minsum32_decode_batch(dec.handle, -1, None, None, None, None, None) == -1
    assert lib.qldpc_minsum32_decode_batch(None, 0, None, None, None, None, None) == -1
    assert lib.qldpc_minsum32_decoder_info(None, None, None, None, None) == -1
    assert lib.qldpc_minsum32_decoder_info(dec.handle, None, None, None, None) == 0
    dec.close()
    assert lib.qldpc_circuit_plan_use_f32(None) == -1


def test_bit_exact_on_the_code_capacity_matrices(L, golden):
    f = golden("steane_minsum")
    g = L.Graph(f["indptr"], f["indices"], int(f["n"]))
    for prior in (f["prior"], f["prior2"]):
        check(L, g, prior, f["syndromes"], "steane", max_iter=int(f["max_iter"]))
    check(L, g, f["prior"], f["syndromes"], "steane seq", max_iter=6, alpha_mode="alvarado-autoregressive", alpha=f["seq_alpha"])
    f = golden("bb72_minsum")
    g = L.Graph(f["Hx_indptr"], f["Hx_indices"], int(f["Hx_shape"][1]))
    for p in ("p005", "p030", "p080"):
        got, info = check(L, g, f[f"Hx_{p}_prior"], f[f"Hx_{p}_syndromes"][:16], f"bb72 Hx {p}")
        assert info["clean"]


@pytest.mark.parametrize("alpha_mode,alpha", [("dynamical", 1.0), ("alvarado", 0.8125), ("alvarado-autoregressive", [0.5, 0.625, 0.75, 0.9])])
def test_bit_exact_on_circ72(L, golden, alpha_mode, alpha):
    for sec, (g, prior, synd) in enumerate(circuit_inputs(L, golden, "circ72", 28)):
        assert len(synd) == 32
        got, info = check(L, g, prior, synd, f"circ72 sector {'ZX'[sec]} {alpha_mode}", alpha_mode=alpha_mode, alpha=alpha)
        assert info["clean"] == (sec == 0)                                  # HdecX has degree-1 rows: the any-input kernel
        assert np.array_equal(L.gf2_spmv_batch(g, got[0])[got[1] == 1], (synd & 1)[got[1] == 1])      # converged: H e = s
        if sec == 1:
            assert np.isinf(got[2]).any()
    g, prior, synd = circuit_inputs(L, golden, "circ72", 0)[0]
    check(L, g, prior, synd, "circ72 Z, max_iter 1, clip 6.5", max_iter=1, alpha_mode=alpha_mode, alpha=alpha, clip_llr=6.5)


def test_bit_exact_on_circ144_and_info(L, golden):
    for sec, (g, prior, synd) in enumerate(circuit_inputs(L, golden, "circ144", 0)):
        assert len(synd) == 16
        got, info = check(L, g, prior, synd, f"circ144 sector {'ZX'[sec]}", max_iter=30)
        assert info["lds_bytes"] <= LDS_MAX and info["wg_per_cu"] >= 2, info                # occupancy is the point: two workgroups share a CU


def test_bit_exact_on_circ288(L):
    from qldpc_amd.data import load_circuit_matrices
    from qldpc_amd.simulation.engine import prior_llrs
    d = load_circuit_matrices("circ288")
    ip, ix, shape = d["HdecZ_indptr"], d["HdecZ_indices"], d["HdecZ_shape"]
    assert tuple(int(x) for x in shape) == (2880, 26209)
    g = L.Graph(ip, ix, int(shape[1]))
    prior = prior_llrs(np.asarray(d["channel_probsZ"], np.float64))
    rng = np.random.default_rng(288)
    e = np.zeros((2, g.n), np.int8)
    for b in range(2):
        e[b, rng.choice(g.n, 20, replace=False)] = 1
    got, info = check(L, g, prior, L.gf2_spmv_batch(g, e), "circ288 sector Z", max_iter=6)
    assert info["block"] == 1024 and info["wg_per_cu"] == 1


def test_bit_exact_on_the_graph_shapes(L):
    """every family of tests/graph_shapes.py inside the limits: empty rows (odd_rows), degree-1 checks (deg1_*), the largest accepted row degree
    (rowdeg56, hub_row), a column in every row (hub_col); the others are refused with QLDPC_ERR_UNSUPPORTED"""
    seen, refused = set(), set()
    for case in GS.families():
        if case.expected_path not in ("WG2", "WG"):
            continue
        g = L.Graph(case.indptr, case.indices, case.n)
        prior = case.priors[next(iter(case.priors))]
        deg = np.diff(case.indptr)
        if case.n >= 65535 or deg.max() > 56 or lds_bytes(g.m, g.n) > LDS_MAX:
            with pytest.raises(L.QldpcError, match="error -4"):
                L.Minsum32Decoder(g, prior)
            refused.add(case.name)
            continue
        got, info = check(L, g, prior, GS.syndromes(case, 5), case.name, max_iter=7)
        assert info["clean"] == bool(np.isfinite(prior).all() and not (deg == 1).any()), case.name
        seen.add(case.name)
    assert {"odd_rows", "deg1_distinct", "deg1_shared", "rowdeg56", "hub_row", "hub_col", "m1025", "alldeg_wide"} <= seen, (seen, refused)


def test_nan_and_subnormal_priors_and_every_form(L, golden):
    g, prior, synd = circuit_inputs(L, golden, "circ72", 8)[1]
    odd = prior.copy()
    odd[3], odd[40], odd[77], odd[200] = np.inf, -np.inf, np.nan, -0.0
    got, _ = check(L, g, odd, synd, "non-finite prior", max_iter=10)
    assert np.isnan(got[2][:, 77]).all()
    gz, pz, sz = circuit_inputs(L, golden, "circ72", 8)[0]
    tiny = pz.copy()
    tiny[5], tiny[6] = 1e-40, -1e-40
    check(L, gz, tiny, sz, "subnormal prior", max_iter=10, alpha_mode="alvarado", alpha=0.5)
    g3 = L.Graph(np.array([0, 2, 4]), np.array([0, 1, 1, 2]), 3)
    got, _ = check(L, g3, np.array([1e-40, 3e-40, -2e-39]), np.array([[1, 0], [0, 1]], np.int8), "all subnormal", max_iter=3, alpha_mode="alvarado", alpha=0.5)
    assert np.all(got[2] != 0) and np.all(np.abs(got[2]) < float(np.finfo(np.float32).tiny))           # kept, not flushed
    # every form: the any-input kernel on clean inputs, the three workgroup sizes
    base, info0 = check(L, gz, pz, sz, "circ72 Z default", max_iter=20)
    assert info0["clean"]
    forms = set()
    for flags in (L.FLAG_F32_GENERIC, L.FLAG_F32_BLOCK_256, L.FLAG_F32_BLOCK_512, L.FLAG_F32_BLOCK_1024, L.FLAG_F32_GENERIC | L.FLAG_F32_BLOCK_1024):
        dec = L.Minsum32Decoder(gz, pz, max_iter=20, flags=flags)
        info = dec.info()
        got = dec.decode(sz)
        dec.close()
        forms.add((info["block"], info["clean"]))
        assert_same(got, base, f"flags {flags:#x}")
        assert info["clean"] == (not flags & L.FLAG_F32_GENERIC)
    assert forms == {(info0["block"], False), (256, True), (512, True), (1024, True), (1024, False)}


def test_batch_splits_dev_call_and_two_threads(L, golden):
    g, prior, synd = circuit_inputs(L, golden, "circ72", 28)[1]
    assert len(synd) == 32
    dec = L.Minsum32Decoder(g, prior, max_iter=30)
    whole = dec.decode(synd)
    assert 0 < whole[1].sum()
    for lo, hi in ((0, 1), (1, 32)):
        assert_same(dec.decode(synd[lo:hi]), [w[lo:hi] for w in whole], f"split {lo}:{hi}")
    singles = [dec.decode(synd[b:b + 1]) for b in range(32)]
    assert_same([np.concatenate([s[k] for s in singles]) for k in range(4)], whole, "32 single calls")
    dev = torch.device("cuda:0")
    B = len(synd)
    ds = torch.from_numpy(np.ascontiguousarray(synd)).to(dev)
    derr = torch.full((B, g.n), 5, dtype=torch.int8, device=dev)
    dllr = torch.full((B, g.n), -7.0, dtype=torch.float64, device=dev)
    dconv = torch.full((B,), 9, dtype=torch.uint8, device=dev)
    dit = torch.full((B,), -3, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    rc = L.lib().qldpc_minsum32_decode_batch_dev(dec.handle, B, C.c_void_p(ds.data_ptr()), C.c_void_p(derr.data_ptr()), C.c_void_p(dllr.data_ptr()),
                                                 C.c_void_p(dconv.data_ptr()), C.c_void_p(dit.data_ptr()), C.c_void_p(st.cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert_same([t.cpu().numpy() for t in (derr, dconv, dllr, dit)], whole, "device entry on a side stream")
    res = {}

    def host(k):
        res[k] = dec.decode(synd)
    ts = [threading.Thread(target=host, args=(k,)) for k in range(2)]
    for th in ts:
        th.start()
    for th in ts:
        th.join()
    for k in range(2):
        assert_same(res[k], whole, f"thread {k}")
    dec.close()


def test_anchor_to_the_f64_decoder_where_no_f32_operation_rounds(L, golden):
    for sec, (g, _, synd) in enumerate(circuit_inputs(L, golden, "circ72", 0)):
        prior = exact_prior(g.n)
        dec = L.Minsum32Decoder(g, prior, max_iter=12, alpha_mode="alvarado", alpha=0.5, clip_llr=20.0)
        got = dec.decode(synd)
        dec.close()
        want = L.minsum_decode_batch(g, synd, prior, 12, "alvarado", 0.5, clip_llr=20.0)
        assert_same(got, want, f"anchor, sector {'ZX'[sec]}")


def _pieces(L, setup, seed, count, cs_order=None, max_iter=50):
    """plan sampler -> f32 decode call -> the existing OSD-0 (or OSD-CS) call on the unconverged -> logical comparison"""
    c, compiled, Mx, graphs, priors, masks, plan = setup
    p = plan(batch=count)
    spz, tz, spx, tx = p.sample(seed, 0, count)
    p.close()
    verdict = np.zeros(count, np.uint8)
    out = dict(conv=[], osd=[], unsat=[], iters=[])
    for sec, (g, prior, mask, synd, true) in enumerate(((graphs[0], priors[0], masks[0], spz, tz), (graphs[1], priors[1], masks[1], spx, tx))):
        dec = L.Minsum32Decoder(g, prior, max_iter=max_iter)
        det, conv, llr, iters = dec.decode(synd)
        dec.close()
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
        out["conv"].append(int(conv.sum())); out["osd"].append(int(bad.size)); out["iters"].append(int((iters.astype(np.int64) + 1).sum()))
        out["unsat"].append(int((L.gf2_spmv_batch(g, det) != (synd & 1)).any(axis=1).sum()))
    return verdict, out


@pytest.mark.parametrize("cs_order", [None, 3])
def test_circuit_plan_matches_the_pieces(L, cs_order):
    count, seed = 256, 4321
    setup = circuit_setup(L, "circ72")
    verdict, h = _pieces(L, setup, seed, count, cs_order)
    p = setup[6](batch=128)
    if cs_order is not None:
        p.use_osd_cs(cs_order)
    p.use_f32()
    got = p.run_outcomes(seed, 0, count)
    tally = p.read(clear=True)
    ph, _ = p.phase_times()
    p.close()
    T = L.TALLY
    print(cs_order, "tally", tally.tolist(), "phases", ph)
    assert np.array_equal(got, verdict)
    assert tally[T["trials"]] == count and tally[T["total_err"]] == np.count_nonzero(verdict)
    assert tally[T["z_err"]] == np.count_nonzero(verdict & 1) and tally[T["x_err"]] == np.count_nonzero(verdict & 2)
    assert [tally[T["bp_conv_z"]], tally[T["bp_conv_x"]]] == h["conv"]
    assert [tally[T["osd_z"]], tally[T["osd_x"]]] == h["osd"]
    assert [tally[T["iters_z"]], tally[T["iters_x"]]] == h["iters"]
    assert [tally[T["unsat_z"]], tally[T["unsat_x"]]] == h["unsat"]
    assert tally[T["legs_z"]] == 0 and tally[T["legs_x"]] == 0
    assert ph["bp_z"] > 0 and ph["bp_x"] > 0


def test_unswitched_plan_is_unchanged_and_switch_rules(L):
    plan = circuit_setup(L, "circ72")[6]
    tallies = []
    for _ in range(2):
        p = plan(batch=128)
        p.run(99, 0, 256)
        tallies.append(p.read(clear=True))
        p.close()
        w = plan(batch=128)                                                # an f32 plan in between
        w.use_f32()
        w.run(99, 0, 256)
        assert w.read()[L.TALLY["trials"]] == 256
        w.close()
    assert np.array_equal(tallies[0], tallies[1])
    for first, name in ((lambda p: p.use_relay(), "Relay-BP"), (lambda p: p.use_window(4, 2), "sliding-window"), (lambda p: p.use_layered(), "layered"),
                        (lambda p: p.use_decimation(), "guided decimation")):
        p = plan(batch=128)
        first(p)
        with pytest.raises(L.QldpcError, match=name) as ei:
            p.use_f32()
        assert "f32" in str(ei.value) and "error -1" in str(ei.value)       # QLDPC_ERR_INVALID, naming both sides
        p.close()
    p = plan(batch=128, damping=0.5)
    with pytest.raises(L.QldpcError, match="damping"):
        p.use_f32()
    p.close()
    p = plan(batch=128, max_iter=0)
    with pytest.raises(L.QldpcError, match="max_iter"):
        p.use_f32()
    p.close()
    p = plan(batch=128)
    p.use_f32()
    for again, name in ((lambda: p.use_relay(), "Relay-BP"), (lambda: p.use_window(4, 2), "sliding-window"), (lambda: p.use_layered(), "layered"),
                        (lambda: p.use_decimation(), "guided decimation")):
        with pytest.raises(L.QldpcError, match="f32") as ei:
            again()
        assert name in str(ei.value) and "error -1" in str(ei.value)
    p.use_osd_cs(3)                                                        # the OSD stage is independent of the precision
    p.use_f32()                                                            # one-way: a second call changes nothing
    p.run(1, 0, 64)
    assert p.read()[L.TALLY["trials"]] == 64
    p.close()


def test_run_simulation_f32(L):
    from qldpc_amd.data import load_code, load_precomputed_matrices
    from qldpc_amd.simulation.engine import run_simulation
    c = load_code("bb72")
    kw = dict(num_cycles=6, precomputed_matrices=load_precomputed_matrices("circ72"), base_seed=2027, batch=512, **_bb_params(c))
    args = (c["Hx"], c["Hz"], c["Lx"], c["Lz"], 0.005)
    r1 = run_simulation(*args, num_trials=1000, devices=[0], precision="f32", **kw)
    assert r1["precision"] == "f32" and r1["tally"][L.TALLY["trials"]] == 1000
    p = circuit_setup(L, "circ72")[6](batch=512)
    p.use_f32()
    p.run(2027, 0, 1000)
    assert np.array_equal(p.read(), r1["tally"])                           # equal to the switched plan driven by hand
    p.close()
    r0 = run_simulation(*args, num_trials=500, devices=[0], **kw)
    assert r0["precision"] == "f64" and r0["tally"][L.TALLY["trials"]] == 500
