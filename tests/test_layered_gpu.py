"""Layered-schedule min-sum on the MI355X: C-level checks, bit equality with tests/layered_model.py (err, conv, final_iter and llr, no tolerance) on the
circuit-level, code-capacity and structured graphs, every form selector, batch splits, the device entry point, two host threads on one decoder, the
circuit plan switch against the pipeline assembled from pieces, run_simulation, and that an unswitched plan is unchanged."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_shapes as GS  # noqa: E402
import layered_model as LM  # noqa: E402
import layered_shapes as LSH  # noqa: E402
from test_relay_gpu import _bb_params, circuit_setup, sampled  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("err", "conv", "llr", "final_iter")
MODEL_ALPHA = {"dynamical": ("dynamical", 1.0), "alvarado": ("const", None), "alvarado-autoregressive": ("seq", None)}


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
        assert bad.size == 0, f"{what}: {name} differs from the model on shots {bad[:8].tolist()} ({bad.size} of {len(a)})"


def check(L, g, prior, synd, what, layers=None, max_iter=50, alpha_mode="dynamical", alpha=1.0, clip_llr=20.0, flags=0):
    """decode with the library and with the model; -> (library outputs, info)"""
    dec = L.LayeredDecoder(g, prior, max_iter=max_iter, alpha_mode=alpha_mode, alpha=alpha, clip_llr=clip_llr, layers=layers, flags=flags)
    info, used = dec.info(), dec.layers()
    got = dec.decode(synd)
    dec.close()
    model = LM.LayeredModel(g.indptr, g.indices, g.n, prior, row_layer=layers)
    assert np.array_equal(used, model.row_layer) and info["layers"] == len(model.stages), what
    assert info["max_layer_rows"] == max(model.layer_sizes()) and info["max_layer_edges"] == max(int(st[3].sum()) for st in model.stages), what
    ns, nl = sum(model.layer_sizes()), len(model.stages)                    # the exact layout of the form that runs, and that form is the rule's
    assert info["lds_bytes"] == LSH.lds_bytes(g.n, ns, nl, len(g.indices), info["v_global"], info["lds_indices"]) <= LSH.LDS_BYTES, (what, info)
    assert LSH.FORMS[2 * info["v_global"] + (not info["lds_indices"])] == LSH.form(g.n, ns, nl, len(g.indices), bool(flags & L.FLAG_LAYERED_VGLOBAL),
                                                                                 bool(flags & L.FLAG_LAYERED_GLOBAL_IDX))[0], (what, info)
    forced = {L.FLAG_LAYERED_BLOCK_256: 256, L.FLAG_LAYERED_BLOCK_512: 512, L.FLAG_LAYERED_BLOCK_1024: 1024}
    assert info["block"] == LSH.block(len(g.indices), nl, sum(v for k, v in forced.items() if flags & k)), (what, info)
    want = model.decode(synd, max_iter=max_iter, alpha_mode=MODEL_ALPHA[alpha_mode][0], alpha=alpha, clip_llr=clip_llr)
    print(f"{what}: {info}; shots {len(synd)}, converged {int(want[1].sum())}, mean iterations {float((want[3] + 1).mean()):.1f}")
    assert_same(got, want, what)
    return got, info


def circuit_inputs(L, golden, tag, count, seed=77):
    c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, tag)
    f = golden(f"{tag}_decode")
    (spz, _), (spx, _) = sampled(L, tag, count, seed=seed)
    return [(graphs[0], priors[0], np.concatenate([f["Z_syndromes"], spz])), (graphs[1], priors[1], np.concatenate([f["X_syndromes"], spx]))]


def test_c_level_validation(L):
    c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, "circ72")
    g, prior = graphs[0], priors[0]
    lib = L.lib()

    def create(graph=g, layers=None, pr=prior, max_iter=50, mode=1, seq=None, clip=20.0, flags=0, out=True):
        h = C.c_void_p()
        pr = None if pr is None else np.ascontiguousarray(pr, np.float64)
        lay = None if layers is None else np.ascontiguousarray(layers, np.int32)
        sq = None if seq is None else np.ascontiguousarray(seq, np.float64)
        rc = lib.qldpc_layered_decoder_create(graph.handle if graph is not None else None, None if lay is None else L.ptr(lay, C.c_int32),
                                              None if pr is None else L.ptr(pr, C.c_double), max_iter, mode, 1.0, None if sq is None else L.ptr(sq, C.c_double),
                                              0 if sq is None else sq.size, clip, flags, C.byref(h) if out else None)
        if rc == 0:
            lib.qldpc_layered_decoder_destroy(h)
        return rc
    assert create() == 0
    assert create(mode=2, seq=[0.5, 0.75]) == 0
    for kw in (dict(max_iter=0), dict(max_iter=-3), dict(clip=0.0), dict(clip=-1.0), dict(clip=float("nan")), dict(mode=9), dict(mode=2), dict(graph=None),
               dict(pr=None), dict(out=False), dict(flags=L.FLAG_LAYERED_BLOCK_256 | L.FLAG_LAYERED_BLOCK_512)):
        assert create(**kw) == -1, kw
    neg = np.arange(g.m)
    neg[9] = -1
    assert create(layers=neg) == -1 and b"row_layer[9]" in lib.qldpc_last_error()
    shares = np.flatnonzero(np.bincount(g.indices, minlength=g.n) >= 2)[0]
    a, b = [i for i in range(g.m) if shares in g.indices[g.indptr[i]:g.indptr[i + 1]]][:2]
    lay = np.arange(g.m)
    lay[b] = lay[a]
    assert create(layers=lay) == -1
    msg = lib.qldpc_last_error().decode()
    assert f"rows {a} and {b}" in msg and f"column {shares}" in msg, msg
    bad = prior.copy()
    bad[3], bad[4] = np.inf, np.nan
    assert create(pr=bad) == 0                                              # a non-finite prior is allowed, as in the plain decoder
    # unsupported: a row of degree 57, and more rows than the LDS records hold
    fam = {c.name: c for c in GS.families()}
    wide = fam["rowdeg57"]
    assert create(graph=L.Graph(wide.indptr, wide.indices, wide.n), pr=np.ones(wide.n)) == -4 and b"row degree" in lib.qldpc_last_error()
    mbig = 6000
    assert create(graph=L.Graph(np.arange(mbig + 1), np.arange(mbig), mbig), pr=np.ones(mbig)) == -4 and b"LDS" in lib.qldpc_last_error()
    ok = fam["rowdeg56"]
    assert create(graph=L.Graph(ok.indptr, ok.indices, ok.n), pr=np.ones(ok.n)) == 0
    # decode calls
    dec = L.LayeredDecoder(g, prior)
    assert lib.qldpc_layered_decode_batch(dec.handle, 0, None, None, None, None, None) == 0           # B = 0: a no-op
    assert lib.qldpc_layered_decode_batch_dev(dec.handle, 0, None, None, None, None, None, None) == 0
    assert lib.qldpc_layered_decode_batch(dec.handle, 1, None, None, None, None, None) == -1
    assert lib.qldpc_layered_decode_batch(dec.handle, -1, None, None, None, None, None) == -1
    assert lib.qldpc_layered_decode_batch(None, 0, None, None, None, None, None) == -1
    assert lib.qldpc_layered_decoder_info(None, None, None, None, None, None) == -1
    assert lib.qldpc_layered_decoder_info(dec.handle, None, None, None, None, None) == 0
    dec.close()
    assert lib.qldpc_check_layers(None, None, None) == -1
    from qldpc_amd.decoding.layered import check_layers
    for gr in graphs:
        lay, nl = L.graph_check_layers(gr)
        assert np.array_equal(lay, check_layers((gr.indptr, gr.indices, gr.n))) and nl == lay.max() + 1


@pytest.mark.parametrize("tag,count", [("circ72", 64), ("circ144", 32)])
def test_bit_exact_on_the_circuit_matrices(L, golden, tag, count):
    for sec, (g, prior, synd) in enumerate(circuit_inputs(L, golden, tag, count)):
        assert len(synd) >= count + (4 if tag == "circ72" else 16)
        got, info = check(L, g, prior, synd, f"{tag} sector {'ZX'[sec]}")
        assert not info["v_global"] and info["lds_indices"]                # everything in LDS for the bundled sets
        assert np.array_equal(L.gf2_spmv_batch(g, got[0])[got[1] == 1], (synd & 1)[got[1] == 1])      # converged: H e = s


def test_bit_exact_on_the_code_capacity_matrices(L, golden):
    for name in ("bb72", "bb144", "bb288"):
        f = golden(f"{name}_minsum")
        for h in ("Hx", "Hz"):
            g = L.Graph(f[f"{h}_indptr"], f[f"{h}_indices"], int(f[f"{h}_shape"][1]))
            for p in ("p005", "p030", "p080"):
                if f"{h}_{p}_syndromes" in f:
                    check(L, g, f[f"{h}_{p}_prior"], f[f"{h}_{p}_syndromes"], f"{name} {h} {p}")
    f = golden("steane_minsum")
    g = L.Graph(f["indptr"], f["indices"], int(f["n"]))
    for prior in (f["prior"], f["prior2"]):
        check(L, g, prior, f["syndromes"], "steane", max_iter=int(f["max_iter"]))
    check(L, g, f["prior"], f["syndromes"], "steane seq", max_iter=6, alpha_mode="alvarado-autoregressive", alpha=f["seq_alpha"])


def test_bit_exact_on_the_graph_shapes(L):
    """every family of tests/graph_shapes.py that the workgroup kernels accept: empty rows (odd_rows), degree-1 checks (deg1_*), the largest accepted
    row degree (rowdeg56, hub_row), more layers than rows per layer (hub_col: every row meets column 17), posteriors beyond LDS (vglobal_beyond_*)"""
    seen = set()
    for case in GS.families():
        if case.expected_path not in ("WG2", "WG"):
            continue
        g = L.Graph(case.indptr, case.indices, case.n)
        prior = case.priors[next(iter(case.priors))]
        got, info = check(L, g, prior, GS.syndromes(case, 5), case.name, max_iter=7)
        seen.add(case.name)
        if case.name == "hub_col":
            assert info["layers"] == 300 and info["max_layer_rows"] == 1
        if case.name.startswith("vglobal_beyond"):
            assert info["v_global"]
    assert {"odd_rows", "deg1_distinct", "deg1_shared", "rowdeg56", "hub_row", "hub_col", "m1025", "alldeg_wide"} <= seen


def test_serial_and_caller_layers(L, golden):
    (gz, pz, sz), (gx, px, sx) = circuit_inputs(L, golden, "circ72", 12)
    check(L, gz, pz, sz, "circ72 Z, one row per layer", layers=np.arange(gz.m), max_iter=20)
    greedy = LM.greedy_layers(gx.indptr, gx.indices, gx.n)
    flipped = greedy.max() - greedy                                         # the greedy layers in reverse order
    got_f, _ = check(L, gx, px, sx, "circ72 X, reversed layers", layers=flipped, max_iter=20)
    last = greedy.copy()
    last[np.diff(gx.indptr) == 1] = greedy.max() + 5                        # the degree-1 checks in a last layer of their own, a gap before it
    got_l, info = check(L, gx, px, sx, "circ72 X, degree-1 checks last", layers=last, max_iter=20)
    assert info["layers"] == greedy.max() + 2
    cols1 = gx.indices[gx.indptr[:-1][np.diff(gx.indptr) == 1]]
    assert np.isinf(got_l[2][:, cols1]).all() and not np.isnan(got_l[2]).any()


def test_alpha_modes_and_clipping(L, golden):
    (gz, pz, sz), (gx, px, sx) = circuit_inputs(L, golden, "circ72", 24)
    for clip in (20.0, 6.5):
        check(L, gx, px, sx, f"const, clip {clip}", alpha_mode="alvarado", alpha=0.8125, clip_llr=clip, max_iter=30)
        check(L, gx, px, sx, f"dynamical, clip {clip}", clip_llr=clip, max_iter=30)
        check(L, gz, pz, sz, f"seq, clip {clip}", alpha_mode="alvarado-autoregressive", alpha=[0.5, 0.625, 0.75, 0.9], clip_llr=clip, max_iter=30)
    check(L, gz, pz, sz, "max_iter 1", max_iter=1)
    odd = px.copy()
    odd[3], odd[40], odd[77], odd[200] = np.inf, -np.inf, np.nan, -0.0
    check(L, gx, odd, sx, "non-finite prior", max_iter=10)


@pytest.mark.parametrize("tag", ["circ72", "circ144"])
def test_results_do_not_depend_on_the_form(L, golden, tag):
    g, prior, synd = circuit_inputs(L, golden, tag, 12)[1]
    base, info0 = check(L, g, prior, synd, f"{tag} default", max_iter=20)
    forms = set()
    for flags in (L.FLAG_LAYERED_BLOCK_256, L.FLAG_LAYERED_BLOCK_512, L.FLAG_LAYERED_BLOCK_1024, L.FLAG_LAYERED_GLOBAL_IDX, L.FLAG_LAYERED_VGLOBAL,
                  L.FLAG_LAYERED_VGLOBAL | L.FLAG_LAYERED_GLOBAL_IDX | L.FLAG_LAYERED_BLOCK_256):
        dec = L.LayeredDecoder(g, prior, max_iter=20, flags=flags)
        info = dec.info()
        got = dec.decode(synd)
        dec.close()
        forms.add((info["block"], info["v_global"], info["lds_indices"]))
        assert_same(got, base, f"{tag} flags {flags:#x}")
        assert info["v_global"] == bool(flags & L.FLAG_LAYERED_VGLOBAL) and info["lds_indices"] == (not flags & L.FLAG_LAYERED_GLOBAL_IDX)
    assert len(forms) == 6


def test_batch_splits_dev_call_and_two_threads(L, golden):
    g, prior, synd = circuit_inputs(L, golden, "circ144", 184)[1]
    synd = synd[:200]
    dec = L.LayeredDecoder(g, prior, max_iter=30)
    whole = dec.decode(synd)
    assert 0 < whole[1].sum() < len(synd)
    for lo, hi in ((0, 1), (1, 77), (77, 200)):
        part = dec.decode(synd[lo:hi])
        assert_same(part, [w[lo:hi] for w in whole], f"split {lo}:{hi}")
    dev = torch.device("cuda:0")
    B = len(synd)
    ds = torch.from_numpy(np.ascontiguousarray(synd)).to(dev)
    derr = torch.full((B, g.n), 5, dtype=torch.int8, device=dev)
    dllr = torch.full((B, g.n), -7.0, dtype=torch.float64, device=dev)
    dconv = torch.full((B,), 9, dtype=torch.uint8, device=dev)
    dit = torch.full((B,), -3, dtype=torch.int32, device=dev)
    st = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    rc = L.lib().qldpc_layered_decode_batch_dev(dec.handle, B, C.c_void_p(ds.data_ptr()), C.c_void_p(derr.data_ptr()), C.c_void_p(dllr.data_ptr()),
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


def _pieces(L, setup, seed, count, cs_order=None, max_iter=50):
    """plan sampler -> layered decode call -> the existing OSD-0 (or OSD-CS) call on the unconverged -> logical comparison"""
    c, compiled, Mx, graphs, priors, masks, plan = setup
    p = plan(batch=count)
    spz, tz, spx, tx = p.sample(seed, 0, count)
    p.close()
    verdict = np.zeros(count, np.uint8)
    out = dict(conv=[], osd=[], unsat=[], iters=[])
    for sec, (g, prior, mask, synd, true) in enumerate(((graphs[0], priors[0], masks[0], spz, tz), (graphs[1], priors[1], masks[1], spx, tx))):
        dec = L.LayeredDecoder(g, prior, max_iter=max_iter)
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


@pytest.mark.parametrize("tag", ["circ72", "circ144"])
@pytest.mark.parametrize("cs_order", [None, 6])
def test_circuit_plan_matches_the_pieces(L, tag, cs_order):
    count, seed = 512, 4321
    setup = circuit_setup(L, tag)
    verdict, h = _pieces(L, setup, seed, count, cs_order)
    p = setup[6](batch=256)
    if cs_order is not None:
        p.use_osd_cs(cs_order)
    p.use_layered()
    got = p.run_outcomes(seed, 0, count)
    tally = p.read(clear=True)
    ph, _ = p.phase_times()
    p.close()
    T = L.TALLY
    print(tag, cs_order, "tally", tally.tolist(), "phases", ph)
    assert np.array_equal(got, verdict)
    assert tally[T["trials"]] == count and tally[T["total_err"]] == np.count_nonzero(verdict)
    assert tally[T["z_err"]] == np.count_nonzero(verdict & 1) and tally[T["x_err"]] == np.count_nonzero(verdict & 2)
    assert [tally[T["bp_conv_z"]], tally[T["bp_conv_x"]]] == h["conv"]
    assert [tally[T["osd_z"]], tally[T["osd_x"]]] == h["osd"]
    assert [tally[T["iters_z"]], tally[T["iters_x"]]] == h["iters"]
    assert [tally[T["unsat_z"]], tally[T["unsat_x"]]] == h["unsat"]
    assert tally[T["legs_z"]] == 0 and tally[T["legs_x"]] == 0
    assert ph["bp_z"] > 0 and ph["bp_x"] > 0


@pytest.mark.parametrize("tag", ["circ72", "circ144"])
def test_unswitched_plan_is_unchanged(L, tag):
    """an unswitched plan's tally for a fixed seed is the same before and after layered plans ran, and equals the flooding pieces"""
    setup = circuit_setup(L, tag)
    c, compiled, Mx, graphs, priors, masks, plan = setup
    count = 1024
    p = plan(batch=512)
    p.run(99, 0, count)
    t0 = p.read(clear=True)
    p.close()
    w = plan(batch=512)
    w.use_layered()
    w.run(99, 0, count)
    tw = w.read(clear=True)
    w.close()
    p = plan(batch=512)
    p.run(99, 0, count)
    t1 = p.read(clear=True)
    p.close()
    assert np.array_equal(t0, t1)
    T = L.TALLY
    assert tw[T["trials"]] == count and not np.array_equal(t0, tw)          # a different schedule: different iteration counts
    # ... and what it gives today is the flooding decoder's: conv / iteration sums of the plain decode call on the sampled syndromes
    q = plan(batch=count)
    spz, tz, spx, tx = q.sample(99, 0, count)
    q.close()
    for sfx, g, prior, synd in (("z", graphs[0], priors[0], spz), ("x", graphs[1], priors[1], spx)):
        det, conv, llr, iters = L.minsum_decode_batch(g, synd, prior, 50, "dynamical", 1.0)
        assert t0[T["bp_conv_" + sfx]] == int(conv.sum()) and t0[T["iters_" + sfx]] == int((iters.astype(np.int64) + 1).sum())


def test_plan_switch_rules(L):
    plan = circuit_setup(L, "circ72")[6]
    p = plan(batch=256)
    p.use_relay()
    with pytest.raises(L.QldpcError, match="Relay-BP"):
        p.use_layered()
    p.close()
    p = plan(batch=256)
    p.use_window(4, 2)
    with pytest.raises(L.QldpcError, match="sliding-window"):
        p.use_layered()
    p.close()
    p = plan(batch=256, damping=0.5)
    with pytest.raises(L.QldpcError, match="damping"):
        p.use_layered()
    p.close()
    p = plan(batch=256, max_iter=0)
    with pytest.raises(L.QldpcError, match="max_iter"):
        p.use_layered()
    p.close()
    p = plan(batch=256)
    with pytest.raises(ValueError):
        p.use_layered(np.zeros(3, np.int32), None)
    with pytest.raises(L.QldpcError, match="share column"):
        p.use_layered(np.zeros(p.graph_z.m, np.int32), None)
    p.use_layered()
    for again in (lambda: p.use_relay(), lambda: p.use_window(4, 2)):
        with pytest.raises(L.QldpcError, match="layered"):
            again()
    p.use_osd_cs(5)                                                        # the OSD stage is independent of the schedule
    p.use_layered(np.arange(p.graph_z.m), None)                            # new layers replace the old ones
    p.run(1, 0, 64)
    assert p.read()[L.TALLY["trials"]] == 64
    p.close()
    p = plan(batch=256, use_osd=False)                                     # BP alone
    p.use_layered()
    p.run(1, 0, 64)
    t = p.read()
    assert t[L.TALLY["trials"]] == 64 and t[L.TALLY["osd_z"]] == 0
    p.close()


def test_run_simulation_layered(L):
    from qldpc_amd.data import load_code, load_precomputed_matrices
    from qldpc_amd.simulation.engine import run_simulation
    c = load_code("bb72")
    kw = dict(num_cycles=6, precomputed_matrices=load_precomputed_matrices("circ72"), base_seed=2027, batch=1024, **_bb_params(c))
    args = (c["Hx"], c["Hz"], c["Lx"], c["Lz"], 0.005)
    r1 = run_simulation(*args, num_trials=3000, devices=[0], schedule="layered", **kw)
    r2 = run_simulation(*args, num_trials=3000, devices=[0, 0], schedule="layered", **kw)
    assert r1["schedule"] == "layered" and (r1["layers_z"], r1["layers_x"]) == (24, 16)
    assert r1["tally"][L.TALLY["trials"]] == 3000 and np.array_equal(r1["tally"], r2["tally"])        # reproducible, whatever the workers
    p = circuit_setup(L, "circ72")[6](batch=1024)
    p.use_layered()
    p.run(2027, 0, 3000)
    assert np.array_equal(p.read(), r1["tally"])                           # ... and equal to the plan run
    p.close()
    r3 = run_simulation(*args, num_trials=1500, devices=[0], schedule="layered", decoder="bp_osd_cs", osd_order=5, **kw)
    assert r3["schedule"] == "layered" and r3["decoder"] == "bp_osd_cs" and r3["tally"][L.TALLY["trials"]] == 1500
    r0 = run_simulation(*args, num_trials=1500, devices=[0], **kw)
    assert "schedule" not in r0 and r0["tally"][L.TALLY["trials"]] == 1500
