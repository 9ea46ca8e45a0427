"""Sliding-window decoding on the MI355X over the layered graph families of tests/window_shapes.py: the library against tests/window_model.py on
every shot of every family, prior and (W, C); the decode paths and OSD-0 forms its windows take; refusals; the argument axes; a batch beyond the grid
cap of the gather and commit kernels; and a two-sector detector error model whose sectors have different layer_rows.  Every compared quantity is an
integer or a bit pattern and must be equal."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import osd_shapes as OS  # noqa: E402
import window_shapes as WS  # noqa: E402
from test_dem_gpu import assert_tally, logical_errors, parts  # noqa: E402
from test_window_gpu import _assert_equal  # noqa: E402

pytestmark = pytest.mark.gpu

FAMILIES = WS.families()
BY_NAME = {c.name: c for c in FAMILIES}
NAMES = ["lr1", "periodic_r42", "small_irregular", "mid_lr33", "wide_lr130", "heavy_rows", "gaps", "one_layer", "prior_variants"]
ARGS = {"iter0": dict(max_iter=0), "iter1": dict(max_iter=1), "iter9": dict(max_iter=9), "const": dict(alpha_mode="alvarado", alpha=0.8),
        "seq": dict(alpha_mode="alvarado-autoregressive", alpha=np.array([0.55, 0.7, 0.9])), "clip6.5": dict(clip_llr=6.5)}
FLAG_SETS = ("FLAG_KERNEL_STREAM", "FLAG_KERNEL_GENERIC", "FLAG_OSD_REFORDER", "FLAG_OSD_GLOBAL")
_T0 = time.perf_counter()
_REF, _GRAPHS = {}, {}
_SEEN = {"paths": set(), "osd": set(), "families": 0, "conv": 0, "osd_windows": 0, "unsat": 0, "shared": 0, "wg2": 0}


def test_the_module_covers_every_family():
    assert NAMES == [c.name for c in WS.families()]


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


def graph_of(L, case):
    if case.name not in _GRAPHS:
        _GRAPHS[case.name] = L.Graph(case.indptr, case.indices, case.n)
    return _GRAPHS[case.name]


def reference(orc, case, prior, W, C, S=None, tag=None, **args):
    """(model, syndromes, the model's five outputs) for one configuration; computed once and left unchanged"""
    key = (case.name, prior, W, C, tag, tuple(sorted((k, repr(v)) for k, v in args.items())))
    if key not in _REF:
        mo = WS.model(case, prior, W, C)
        S = WS.syndromes(case, WS.SHOTS) if S is None else S
        _REF[key] = (mo, S, mo.decode(orc, S, **dict(dict(max_iter=WS.MAX_ITER), **args)))
    return _REF[key]


def decoded(case):
    return [(p, W, C) for p in case.priors for W, C in case.configs if (W, C) not in case.refused]


def path_names(L):
    return {L.PATH_REGULAR: "REGULAR", L.PATH_RESIDENT: "RESIDENT", L.PATH_WG2: "WG2", L.PATH_WG: "WG", L.PATH_STREAM: "STREAM"}


def osd_names(L):
    return {L.OSD_PATH_SMALL: "SMALL", L.OSD_PATH_GJ: "GJ", L.OSD_PATH_GJG: "GJG", L.OSD_PATH_REFORDER_LDS: "REFORDER_LDS",
            L.OSD_PATH_REFORDER_UG: "REFORDER_UG", L.OSD_PATH_GLOBAL: "GLOBAL"}


@pytest.mark.parametrize("name", NAMES)
def test_library_equals_model_and_takes_the_expected_paths(L, oracle, name):
    c = BY_NAME[name]
    g = graph_of(L, c)
    alone, osd_done, paths_family, want_family = {}, set(), set(), set()
    rng = np.random.default_rng(c.seed)
    for prior, W, Cm in decoded(c):
        model, S, want = reference(oracle, c, prior, W, Cm)
        dec = L.WindowDecoder(g, c.layer_rows, W, Cm, c.priors[prior], max_iter=WS.MAX_ITER)
        info = dec.info()
        got = dec.decode(S)
        dec.close()
        what = f"{name}, {prior}, ({W}, {Cm})"
        _assert_equal(got, want, what)
        assert np.array_equal((L.gf2_spmv_batch(g, got[0]) != (S & 1)).any(axis=1), got[4] != 0), what      # unsat is exactly H err != s
        assert info["windows"] == len(model.stages) and info["graphs"] == model.distinct_graphs(), (what, info)
        assert info["max_rows"] == max(s["r1"] - s["r0"] for s in model.stages) and info["max_cols"] == max(s["cols"].size for s in model.stages), (what, info)
        # stand-alone handles of the model's window graphs: the path each takes with its prior slice, and the OSD-0 form of every window size
        paths = {}
        for gid, st in zip(model.graph_ids(), model.stages):
            if gid in paths:
                continue
            key = (st["indptr"].tobytes(), st["indices"].tobytes(), st["cols"].size)
            if key not in alone:
                alone[key] = L.Graph(st["indptr"], st["indices"], st["cols"].size)
            wg = alone[key]
            paths[gid] = L.minsum_decode_path(wg, st["prior"], WS.MAX_ITER, "dynamical", 1.0)[0]
            if (wg.m, wg.n) not in osd_done:
                osd_done.add((wg.m, wg.n))
                s2 = (rng.random((2, wg.m)) < 0.5).astype(np.int8)
                llr = rng.normal(1.0, 2.0, (2, wg.n))
                hard = (llr < 0).astype(np.int8)
                sol = L.osd0_batch(wg, s2, llr, hard)
                for b in range(2):
                    assert np.array_equal(sol[b], oracle.osd0(st["indptr"], st["indices"], wg.n, s2[b], llr[b], hard[b])), (what, wg.m, wg.n)
                form = osd_names(L)[L.osd0_last_path(wg)[0]]
                cd = np.bincount(st["indices"], minlength=wg.n)
                assert form == OS.rule_path(wg.m, wg.n, int(cd.max())).path, (what, wg.m, wg.n, form)
                assert (form == "SMALL") == (wg.m <= 128 and wg.n <= 1024) and (form == "GJG" or wg.m <= 1024), (what, wg.m, wg.n, form)
                _SEEN["osd"].add("m > 1024" if wg.m > 1024 else form)
        assert info["wg2_windows"] == sum(paths[gid] == L.PATH_WG2 for gid in model.graph_ids()), (what, info, paths)
        taken = {path_names(L)[p] for p in paths.values()}
        assert taken == WS.expected_paths(c, prior, W, Cm), what
        paths_family |= taken
        want_family |= WS.expected_paths(c, prior, W, Cm)
        _SEEN["conv"] += int(want[1].sum()); _SEEN["osd_windows"] += int(want[3].sum()); _SEEN["unsat"] += int(want[4].sum())
        _SEEN["shared"] += int(info["graphs"] < info["windows"]); _SEEN["wg2"] += info["wg2_windows"]
        if name == "prior_variants" and prior == "all distinct":
            assert info["graphs"] == info["windows"] and info["wg2_windows"] == 0
        if W >= c.layers:                                                   # rule 7 of the header, against the library's own whole-graph calls
            det, cv, llr, it = L.minsum_decode_batch(g, S, c.priors[prior], WS.MAX_ITER, "dynamical", 1.0)
            bad = np.flatnonzero(cv == 0)
            if bad.size:
                det[bad] = L.osd0_batch(g, S[bad], llr[bad], det[bad])
            assert info["windows"] == 1 and np.array_equal(got[0], det) and np.array_equal(got[2], it + 1), what
    assert paths_family == want_family
    print(f"{name}: paths {sorted(paths_family)}, {len(osd_done)} window sizes, {time.perf_counter() - _T0:.1f} s since the module was imported")
    _SEEN["paths"] |= paths_family
    _SEEN["families"] += 1
    if _SEEN["families"] == len(NAMES):                                     # the sweep was about what it says: every path, every OSD-0 form, both outcomes
        assert _SEEN["paths"] == {"REGULAR", "RESIDENT", "WG2", "WG", "STREAM"}, _SEEN
        assert _SEEN["osd"] >= {"SMALL", "GJ", "m > 1024"}, _SEEN
        assert min(_SEEN["conv"], _SEEN["osd_windows"], _SEEN["unsat"], _SEEN["shared"], _SEEN["wg2"]) > 0, _SEEN


def test_refusals(L, oracle):
    UNSUPPORTED = -4                                                        # QLDPC_ERR_UNSUPPORTED
    refusing = [c for c in FAMILIES if c.refused]
    assert [c.name for c in refusing] == ["gaps"]
    for c in refusing:
        g = graph_of(L, c)
        for (W, Cm), layer in c.refused.items():
            for prior in c.priors.values():
                out = C.c_void_p(0xdead)
                pr = np.ascontiguousarray(prior, np.float64)
                rc = L.lib().qldpc_window_decoder_create(g.handle, c.layer_rows, W, Cm, L.ptr(pr, C.c_double), WS.MAX_ITER, L.ALPHA_DYNAMIC, 1.0, None, 0, 20.0, 0,
                                                         C.byref(out))
                text = (L.lib().qldpc_last_error() or b"").decode()
                assert rc == UNSUPPORTED and not out.value, (W, Cm, rc, text)
                assert f"the window at layer {layer} has no columns" in text, (W, Cm, text)
                with pytest.raises(L.QldpcError, match=f"layer {layer} "):
                    L.WindowDecoder(g, c.layer_rows, W, Cm, prior)
            # a decoder created right afterwards on the same graph works
            prior, W2, C2 = decoded(c)[0]
            model, S, want = reference(oracle, c, prior, W2, C2)
            dec = L.WindowDecoder(g, c.layer_rows, W2, C2, c.priors[prior], max_iter=WS.MAX_ITER)
            got = dec.decode(S)
            dec.close()
            _assert_equal(got, want, f"{c.name} after the refusal of ({W}, {Cm})")


def _axis_configs(c):
    return [(p, W, Cm) for p, W, Cm in decoded(c) if (W, Cm) in ((1, 1), (2, 1), (3, 2), (4, 3))]


@pytest.mark.parametrize("name", NAMES)
def test_arguments(L, oracle, name):
    c = BY_NAME[name]
    g = graph_of(L, c)
    for axis in c.axes:
        if axis in ("big", "flags", "generic"):
            continue
        args = ARGS[axis]
        for prior, W, Cm in _axis_configs(c):
            model, S, want = reference(oracle, c, prior, W, Cm, **args)
            dec = L.WindowDecoder(g, c.layer_rows, W, Cm, c.priors[prior], **dict(dict(max_iter=WS.MAX_ITER), **args))
            got = dec.decode(S)
            dec.close()
            _assert_equal(got, want, f"{name}, {prior}, ({W}, {Cm}), {axis}")
            if axis == "iter0":                                             # no iteration: nothing converges, every window goes through OSD-0, final_iter = -1
                assert not got[1].any() and not got[2].any() and (got[3] == len(model.stages)).all()
    if "clip6.5" in c.axes:
        assert any((np.abs(p) > 6.5).any() for p in c.priors.values())      # a clip below the prior
    # the flag sets: results never depend on them.  QLDPC_FLAG_KERNEL_GENERIC asks for the resident family (here: the generic resident kernel in place of
    # the regular one); where a window graph is outside that family creation refuses it, as qldpc_minsum_decode_batch does with that flag
    flag_sets = [f for f in FLAG_SETS if ("generic" if f == "FLAG_KERNEL_GENERIC" else "flags") in c.axes]
    for prior, W, Cm in _axis_configs(c) if flag_sets else ():
        model, S, want = reference(oracle, c, prior, W, Cm)
        for fname in flag_sets:
            dec = L.WindowDecoder(g, c.layer_rows, W, Cm, c.priors[prior], max_iter=WS.MAX_ITER, flags=getattr(L, fname))
            got = dec.decode(S)
            dec.close()
            _assert_equal(got, want, f"{name}, {prior}, ({W}, {Cm}), {fname}")
        if "generic" in c.axes:
            assert WS.expected_paths(c, prior, W, Cm) <= {"REGULAR", "RESIDENT"}
        elif not WS.expected_paths(c, prior, W, Cm) <= {"REGULAR", "RESIDENT"}:
            with pytest.raises(L.QldpcError, match="error -4: resident kernel does not support this graph"):
                L.WindowDecoder(g, c.layer_rows, W, Cm, c.priors[prior], max_iter=WS.MAX_ITER, flags=L.FLAG_KERNEL_GENERIC)
    assert set(WS.AXES) == set(a for f in FAMILIES for a in f.axes)
    assert [f.name for f in FAMILIES if "generic" in f.axes] == ["periodic_r42", "small_irregular"] and len([f for f in FAMILIES if "flags" in f.axes]) == 2


def test_big_batch(L, oracle):
    c, prior, (W, Cm), S, max_iter = WS.big_batch(FAMILIES)
    B = len(S)
    assert B == 8200
    model, S, want = reference(oracle, c, prior, W, Cm, S=S, tag="big", max_iter=max_iter)
    g = graph_of(L, c)
    dec = L.WindowDecoder(g, c.layer_rows, W, Cm, c.priors[prior], max_iter=max_iter)
    whole = dec.decode(S)
    _assert_equal(whole, want, "8200 shots")
    assert (want[3] > 0).sum() > 2048
    for lo, hi in ((0, 1), (1, 8193), (8193, 8200)):
        part = dec.decode(S[lo:hi])
        for nm, a, b in zip(("err", "conv", "iters", "osd", "unsat"), part, whole):
            assert np.array_equal(a, b[lo:hi]), (nm, lo, hi)
    dev = torch.device("cuda:0")
    ds = torch.from_numpy(np.ascontiguousarray(S)).to(dev)
    derr = torch.full((B, c.n), 5, dtype=torch.int8, device=dev)
    dconv, dit, dosd = (torch.full((B,), -3, dtype=torch.int32, device=dev) for _ in range(3))
    dun = torch.full((B,), 9, dtype=torch.uint8, device=dev)
    st = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    rc = L.lib().qldpc_window_decode_batch_dev(dec.handle, B, C.c_void_p(ds.data_ptr()), C.c_void_p(derr.data_ptr()), C.c_void_p(dconv.data_ptr()),
                                               C.c_void_p(dit.data_ptr()), C.c_void_p(dosd.data_ptr()), C.c_void_p(dun.data_ptr()), C.c_void_p(st.cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    for nm, a, b in zip(("err", "conv", "iters", "osd", "unsat"), (derr, dconv, dit, dosd, dun), whole):
        assert np.array_equal(a.cpu().numpy(), b), nm
    dec.close()


def _two_sector_dem(L):
    """gaps (layer_rows 10) and periodic_r42 (layer_rows 12) as the two sectors of one model: the mechanisms are the columns of the first, then those of
    the second, each touching its own sector; three observables per sector, each a random subset of the columns."""
    from qldpc_amd.simulation.dem import DetectorErrorModel
    secs = [BY_NAME["gaps"], BY_NAME["periodic_r42"]]
    rng = np.random.default_rng(20261019)
    prob, columns = [], []
    for s, c in enumerate(secs):
        rows = np.repeat(np.arange(c.m), np.diff(c.indptr))
        for j in range(c.n):
            mine = (rows[c.indices == j], int(sum(int(rng.random() < 0.15) << r for r in range(3))))
            columns.append([mine, ([], 0)] if s == 0 else [([], 0), mine])
            prob.append(rng.uniform(0.02, 0.08))                            # high enough that min-sum fails in some windows of both sectors
    dem = DetectorErrorModel.from_columns(np.array(prob), columns, [c.m for c in secs], [3, 3], layer_rows=[c.layer_rows for c in secs])
    views = [dem.decoder_view(s) for s in range(2)]
    return dem, views, [L.Graph(v.indptr, v.indices, v.shape[1]) for v in views]


def test_plan_level(L):
    from qldpc_amd.simulation.dem import DemDecoder
    dem, views, graphs = _two_sector_dem(L)
    assert dem.layer_rows == (10, 12) and [v.shape[0] for v in views] == [80, 96]
    W, Cm, seed, count, max_iter = 3, 2, 20261019, 256, 12
    dets = {}

    def decode(s, g, v, synd):
        dec = L.WindowDecoder(g, dem.layer_rows[s], W, Cm, v.prior, max_iter=max_iter)
        err, conv, iters, osd, unsat = dec.decode(synd)
        nwin = dec.info()["windows"]
        dec.close()
        dets[s] = err
        return err, (conv == nwin).astype(np.uint8), int(iters.astype(np.int64).sum()), int((osd > 0).sum())

    plan = dem.plan(graphs, max_iter=max_iter, batch=128)
    plan.use_window(W, Cm)
    verdict, want = parts(L, dem, graphs, plan, seed, 0, count, max_iter, decode)
    got = plan.run_outcomes(seed, 0, count)
    tally = plan.read(clear=True)
    sampled = plan.sample(seed, 0, count)
    plan.close()
    bad = np.flatnonzero(got != verdict)
    assert bad.size == 0, f"verdicts of trials {bad[:8].tolist()} differ ({bad.size} of {count})"
    assert_tally(L, tally, want, slots=set(L.TALLY) - {"legs_z", "legs_x"})
    T = L.TALLY
    assert want[T["osd_z"]] > 0 and want[T["osd_x"]] > 0 and want[T["bp_conv_z"]] > 0 and want[T["bp_conv_x"]] > 0
    # the same trials as recorded detection events: the predicted observable flips are those of the host pieces
    events = np.concatenate([sampled[0], sampled[2]], axis=1).astype(bool)
    dd = DemDecoder(dem, maxIter=max_iter, window=(W, Cm), batch=128)
    pred = dd.decode_batch(events)
    dd.close()
    for s in range(2):
        rows = np.stack([(views[s].logmask >> np.uint64(r)) & np.uint64(1) for r in range(3)]).astype(np.int64)
        assert np.array_equal(pred[s], ((dets[s].astype(np.int64) @ rows.T) % 2).astype(bool)), f"sector {s}"
        true = sampled[2 * s + 1]
        assert np.array_equal((pred[s] != true.astype(bool)).any(axis=1), logical_errors(dets[s], views[s].logmask, true)), f"sector {s}"
