"""LSD cluster statistics and the confidence of a trial on the MI355X: qldpc_lsd_stats_batch equals tests/lsd_stats_model.py bit for bit in all eight
words on the seeded shots of tests/lsd_shapes.py (with solution and info those of qldpc_lsd_batch), order-freedom, the device entry point; the circuit
plan's scores and histogram against the pieces put together by hand; the switch rules; run_simulation / run_dem_simulation / DemDecoder."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lsd_shapes as LS  # noqa: E402
import lsd_stats_model as SM  # noqa: E402
import osd_shapes as S  # noqa: E402
from test_relay_gpu import _bb_params, circuit_setup  # noqa: E402

pytestmark = pytest.mark.gpu

NONE = SM.NONE
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


def _weights(n, seed=7):
    """a seeded uint16 table that holds 0 and 65535"""
    w = np.random.default_rng([seed, n]).integers(0, 65536, n).astype(np.uint16)
    w[0], w[n // 2] = 0, 65535
    return w


def _held(L, key, name, shots, bps, max_rows, weighted=True):
    """library == model in all eight words on every shot; solution and info == qldpc_lsd_batch's on the same call -> (info, stats)"""
    g = _graph(L, key)
    f, G = LS.matrix(key)
    w = _weights(f.n) if weighted else None
    _, want_info, traces = LS.answers(key, name, shots, bps, max_rows)
    want = SM.stats_from_traces(G, shots, want_info, traces, w)
    sol, info, stats = L.lsd_stats_batch(g, shots.synd, shots.llr, shots.hard, bps, max_rows, w)
    sol0, info0 = L.lsd_batch(g, shots.synd, shots.llr, shots.hard, bps, max_rows)
    assert np.array_equal(sol, sol0) and np.array_equal(info, info0) and np.array_equal(info, want_info)
    for b in range(shots.synd.shape[0]):
        assert stats[b].tolist() == want[b].tolist(), f"{key}/{name} bits {bps} cap {max_rows} shot {b} (flag {info[b, 0]}): {stats[b].tolist()} vs model {want[b].tolist()}"
    assert (stats[info[:, 0] != 0] == np.uint64(NONE)).all() and (stats[:, 1][info[:, 0] == 0] == info[:, 3][info[:, 0] == 0]).all()
    return info, stats


@pytest.mark.parametrize("bps", (1, 2, 64))
@pytest.mark.parametrize("key", sorted(LS.MATRICES))
def test_general_shots(L, key, bps):
    info, stats = _held(L, key, "general", LS.general(key), bps, 128)
    assert (info[:, 0] == 0).sum() > 12 and (stats[info[:, 0] == 0][:, 0] >= 1).any()
    if key in ("ident", "tiny"):
        assert (stats[info[:, 0] == 0][:, 0] >= 2).sum() >= 5                  # several clusters to the end
    if bps == 1:
        _, bare = _held(L, key, "general", LS.general(key), bps, 128, weighted=False)      # weight == NULL: words 4 .. 6 are 0
        ok = info[:, 0] == 0
        assert not bare[ok][:, 4:7].any() and np.array_equal(bare[:, :4], stats[:, :4]) and np.array_equal(bare[:, 7], stats[:, 7])


@pytest.mark.parametrize("bps", (1, 2))
@pytest.mark.parametrize("name, key", (("single_seed", "ident"), ("merging", "dep"), ("apart", "ident"), ("duplicates", "doubled"), ("empty_rows", "tiny")))
def test_special_shots(L, name, key, bps):
    info, stats = _held(L, key, name, getattr(LS, name)(), bps, 128)
    if name == "empty_rows":
        assert (stats == np.uint64(NONE)).all()
    if name == "apart":
        assert (stats[:, 0] == 2).all()
    if name == "merging":
        assert (stats[:, 0] == 1).all()


@pytest.mark.parametrize("max_rows", (1, 64, 65))
def test_row_caps(L, max_rows):
    """capped shots carry all-ones words beside shots the cap does not stop"""
    res = [_held(L, "ident", "general", LS.general("ident"), 1, max_rows), _held(L, "ident", "single_seed", LS.single_seed(), 1, max_rows),
           _held(L, "tiny", "empty_rows", LS.empty_rows(), 1, max_rows)]
    info, stats = np.concatenate([r[0] for r in res]), np.concatenate([r[1] for r in res])
    flags = np.bincount(info[:, 0], minlength=3)
    assert flags[0] > 0 and flags[1] > 0 and flags[2] > 0
    assert (stats[info[:, 0] == 0][:, 7] <= max_rows).all()


def test_big_batch_twice(L):
    """600 shots: the ticket counter hands every workgroup a second shot, so the accumulators are zeroed again; the same batch a second time gives the
    same words (which local index a seed gets varies from run to run; the sums and maxima over clusters do not)"""
    shots = LS.general("doubled")
    rep = S.BIG_BATCH // shots.synd.shape[0]
    big = LS._shots(np.tile(shots.synd, (rep, 1)), np.tile(shots.llr, (rep, 1)), np.tile(shots.hard, (rep, 1)))
    assert big.synd.shape[0] == S.BIG_BATCH > 512
    f, G = LS.matrix("doubled")
    w = _weights(f.n)
    _, want_info, traces = LS.answers("doubled", "general", shots, 2, 128)
    want = np.tile(SM.stats_from_traces(G, shots, want_info, traces, w), (rep, 1))
    g = _graph(L, "doubled")
    first = L.lsd_stats_batch(g, big.synd, big.llr, big.hard, 2, 128, w)
    again = L.lsd_stats_batch(g, big.synd, big.llr, big.hard, 2, 128, w)
    assert np.array_equal(first[2], want) and np.array_equal(first[1], np.tile(want_info, (rep, 1)))
    for a, b in zip(first, again):
        assert np.array_equal(a, b)


def _dev_call(L, g, t, bps, max_rows, dsel, dcnt, dw, dsol, dinfo, dstats, stream=0):
    ds, dl, dh = t
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None      # noqa: E731
    return L.lib().qldpc_lsd_stats_batch_dev(g.handle, ds.shape[0], p(ds), p(dl), p(dh), bps, max_rows, p(dsel), p(dcnt), p(dw), p(dsol), p(dinfo), p(dstats),
                                             C.c_void_p(stream))


def test_dev_entry_select_list(L):
    """device pointers and a select list: the listed rows of d_stats are the host call's, the others are untouched"""
    shots = LS.general("dep")
    g = _graph(L, "dep")
    w = _weights(g.n)
    whole = L.lsd_stats_batch(g, shots.synd, shots.llr, shots.hard, 1, 64, w)
    assert set(whole[1][:, 0]) == {0, 1, 2}
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)        # noqa: E731
    ds, dl, dh, dw = t(shots.synd), t(shots.llr), t(shots.hard), t(w.view(np.int16))
    B = shots.synd.shape[0]
    sel = np.array([5, 0, 3, 11, 19, 7, 2, 23], np.int32)
    dsel, dcnt = t(sel), t(np.array([sel.size], np.int32))
    dinfo = torch.full((B, 4), -7, dtype=torch.int32, device=dev)
    dstats = torch.full((B, 8), 12345, dtype=torch.int64, device=dev)
    dsol = torch.zeros((B, g.n), dtype=torch.int8, device=dev)
    assert _dev_call(L, g, (ds, dl, dh), 1, 64, dsel, dcnt, dw, dsol, dinfo, dstats) == 0
    torch.cuda.synchronize()
    sol, info, stats = dsol.cpu().numpy(), dinfo.cpu().numpy(), dstats.cpu().numpy().view(np.uint64)
    for i in range(B):
        if i in sel:
            assert np.array_equal(sol[i], whole[0][i]) and np.array_equal(info[i], whole[1][i]) and np.array_equal(stats[i], whole[2][i]), i
        else:
            assert not sol[i].any() and (info[i] == -7).all() and (stats[i] == 12345).all(), i
    # refusals: those of qldpc_lsd_batch_dev, plus stats == NULL
    assert _dev_call(L, g, (ds, dl, dh), 1, 64, dsel, dcnt, dw, dsol, dinfo, None) == -1 and b"stats" in L.lib().qldpc_last_error()
    assert _dev_call(L, g, (ds, dl, dh), 1, 64, dsel, None, dw, dsol, dinfo, dstats) == -1
    assert _dev_call(L, g, (ds, dl, dh), 65, 64, None, None, dw, dsol, dinfo, dstats) == -1
    sol_, info_, st_ = np.zeros((B, g.n), np.int8), np.zeros((B, 4), np.int32), np.zeros((B, 8), np.uint64)
    raw = lambda stats, rows=64: L.lib().qldpc_lsd_stats_batch(g.handle, B, L.ptr(shots.synd, C.c_int8), L.ptr(shots.llr, C.c_double),      # noqa: E731
                                                                L.ptr(shots.hard, C.c_int8), 1, rows, None, L.ptr(sol_, C.c_int8), L.ptr(info_, C.c_int32), stats)
    assert raw(None) == -1 and raw(L.ptr(st_, C.c_uint64), 1025) == -1 and raw(L.ptr(st_, C.c_uint64)) == 0
    with pytest.raises(ValueError):
        L.lsd_stats_batch(g, shots.synd, shots.llr, shots.hard, 1, 64, w[:-1])


def test_two_streams_and_two_threads(L):
    """the same batch on two streams from two threads: identical words (no lane or seed-index order enters)"""
    shots = LS.general("ident")
    g = _graph(L, "ident")
    w = _weights(g.n)
    alone = L.lsd_stats_batch(g, shots.synd, shots.llr, shots.hard, 2, 128, w)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)        # noqa: E731
    tens, dw = (t(shots.synd), t(shots.llr), t(shots.hard)), t(w.view(np.int16))
    B = shots.synd.shape[0]
    outs = [(torch.zeros((B, g.n), dtype=torch.int8, device=dev), torch.zeros((B, 4), dtype=torch.int32, device=dev),
             torch.zeros((B, 8), dtype=torch.int64, device=dev)) for _ in range(2)]
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    torch.cuda.synchronize()
    rcs = {}

    def enqueue(k):
        rcs[k] = _dev_call(L, g, tens, 2, 128, None, None, dw, outs[k][0], outs[k][1], outs[k][2], streams[k].cuda_stream)
    ts = [threading.Thread(target=enqueue, args=(k,)) for k in range(2)]
    for th in ts:
        th.start()
    for th in ts:
        th.join()
    assert rcs == {0: 0, 1: 0}
    torch.cuda.synchronize()
    for dsol, dinfo, dstats in outs:
        assert np.array_equal(dsol.cpu().numpy(), alone[0]) and np.array_equal(dinfo.cpu().numpy(), alone[1])
        assert np.array_equal(dstats.cpu().numpy().view(np.uint64), alone[2])


def test_lsd_decoder_return_stats(L):
    from qldpc_amd.decoding.lsd import LsdDecoder
    f, _ = LS.matrix("ident")
    shots = LS.general("ident")
    import scipy.sparse as sp
    H = sp.csr_matrix((np.ones(f.indices.size, np.int8), f.indices, f.indptr), shape=(f.m, f.n))
    dec = LsdDecoder(H, bits_per_step=2, max_rows=128)
    w = _weights(f.n)
    want = L.lsd_stats_batch(_graph(L, "ident"), shots.synd, shots.llr, shots.hard, 2, 128, w)
    got = dec.decode(shots.synd, shots.llr, shots.hard, weights=w, return_stats=True)
    one = dec.decode(shots.synd[5], shots.llr[5], shots.hard[5], weights=w, return_stats=True)
    plain = dec.decode(shots.synd, shots.llr, shots.hard)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)) and all(np.array_equal(a, b[5]) for a, b in zip(one, want))
    assert len(plain) == 2 and np.array_equal(plain[0], want[0])


# ---------------------------------------------------------------------------------------------------------------- the circuit plan
_HAND = {}


def _by_hand(L, tag, seed, count, bps, max_rows):
    """sampler -> BP -> qldpc_lsd_stats_batch on the unconverged shots -> numpy judge: (verdict uint8[count], statistics uint64[count, 8] per sector with
    zero rows where BP converged, osd counts, flag counts), through the C ABI piece by piece; computed once per case"""
    k = (tag, seed, count, bps, max_rows)
    if k in _HAND:
        return _HAND[k]
    c, compiled, Mx, graphs, priors, masks, plan = circuit_setup(L, tag)
    p = plan(batch=count)
    spz, tz, spx, tx = p.sample(seed, 0, count)
    p.close()
    verdict = np.zeros(count, np.uint8)
    stats, osd, flags = [], [], []
    for sec, (g, prior, mask, synd, true) in enumerate(((graphs[0], priors[0], masks[0], spz, tz), (graphs[1], priors[1], masks[1], spx, tx))):
        det, conv, llr, iters = L.minsum_decode_batch(g, synd, prior, 50, "dynamical", 1.0)
        bad = np.flatnonzero(conv == 0)
        st = np.zeros((count, 8), np.uint64)
        det[bad], info, st[bad] = L.lsd_stats_batch(g, synd[bad], llr[bad], det[bad], bps, max_rows, L.quantise_weights(prior))
        rows = np.stack([(mask >> np.uint64(r)) & np.uint64(1) for r in range(true.shape[1])]).astype(np.int64)
        dec = (det.astype(np.int64) @ rows.T) % 2
        verdict |= (np.any(dec != true.astype(np.int64), axis=1).astype(np.uint8) << sec)
        stats.append(st)
        osd.append(int(bad.size))
        flags.append(np.bincount(info[:, 0], minlength=3))
    _HAND[k] = (verdict, stats, osd, np.stack(flags))
    return _HAND[k]


EDGES = np.array([1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 256, 512, 1024, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20, 1 << 24, 1 << 28, 1 << 32,
                  1 << 40, 1 << 48, 1 << 56], np.uint64)


@pytest.mark.parametrize("bps, max_rows", ((1, 512), (4, 24)))
def test_circuit_plan_matches_the_pieces(L, bps, max_rows):
    count, seed = 2048, 9876
    verdict, stats, osd, flags = _by_hand(L, "circ72", seed, count, bps, max_rows)
    c, compiled, Mx, graphs, priors, masks, plan = circuit_setup(L, "circ72")
    wz, wx = (L.quantise_weights(p) for p in priors)
    T = L.TALLY
    ref = plan(batch=1024)                                                        # the unswitched LSD plan
    ref.use_lsd(bps, max_rows)
    ref_out, ref_tally, ref_counts = ref.run_outcomes(seed, 0, count), ref.read(), ref.lsd_counts()
    ref.close()
    assert np.array_equal(ref_out, verdict)
    got = {}
    for batch in (1024, 256):
        p = plan(batch=batch)
        p.use_lsd(bps, max_rows)
        for kind in SM.KINDS:
            p.use_confidence(kind, EDGES, wz, wx)                                 # (again with new arguments: the histogram starts at zero)
            p.read(clear=True)
            p.lsd_counts(clear=True)
            out, score = p.run_scores(seed, 0, count)
            want = SM.scores(kind, stats[0], stats[1])
            assert np.array_equal(out, verdict) and np.array_equal(score, want), (kind, batch)
            hist = p.confidence_hist()
            assert np.array_equal(hist, SM.histogram(want, verdict, EDGES)), (kind, batch)
            tally, counts = p.read(), p.lsd_counts()
            assert np.array_equal(tally, ref_tally) and np.array_equal(counts, ref_counts) and np.array_equal(counts, flags)
            col = hist.sum(axis=0)
            assert int(col.sum()) == tally[T["trials"]] == count and int(col[1] + col[3]) == tally[T["z_err"]] and int(col[2] + col[3]) == tally[T["x_err"]]
            assert int(col[1:].sum()) == tally[T["total_err"]]
            got[(kind, batch)] = (score, hist)
            silent = (score == np.uint64(NONE)).sum()
            assert silent == ((stats[0][:, 0] == np.uint64(NONE)) | (stats[1][:, 0] == np.uint64(NONE))).sum() == hist[-1].sum() and (score > 0).sum() > silent
            if max_rows == 24:
                assert silent > 0                                                 # the small cap: some trials land in the last bin with no statement
        # a range split over calls, and plain run / run_outcomes, fill the same histogram
        p.use_confidence("llr_2", EDGES, wz, wx)
        a = p.run_scores(seed, 0, 700)
        b = p.run_scores(seed, 700, count - 700)
        assert np.array_equal(np.concatenate([a[1], b[1]]), got[("llr_2", batch)][0]) and np.array_equal(p.confidence_hist(clear=True), got[("llr_2", batch)][1])
        p.run(seed, 0, 1000)
        assert np.array_equal(p.run_outcomes(seed, 1000, count - 1000), verdict[1000:]) and np.array_equal(p.confidence_hist(), got[("llr_2", batch)][1])
        p.close()
    for kind in SM.KINDS:
        assert np.array_equal(got[(kind, 1024)][0], got[(kind, 256)][0]) and np.array_equal(got[(kind, 1024)][1], got[(kind, 256)][1])
    assert [ref_tally[T["osd_z"]], ref_tally[T["osd_x"]]] == osd and min(osd) > 0


def test_plan_switch_rules(L):
    c, compiled, Mx, graphs, priors, masks, plan = circuit_setup(L, "circ72")
    wz, wx = (L.quantise_weights(p) for p in priors)

    def refused(p, call, match):
        with pytest.raises(L.QldpcError, match=match):
            call(p)
        p.close()
    conf = lambda p: p.use_confidence("llr_2", EDGES, wz, wx)                 # noqa: E731
    refused(plan(batch=256), conf, "BP \\+ OSD-0: a confidence needs BP \\+ LSD")          # before use_lsd
    refused(plan(batch=256, use_osd=False), conf, "use_osd = 0")
    for first, match in ((lambda p: p.use_osd_cs(7), "BP \\+ OSD-CS"), (lambda p: p.use_relay(), "Relay-BP"), (lambda p: p.use_window(3, 1), "sliding-window")):
        p = plan(batch=256)
        first(p)
        refused(p, conf, match)
    p = plan(batch=256)
    p.use_lsd()
    raw = lambda kind, nbins, edges, z=wz, x=wx: L.lib().qldpc_circuit_plan_use_confidence(      # noqa: E731
        p.handle, kind, nbins, L.ptr(edges, C.c_uint64) if edges is not None else None, L.ptr(z, C.c_uint16) if z is not None else None,
        L.ptr(x, C.c_uint16) if x is not None else None)
    two = np.array([5, 5], np.uint64)
    assert raw(6, 3, EDGES[:2]) == -1 and raw(-1, 3, EDGES[:2]) == -1 and raw(0, 0, None) == -1 and raw(0, 4097, EDGES) == -1 and raw(0, 3, None) == -1
    assert raw(0, 3, two) == -1 and b"edges[1]" in L.lib().qldpc_last_error()
    assert raw(3, 3, EDGES[:2], None, wx) == -1 and raw(4, 3, EDGES[:2], wz, None) == -1 and b"weight_x" in L.lib().qldpc_last_error()
    assert raw(0, 3, EDGES[:2], None, None) == 0 and raw(2, 1, None, None, None) == 0          # the COLS kinds go without weights; one bin without edges
    with pytest.raises(L.QldpcError):
        L.CircuitPlan.confidence_hist(plan_without := plan(batch=256))
    hist = np.zeros((1, 4), np.uint64)
    assert L.lib().qldpc_circuit_plan_confidence_read(plan_without.handle, None, 0, L.ptr(hist, C.c_uint64)) == -1
    out, sc = np.zeros(4, np.uint8), np.zeros(4, np.uint64)
    assert L.lib().qldpc_circuit_plan_run_scores(plan_without.handle, 1, 0, 4, None, L.ptr(out, C.c_uint8), L.ptr(sc, C.c_uint64)) == -1
    plan_without.close()
    p.close()

    # what stays open: either order with layered, decimation and f32; a second call clears the histogram
    def result(p):
        out, score = p.run_scores(11, 0, 512)
        res = (out, score, p.confidence_hist(), p.read(), p.lsd_counts())
        p.close()
        return res
    for path in (lambda p: p.use_layered(), lambda p: p.use_decimation(), lambda p: p.use_f32()):
        p, q = plan(batch=256), plan(batch=256)
        p.use_lsd()
        conf(p)
        path(p)
        q.use_lsd()
        path(q)
        conf(q)
        rp, rq = result(p), result(q)
        assert all(np.array_equal(a, b) for a, b in zip(rp, rq)) and rp[2].sum() == 512 and rp[4].sum() > 0
    p = plan(batch=256)
    p.use_lsd()
    conf(p)
    p.run(11, 0, 512)
    first = p.confidence_hist()
    assert first.sum() == 512 and np.array_equal(p.confidence_hist(clear=True), first) and not p.confidence_hist().any()
    p.run(11, 0, 300)
    conf(p)                                                                       # a second call clears the histogram
    assert not p.confidence_hist().any()
    p.use_lsd(4, 16)                                                              # LSD again with new parameters keeps the confidence
    p.run(11, 0, 512)
    assert p.confidence_hist().sum() == 512 and p.confidence_hist()[-1].sum() > 0
    p.close()


def test_run_simulation_and_dem_decoder(L):
    from qldpc_amd.data import load_code, load_precomputed_matrices
    from qldpc_amd.simulation.dem import DemDecoder, DetectorErrorModel, run_dem_simulation
    from qldpc_amd.simulation.engine import run_simulation
    from qldpc_amd.simulation.postselect import PostSelection, default_edges
    c = load_code("bb72")
    mats = load_precomputed_matrices("circ72")
    kw = dict(num_cycles=6, precomputed_matrices=mats, base_seed=2026, batch=1024, decoder="bp_lsd", **_bb_params(c))
    run = lambda **more: run_simulation(c["Hx"], c["Hz"], c["Lx"], c["Lz"], 0.005, num_trials=2048, **dict(kw, **more))      # noqa: E731
    r0 = run(devices=[0])
    r1 = run(devices=[0], post_select={"kind": "llr_2"})
    r2 = run(devices=[0, 0], post_select={"kind": "llr_2", "edges": None})
    T = L.TALLY
    ps = r1["post_selection"]
    assert "post_selection" not in r0 and isinstance(ps, PostSelection) and ps.kind == "llr_2" and np.array_equal(ps.edges, default_edges("llr_2"))
    assert np.array_equal(ps.hist, r2["post_selection"].hist) and np.array_equal(r1["tally"], r2["tally"]) and np.array_equal(r1["tally"], r0["tally"])
    col = ps.hist.sum(axis=0)
    assert ps.trials == 2048 and int(col[1:].sum()) == r1["tally"][T["total_err"]] and int(col[1] + col[3]) == r1["tally"][T["z_err"]]
    assert ps.hist[0].sum() > 0 and ps.hist[1:].sum() > 0                         # bin 0: no cluster at all
    curve = ps.curve()
    assert curve["ler"][-1] == r1["logical_error_rate"] and ps.at_abort_rate(0.0)["accepted"] == 2048
    r3 = run(devices=[0], post_select={"kind": "cols_inf", "edges": [1, 5, 40]})
    assert r3["post_selection"].hist.shape == (4, 4) and r3["post_selection"].trials == 2048
    for bad in (dict(decoder="bp_osd", post_select={"kind": "llr_2"}), dict(post_select={"kind": "llr_2"}, target_logical_errors=3),
                dict(post_select={"kind": "llr_2", "edges": [4, 4]})):
        with pytest.raises(ValueError):
            run_simulation(c["Hx"], c["Hz"], c["Lx"], c["Lz"], 0.005, num_trials=8, devices=[0], **dict(kw, **bad))
    dem = DetectorErrorModel.from_decoding_matrices("circ72", layer_rows=36)
    par = {"bits_per_step": 2, "max_rows": 256}
    d1 = run_dem_simulation(dem, num_trials=2048, base_seed=5, batch=1024, devices=[0], decoder="bp_lsd", lsd=par, post_select={"kind": "cols_1"})
    d2 = run_dem_simulation(dem, num_trials=2048, base_seed=5, batch=1024, devices=[0, 0], decoder="bp_lsd", lsd=par, post_select={"kind": "cols_1"})
    assert np.array_equal(d1["post_selection"].hist, d2["post_selection"].hist) and d1["post_selection"].trials == 2048
    assert int(d1["post_selection"].hist[:, 1:].sum()) == d1["tally"][T["total_err"]]
    # DemDecoder(confidence=) == decode_events(scores=True) on a plan switched by hand; predictions and flags are the unscored call's
    count, seed = 512, 5
    views = [dem.decoder_view(0), dem.decoder_view(1)]
    plan = dem.plan([L.Graph(v.indptr, v.indices, v.shape[1]) for v in views], max_iter=50, batch=128)
    spz, _, spx, _ = plan.sample(seed, 0, count)
    events = np.hstack([spz, spx]).astype(np.uint8)
    plan.use_lsd(**par)
    unscored = plan.decode_events(L.pack_events(events), seed, 0)
    with pytest.raises(L.QldpcError):
        plan.decode_events(L.pack_events(events), seed, 0, scores=True)           # no confidence yet
    plan.use_confidence("llr_2", None, *(L.quantise_weights(v.prior) for v in views))
    want = plan.decode_events(L.pack_events(events), seed, 0, scores=True)
    assert not plan.confidence_hist().any()                                       # recorded events have no outcome: the histogram is left alone
    # ... and the score of a shot is that of the trial it was sampled as
    out, score = plan.run_scores(seed, 0, count)
    plan.close()
    assert all(np.array_equal(a, b) for a, b in zip(want[:3], unscored)) and np.array_equal(want[3], score) and (score > 0).any()
    dec = DemDecoder(dem, decoder="bp_lsd", lsd=par, batch=200, seed=seed, confidence="llr_2")
    (a0, a1), conf = dec.decode_batch(events, return_confidence=True)
    b0, b1 = dec.decode_batch(events)
    flags = dec.decode_to_flags(events)[1]
    dec.close()
    bits = lambda v, k: ((v[:, None] >> np.arange(k, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)      # noqa: E731
    assert np.array_equal(conf, want[3]) and np.array_equal(a0, bits(want[0], dem.k[0])) and np.array_equal(a1, bits(want[1], dem.k[1]))
    assert np.array_equal(a0, b0) and np.array_equal(a1, b1) and np.array_equal(flags, want[2])
