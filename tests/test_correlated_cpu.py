"""Correlated two-sector decoding without a GPU: the reweighting rule on its edge cases, the link tables of the toy model checked by hand, the decisive
behaviour on the numpy model alone (the links turn a wrong verdict into the right one), the restated storage rule, the argument rules and the binding."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import correlated_model as CM  # noqa: E402


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    return _lib


# ---------------------------------------------------------------------------------------- reweight
def test_reweight_edge_cases():
    # column 0: links from sources 0 and 4 (= n_src - 1); column 1: an empty run; column 2: one link above the base; column 3: a negative link value
    ptr, src, llr = [0, 2, 2, 3, 4], [0, 4, 2, 1], [1.5, -0.25, 9.0, -7.0]
    base = np.array([3.0, 2.0, 4.0, 0.5])
    fired = np.array([[0, 0, 0, 0, 0],        # no source fired: the base
                      [1, 0, 0, 0, 1],        # two fired links on column 0: the minimum wins
                      [1, 0, 1, 0, 0],        # source 0 alone; the link above the base leaves column 2 alone
                      [0, 1, 0, 0, 1],        # source n_src - 1 alone; the negative value
                      [2, 2, 2, 2, 2]], np.int8)      # only the value 1 fires
    P = CM.reweight(base, fired, ptr, src, llr)
    assert P.tolist() == [[3.0, 2.0, 4.0, 0.5], [-0.25, 2.0, 4.0, 0.5], [1.5, 2.0, 4.0, 0.5], [-0.25, 2.0, 4.0, -7.0], [3.0, 2.0, 4.0, 0.5]]
    per_shot = np.arange(20, dtype=np.float64).reshape(5, 4) - 6.0
    Q = CM.reweight(per_shot, fired, ptr, src, llr)
    assert Q[1].tolist() == [-2.0, -1.0, 0.0, 1.0] and Q[3].tolist() == [-0.25, 7.0, 8.0, -7.0] and Q[4].tolist() == per_shot[4].tolist()
    assert CM.reweight(base, fired, [0, 0, 0, 0, 0], [], []).tolist() == np.tile(base, (5, 1)).tolist()


# ---------------------------------------------------------------------------------------- the toy model
def test_links_of_the_toy_model_by_hand():
    from qldpc_amd.simulation import correlated
    dem = CM.toy_dem()
    v0, v1 = dem.decoder_view(0), dem.decoder_view(1)
    assert v0.shape == (2, 3) and v1.shape == (2, 4)                       # columns A C D and A B E F
    assert v1.logmask.tolist() == [1, 0, 0, 0]
    lk = correlated.links_from_dem(dem)
    assert lk.pairs() == [(0, 0, -50.0)] and lk.ptr.tolist() == [0, 1, 1, 1, 1]      # sector-0 column A -> sector-1 column A: J / P0 = 1
    assert lk.base is None and lk.unmatched == 0 and lk.n_src == 3
    cond = correlated.links_from_dem(dem, mode="condition")
    assert cond.pairs() == lk.pairs()
    # U: A reaches sector 1 only together with sector 0, so it gets the floor (the smallest positive probability, 0.01); B, E, F keep theirs
    want = [math.log((1 - p) / p) for p in (0.01, 0.03, 0.02, 0.02)]
    assert np.allclose(cond.base, want, rtol=0, atol=1e-12)
    assert np.allclose(correlated.links_from_dem(dem, mode="condition", floor=0.001).base[0], math.log(0.999 / 0.001))
    with pytest.raises(ValueError):
        correlated.links_from_dem(dem, mode="lower")
    with pytest.raises(ValueError):
        correlated.links_from_dem(dem.sector(0))


def test_links_split_the_mass_of_a_shared_source():
    """two mechanisms through one sector-0 column: the link carries J / P0, and a projection no column of an explicit view holds is counted"""
    from qldpc_amd.simulation import correlated
    from qldpc_amd.simulation.dem import DetectorErrorModel
    cols = [[([0], 0), ([0], 1)], [([0], 0), ([1], 0)], [([0], 0), ([], 0)], [([1], 0), ([0, 1], 0)]]
    dem = DetectorErrorModel.from_columns([0.01, 0.03, 0.04, 0.02], cols, (2, 2), (1, 1))
    lk = correlated.links_from_dem(dem)
    # sector-0 column 0 = {0} has mass 0.08; it leads to sector-1 column 0 with 0.01 and column 1 with 0.03
    p = [(0.01 + 0.0) / (0.01 + 0.03 + 0.04), 0.03 / (0.01 + 0.03 + 0.04), 1.0]
    want = [(0, 0, math.log((1 - p[0]) / p[0])), (0, 1, math.log((1 - p[1]) / p[1])), (1, 2, -50.0)]
    assert [(i, j) for i, j, _ in lk.pairs()] == [(i, j) for i, j, _ in want]
    assert np.allclose([v for _, _, v in lk.pairs()], [v for _, _, v in want], rtol=1e-15, atol=0)
    ev = [(correlated._key([0], 0), correlated._key([5], 0), 0.5), (correlated._key([9], 0), None, 0.5)]
    cols0 = {correlated._key([0], 0): 0}
    out = correlated.links_from_events(ev, cols0, {}, 1, 1, None)
    assert out.unmatched == 2 and out.n_links == 0


@pytest.mark.parametrize("alpha", [1.0, 0.875])
def test_the_links_decide_the_verdict_on_the_model(alpha):
    from qldpc_amd.simulation import correlated
    dem = CM.toy_dem()
    v0, v1 = dem.decoder_view(0), dem.decoder_view(1)
    lk = correlated.links_from_dem(dem)
    s0, s1 = np.array([[1, 0]], np.int8), np.array([[1, 0]], np.int8)       # the syndrome of A firing
    e0, _, c0, i0 = CM.decode(v0.indptr, v0.indices, 3, s0, v0.prior, alpha, 20.0, 50)
    assert e0.tolist() == [[1, 0, 0]] and c0[0] == 1 and i0[0] == 2         # sector 0 returns column A
    e1, _, c1, i1 = CM.decode(v1.indptr, v1.indices, 4, s1, v1.prior, alpha, 20.0, 50)
    assert e1.tolist() == [[0, 1, 0, 0]] and c1[0] == 1 and i1[0] <= 2      # alone, sector 1 returns B: the observable is predicted wrong
    P = CM.reweight(v1.prior, e0, lk.ptr, lk.src, lk.llr)
    assert P[0, 0] == -50.0 and P[0, 1:].tolist() == v1.prior[1:].tolist()
    e2, _, c2, i2 = CM.decode(v1.indptr, v1.indices, 4, s1, P, alpha, 20.0, 50)
    assert e2.tolist() == [[1, 0, 0, 0]] and c2[0] == 1 and i2[0] == 1      # reweighted, it returns A: predicted right
    assert int(v1.logmask[np.flatnonzero(e2[0])].sum()) == 1 and int(v1.logmask[np.flatnonzero(e1[0])].sum()) == 0


def test_decode_with_a_shared_prior_is_a_round_of_decimation():
    import decimation_model as DM
    rng = np.random.default_rng(7)
    n, m = 24, 12
    H = (rng.random((m, n)) < 0.2).astype(np.int8)
    ip = np.concatenate([[0], np.cumsum(H.sum(axis=1))]).astype(np.int32)
    ix = np.concatenate([np.flatnonzero(r) for r in H]).astype(np.int32)
    prior = rng.normal(2.0, 1.5, n)
    synd = (rng.random((6, m)) < 0.3).astype(np.int8)
    a = CM.decode(ip, ix, n, synd, prior, 0.875, 6.5, 9)
    b = DM.decim_decode(ip, ix, n, synd, prior, 0.875, 6.5, 9, 0, 1, 30.0)
    for x, y in zip(a, b[:4]):
        assert np.array_equal(x, y)


# ---------------------------------------------------------------------------------------- the storage rule
def test_storage_rule_has_three_modes_and_the_workload_sits_in_the_second():
    assert CM.shotprior_mode(1008, 8857, 35) == 2                          # circ144: V | SP | SI fits, P does not: the slab form is the production form
    assert CM.shotprior_lds_bytes(1008, 8857, False, True) > CM.LDS_BYTES >= CM.shotprior_lds_bytes(1008, 8857, False, False)
    assert CM.shotprior_mode(300, 4000, 10) == 1 and CM.shotprior_mode(300, 15000, 10) == 2 and CM.shotprior_mode(300, 21000, 10) == 3 and CM.shotprior_mode(6900, 64, 5) == 0
    assert CM.shotprior_mode(300, 4000, 57) == 0 and CM.shotprior_mode(300, 65535, 5) == 0 and CM.shotprior_mode(0, 5, 0) == 0
    for m in (1, 300, 1008):                                               # modes are monotone in n
        modes = [CM.shotprior_mode(m, n, 5) for n in range(1, 30000, 97)]
        assert modes == sorted(modes) and set(modes) == {1, 2, 3}


# ---------------------------------------------------------------------------------------- argument rules, no device call
CORR = dict(alpha=1.0, mode="raise")


@pytest.mark.parametrize("kw", [
    dict(decoder="relay_bp"), dict(window=(4, 2)), dict(schedule="layered"), dict(precision="f32"), dict(decimation=dict(alpha=1.0)), dict(osd_order=2),
    dict(alpha_mode="dynamical"), dict(alpha_mode="alvarado"), dict(alpha_mode="alvarado-autoregressive"), dict(alvarado_alpha=0.8),
    dict(use_dynamic_alpha=False), dict(scopt=True), dict(correlated=dict(CORR, alpha=0.0)), dict(correlated=dict(CORR, alpha=float("nan"))),
    dict(correlated=dict(CORR, mode="lower")), dict(correlated=dict(CORR, floor=0.0)), dict(correlated=dict(CORR, bogus=1)), dict(correlated=[1.0]),
    dict(correlated=True)])
def test_run_simulation_rejects_bad_combinations(L, kw, monkeypatch):
    from qldpc_amd.simulation import engine

    def no_gpu(*a, **k):
        raise AssertionError("GPU work started before the arguments were checked")
    monkeypatch.setattr(engine, "BBCodeCircuit", no_gpu)
    monkeypatch.setattr(L, "Graph", no_gpu)
    monkeypatch.setattr(L, "device_count", no_gpu)
    args = dict(correlated=CORR)
    args.update(kw)
    with pytest.raises(ValueError):
        engine.run_simulation(None, None, None, None, 0.005, num_trials=10, devices=[0], **args)


def test_extension_rules_accept_and_normalise(L):
    from qldpc_amd.simulation import engine
    for decoder, order, lsd in (("bp_osd", 0, None), ("bp_osd_cs", 7, None), ("bp_lsd", 0, {"max_rows": 64})):
        r = engine._extension_rules(order, "f64", None, "flooding", None, None, decoder, None, None, None, True, False, 50, None, lsd=lsd, correlated={})
        assert r.path == "correlated" and r.correlated == {"alpha": 1.0, "mode": "raise", "floor": None} and r.links is None
    r = engine._extension_rules(0, "f64", None, "flooding", None, None, "bp_osd", None, None, None, True, False, 50, None,
                                correlated={"alpha": 0.875, "mode": "condition", "floor": 1e-4})
    assert r.correlated == {"alpha": 0.875, "mode": "condition", "floor": 1e-4}
    r = engine._extension_rules(0, "f64", None, "flooding", None, None, "bp_osd", None, None, None, True, False, 50, None)
    assert r.path == "flooding" and r.correlated is None


def test_dem_rules(L, monkeypatch):
    from qldpc_amd.simulation import dem as D

    def no_gpu(*a, **k):
        raise AssertionError("GPU work started before the arguments were checked")
    monkeypatch.setattr(L, "Graph", no_gpu)
    toy = CM.toy_dem()
    with pytest.raises(ValueError, match="two sectors"):
        D.run_dem_simulation(toy.sector(1), num_trials=10, devices=[0], correlated=CORR)
    with pytest.raises(ValueError):
        D.DemDecoder(toy, correlated=CORR, decimation=dict(alpha=1.0))
    with pytest.raises(ValueError):
        D.DemDecoder(toy, correlated=CORR, alvarado_alpha=0.9, alpha_mode="alvarado")
    dec = D.DemDecoder(toy, correlated=CORR)                               # no device call before the first decode
    assert dec._rules.links.pairs() == [(0, 0, -50.0)]


def test_python_validation_before_any_graph(L, monkeypatch):
    from qldpc_amd.decoding import shot_prior

    def no_graph(*a, **k):
        raise AssertionError("a graph was created before the arguments were checked")
    monkeypatch.setattr(L, "Graph", no_graph)
    H = np.array([[1, 1, 0], [0, 1, 1]], np.uint8)
    for kw in (dict(alpha=0.0), dict(alpha=float("inf")), dict(clip_llr=-1.0), dict(max_iter=0), dict(max_iter=2.5)):
        with pytest.raises(ValueError):
            shot_prior.ShotPriorMinSumDecoder(H, **kw)
    with pytest.raises(ValueError):
        L.link_tables(([0, 1], [0], [1.0]), 3)
    with pytest.raises(ValueError):
        L.link_tables(([0, 1, 1, 2], [0], [1.0]), 3)
    lp, ls, ll, nl = L.link_tables(None, 3)
    assert lp.tolist() == [0, 0, 0, 0] and nl == 0 and ls.size >= 1 and ll.size >= 1


def test_null_handles_are_invalid_and_binding_follows_the_header(L):
    names = L.exports()
    for fn in ("qldpc_shotprior_decode_batch", "qldpc_shotprior_decode_batch_dev", "qldpc_circuit_plan_use_correlated"):
        assert fn in names
        getattr(L.lib(), fn)
    assert L.lib().qldpc_version() == 101
    argtypes = L.signatures()["qldpc_shotprior_decode_batch_dev"][1]
    assert len(argtypes) == 19 and all(argtypes[i] is C.c_void_p for i in (2, 3, 6, 7, 8, 9, 13, 14, 15, 16, 17, 18))
    assert len(L.signatures()["qldpc_shotprior_decode_batch"][1]) == 18
    synd, prior = np.zeros(3, np.int8), np.ones(3)
    e, c, i = np.zeros(3, np.int8), np.zeros(1, np.uint8), np.zeros(1, np.int32)
    rc = L.lib().qldpc_shotprior_decode_batch(None, 1, L.ptr(synd, C.c_int8), L.ptr(prior, C.c_double), 0, 0, None, None, None, None, 1.0, 20.0, 5,
                                              L.ptr(e, C.c_int8), None, L.ptr(c, C.c_uint8), L.ptr(i, C.c_int32), None)
    assert rc == -1 and b"graph is NULL" in L.lib().qldpc_last_error()
    assert L.lib().qldpc_shotprior_decode_batch_dev(None, 1, None, None, 0, 0, None, None, None, None, 1.0, 20.0, 5, None, None, None, None, None, None) == -1
    assert L.lib().qldpc_circuit_plan_use_correlated(None, 1.0, None, 0, None, None, None) == -1
    assert b"plan is NULL" in L.lib().qldpc_last_error()
    text = open(L.HEADER_PATH).read()
    assert "qldpc_shotprior_decode_batch[_dev] and" in text and "P[b][j] = min( prior[b * prior_stride + j]," in text
