"""Soft readout without a GPU: the cuts and level flip probabilities of hand-worked channels, the Gaussian masses against an independent erfc
evaluation, the decoder tables of simulation/soft.py on a hand-made circuit -- by hand, against the product formula and against the numpy model --
the prior rule, marginal_priors, the table validation of qldpc_soft_priors (it runs before any device call), the argument rules of
run_simulation(soft=...), the refusals of the strata and DEM entry points and the binding."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import soft_model as SM  # noqa: E402
from soft_model import OP_MEAS_X, OP_MEAS_Z  # noqa: E402


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def S():
    from qldpc_amd.simulation import soft
    return soft


# ---------------------------------------------------------------------------------------- 1. the channel
def test_cuts_and_flip_probabilities_by_hand(S):
    h = S.SoftReadout.hard(0.25)                                           # K = 1: one cut, and the closing 2^32
    assert h.levels == 1 and h.cut == [1 << 30, 1 << 32] and h.q.tolist() == [0.25] and h.qbar == 0.25
    z = S.SoftReadout([1, 0, 1], [1, 2, 3])                                # K = 3, sum 8, flipped level 1 has no mass: it never flips
    u = 1 << 29
    assert z.levels == 3 and z.cut == [u, u, 2 * u, 3 * u, 5 * u, 8 * u]
    assert z.q.tolist() == [0.5, 0.0, 0.25] and z.qbar == 0.25
    w = S.SoftReadout([1] * 16, [3] * 16)                                  # K = 16, sum 64
    v = 1 << 26
    assert w.levels == 16 and w.cut == [(b + 1) * v for b in range(16)] + [16 * v + 3 * (b + 1) * v for b in range(16)]
    assert w.q.tolist() == [0.25] * 16 and w.qbar == 0.25
    k = S.SoftReadout([2, 1], [0, 5])                                      # a kept level without mass: that level always flips
    assert k.q.tolist() == [1.0, 1 / 6] and k.cut[-1] == 1 << 32
    for r in (h, z, w, k, S.SoftReadout.gaussian(0.5, 8), S.SoftReadout([0.3, 1e-3, 7.0], [5.0, 0.11, 1e-9])):      # and the model agrees, floor and all
        assert r.cut == SM.cuts(r.flip_mass, r.keep_mass) and np.array_equal(r.q, SM.level_flip_probs(r.cut))
        assert all(a <= b for a, b in zip(r.cut, r.cut[1:])) and r.qbar == r.cut[r.levels - 1] / 2 ** 32


@pytest.mark.parametrize("sigma,K", [(0.5, 8), (0.3, 3), (0.8, 16), (0.4, 1)])
def test_gaussian_masses(S, sigma, K):
    r = S.SoftReadout.gaussian(sigma, K)
    flip, keep = SM.gaussian_masses(sigma, K)
    assert r.levels == K
    assert np.allclose(r.flip_mass, flip, rtol=1e-9, atol=1e-15) and np.allclose(r.keep_mass, keep, rtol=1e-9, atol=1e-15)
    assert abs(r.flip_mass.sum() + r.keep_mass.sum() - 1.0) <= 1e-14
    assert abs(r.flip_mass.sum() - 0.5 * math.erfc(1 / (sigma * math.sqrt(2)))) <= 1e-15         # P(y < 0)
    assert (np.diff(r.q) < 0).all() and r.q[0] < 0.5                        # level 0 is the least confident
    e = [0.0, 0.1, 0.5][:K] if K <= 3 else None
    if e is not None:
        r2 = S.SoftReadout.gaussian(sigma, K, edges=e)
        f2, k2 = SM.gaussian_masses(sigma, K, e)
        assert np.allclose(r2.flip_mass, f2, rtol=1e-9, atol=1e-15) and np.allclose(r2.keep_mass, k2, rtol=1e-9, atol=1e-15)


def test_bad_channels_raise(S):
    R = S.SoftReadout
    for flip, keep in (([], []), ([0.1] * 17, [0.9] * 17), ([0.1, 0.1], [0.8]), ([-0.1], [1.0]), ([float("nan")], [1.0]), ([0.1], [float("inf")]),
                       ([0.0, 0.0], [0.0, 0.0]), ([0.0, 1.0], [0.0, 1.0]), ([1e-30, 0.1], [1e-30, 0.9]), ([[0.1]], [[0.9]])):
        with pytest.raises(ValueError):
            R(flip, keep)
    with pytest.raises(ValueError, match="level 0 has no mass"):
        R([0.0, 1.0], [0.0, 1.0])
    with pytest.raises(ValueError, match=r"keep_mass\[1\]"):
        R([0.1, 0.1], [0.5, -1.0])
    for sigma, K, e in ((0.0, 8, None), (-1.0, 8, None), (float("nan"), 8, None), ("0.4", 8, None), (0.4, 0, None), (0.4, 17, None), (0.4, 3, [0.0, 0.5]),
                        (0.4, 3, [0.1, 0.5, 1.0]), (0.4, 3, [0.0, 0.5, 0.5])):
        with pytest.raises(ValueError):
            R.gaussian(sigma, K, e)
    for q in (-0.1, 1.5, "x"):
        with pytest.raises(ValueError):
            R.hard(q)


# ---------------------------------------------------------------------------------------- 2. a hand-made circuit: 3 locations, 3 detectors per sector, k = 1
OPS = [OP_MEAS_X, OP_MEAS_Z, OP_MEAS_X]
E = ((), 0)
SIG_Z = [((0,), 0), E,   ((1,), 1), E,   ((0,), 0), E]                     # (detectors, logical mask) of (slot 0, slot 1) per location
SIG_X = [((2,), 0), E,   ((1,), 1), E,   E, E]
COLS_Z = [((1,), 1), ((0,), 0), ((2,), 0)]                                 # column 1 takes both MeasX locations
COLS_X = [((0,), 0), ((2,), 0), ((1,), 1)]
PROBS_Z, PROBS_X = np.array([0.01, 0.02, 0.004]), np.array([0.015, 0.002, 0.01])
OPS_B = [OP_MEAS_X, OP_MEAS_X, OP_MEAS_Z]                                  # a second one: an empty projection and one no column holds
SIG_ZB = [E, E,   ((0, 2), 0), E,   ((0,), 0), E]
SIG_XB = [E, E,   E, E,   ((0,), 0), E]


def sig_table(sig):
    ptr, idx = [0], []
    for dets, _ in sig:
        idx += list(dets)
        ptr.append(len(idx))
    return np.array(ptr, np.int32), np.array(idx, np.uint16), np.array([m for _, m in sig], np.uint64)


def matrices():
    M = {}
    for s, cols, probs in (("Z", COLS_Z, PROBS_Z), ("X", COLS_X, PROBS_X)):
        H, Lg = np.zeros((3, len(cols)), np.uint8), np.zeros((1, len(cols)), np.uint8)
        for j, (dets, mask) in enumerate(cols):
            H[list(dets), j] = 1
            Lg[0, j] = mask
        M.update({f"Hdec{s}": H, f"H{s}_logical": Lg, f"channel_probs{s}": probs})
    return M


def make(S, readout, ops=OPS, sigs=(SIG_Z, SIG_X)):
    return S.soft_tables_from_circuit({"base_ops": np.array(ops)}, np.zeros((1, 2)), np.zeros((1, 2)), matrices(), readout,
                                      signatures=(sig_table(sigs[0]), sig_table(sigs[1])))


@pytest.fixture(scope="module")
def readout(S):
    return S.SoftReadout([1, 0, 1], [1, 2, 3])                             # q = 1/2, 0, 1/4


def test_tables_by_hand(S, readout):
    tz, tx = make(S, readout)
    assert tz.meas_col.tolist() == [1, -1, 1] and tz.meas_w[[0, 2]].tolist() == [1, 3]      # mixed radix: the second measurement of column 1 weighs K
    assert tx.meas_col.tolist() == [-1, 2, -1] and tx.meas_w[1] == 1
    assert (tz.n_meas, tz.n, tx.n_meas, tx.n, tz.levels) == (3, 3, 3, 3, 3) and tz.unmatched == tx.unmatched == 0
    assert np.diff(tz.lut_ptr).tolist() == [1, 9, 1] and np.diff(tx.lut_ptr).tolist() == [1, 1, 3]
    assert tz.measurements(1) == [0, 2] and tx.measurements(2) == [1]
    from qldpc_amd.simulation.engine import prior_llrs
    assert np.array_equal(tz.lut[[0, 10]], prior_llrs(PROBS_Z[[0, 2]])) and np.array_equal(tx.lut[[0, 1]], prior_llrs(PROBS_X[[0, 1]]))      # length 1: verbatim
    q = [0.5, 0.0, 0.25]
    for a in range(3):                                                     # the product formula
        for b in range(3):
            f = (1 - (1 - 2 * 0.02) * (1 - 2 * q[a]) * (1 - 2 * q[b])) / 2
            assert abs(tz.lut[1 + a + 3 * b] - math.log((1 - f) / f)) <= 1e-12, (a, b)
        f = (1 - (1 - 2 * 0.01) * (1 - 2 * q[a])) / 2
        assert abs(tx.lut[2 + a] - math.log((1 - f) / f)) <= 1e-12
    assert tz.lut[1] == 0.0 and abs(tz.lut[1 + 1 + 3 * 1] - prior_llrs(np.float64(0.02))) <= 1e-12      # a level-0 readout is a coin; two level-1 readouts change nothing
    tz, tx = make(S, readout, OPS_B, (SIG_ZB, SIG_XB))
    assert tz.meas_col.tolist() == [-1, -1, -1] and tz.unmatched == 1       # empty: not counted; ({0, 2}, 0): no column
    assert tx.meas_col.tolist() == [-1, -1, 0] and tx.unmatched == 0


@pytest.mark.parametrize("which", ["zero-mass", "gaussian", "hard", "sixteen"])
def test_tables_equal_the_model(S, readout, which):
    r = {"zero-mass": readout, "gaussian": S.SoftReadout.gaussian(0.5, 8), "hard": S.SoftReadout.hard(0.02), "sixteen": S.SoftReadout([1] * 16, [3] * 16)}[which]
    M = matrices()
    for ops, sigs in ((OPS, (SIG_Z, SIG_X)), (OPS_B, (SIG_ZB, SIG_XB))):
        tables = make(S, r, ops, sigs)
        for s, probs in enumerate((PROBS_Z, PROBS_X)):
            name = "ZX"[s]
            want = SM.build_tables(ops, sig_table(sigs[s]), bool(s), SM.columns_of(M[f"Hdec{name}"], M[f"H{name}_logical"][0]), 3, probs, r.cut)
            for k in ("meas_col", "meas_w", "lut_ptr", "lut"):
                assert np.array_equal(getattr(tables[s], k), want[k]), (s, k)
            assert tables[s].unmatched == want["unmatched"] and tables[s].levels == want["levels"]


def test_a_run_above_65536_entries_raises(S):
    with pytest.raises(ValueError, match="column 0 has 5 measurements"):
        S.tables_from_columns([0] * 5, 2, np.array([0.01, 0.01]), S.SoftReadout([1] * 16, [3] * 16))
    t = S.tables_from_columns([0] * 4, 2, np.array([0.01, 0.01]), S.SoftReadout([1] * 16, [3] * 16))
    assert np.diff(t.lut_ptr).tolist() == [65536, 1] and t.meas_w.tolist() == [1, 16, 256, 4096]


def test_prior_rule_on_the_model(S, readout):
    tz, tx = make(S, readout)
    levels = np.array([[0, 0, 0], [2, 1, 1], [1, 2, 2], [2, 0, 2]], np.uint8)
    Pz, Px = SM.priors(levels, tz), SM.priors(levels, tx)
    assert Pz[:, 1].tolist() == [tz.lut[1], tz.lut[1 + 2 + 3], tz.lut[1 + 1 + 6], tz.lut[1 + 8]]
    assert (Pz[:, 0] == tz.lut[0]).all() and (Pz[:, 2] == tz.lut[10]).all()
    assert Px[:, 2].tolist() == [tx.lut[2], tx.lut[3], tx.lut[4], tx.lut[2]]


def test_marginal_priors(S, readout):
    from qldpc_amd.simulation.engine import prior_llrs
    tables = make(S, readout)
    mz, mx = S.marginal_priors(matrices(), tables, readout)
    assert readout.qbar == 0.25
    assert np.array_equal(mz[[0, 2]], prior_llrs(PROBS_Z[[0, 2]])) and np.array_equal(mx[[0, 1]], prior_llrs(PROBS_X[[0, 1]]))      # no measurement: verbatim
    f = 0.02
    for _ in range(2):                                                     # p (+) qbar, once per measurement
        f = f * (1 - 0.25) + 0.25 * (1 - f)
    assert abs(mz[1] - math.log((1 - f) / f)) <= 1e-12
    f = 0.01 * 0.75 + 0.25 * 0.99
    assert abs(mx[2] - math.log((1 - f) / f)) <= 1e-12
    assert np.array_equal(mz, SM.marginal_priors(PROBS_Z, tables[0].meas_col, readout.qbar))
    assert np.array_equal(mx, SM.marginal_priors(PROBS_X, tables[1].meas_col, readout.qbar))
    h = S.SoftReadout.hard(0.25)                                           # K = 1: the only lut entry of a measured column IS the marginal prior
    th = make(S, h)
    assert np.array_equal(th[0].lut, S.marginal_priors(matrices(), th, h)[0])


# ---------------------------------------------------------------------------------------- 3. the library's table validation: no device is touched
def test_malformed_tables_are_refused_with_the_index_named(L, S, readout):
    tz = make(S, readout)[0]
    mc, mw, up, lu, K = SM.as_tuple(tz)
    levels = np.zeros((2, 3), np.uint8)

    def refused(t, text, lv=levels):
        with pytest.raises(L.QldpcError, match="error -1") as ei:
            L.soft_priors(lv, t)
        assert text in str(ei.value), str(ei.value)

    def put(a, i, v):
        a = a.copy()
        a[i] = v
        return a
    refused((put(mc, 2, 3), mw, up, lu, K), "meas_col[2] = 3 is outside -1..2")
    refused((put(mc, 0, -2), mw, up, lu, K), "meas_col[0] = -2 is outside -1..2")
    refused((mc, put(mw, 2, 1), up, lu, K), "meas_w[2] = 1")
    refused((mc, put(mw, 0, 3), up, lu, K), "meas_w[0] = 3")
    refused((mc, mw, put(up, 0, 1), lu, K), "lut_ptr[0] = 1")
    refused((put(mc, 2, -1), mw, up, lu, K), "lut_ptr[2] - lut_ptr[1] = 9, but column 1 has a run of 3 entries")
    refused((mc, mw, up, put(lu, 5, np.inf), K), "lut[5] is not finite")
    refused((mc, mw, up, put(lu, 0, np.nan), K), "lut[0] is not finite")
    refused((mc, mw, up, lu, 0), "levels = 0 is outside 1..16")
    refused((mc, mw, up, lu, 17), "levels = 17 is outside 1..16")
    refused((mc, mw, up, lu, K), "level[1][2] = 3 is not below levels = 3 (shot 1, measurement 2)", put(levels, (1, 2), 3))
    five = (np.zeros(5, np.int32), 16 ** np.arange(5, dtype=np.int32), np.array([0, 16 ** 5], np.int32), np.zeros(16 ** 5), 16)
    refused(five, "column 0: measurement 4 brings its run to 1048576 entries", np.zeros((1, 5), np.uint8))
    with pytest.raises(ValueError):
        L.soft_priors(np.zeros((1, 2), np.uint8), (mc, mw, up, lu, K))      # three levels per shot expected
    with pytest.raises(ValueError):
        L.soft_table_args((mc, mw[:2], up, lu, K))
    with pytest.raises(ValueError):
        L.soft_table_args((mc, mw, up, lu, 3.0))


# ---------------------------------------------------------------------------------------- 4. argument rules
def rules(engine, soft, **kw):
    a = dict(osd_order=0, precision="f64", decimation=None, schedule="flooding", layers=None, window=None, decoder="bp_osd", relay_params=None,
             alpha_mode=None, alvarado_alpha=None, use_dynamic_alpha=True, scopt=False, lsd=None, correlated=None, erasure=None)
    a.update(kw)
    return engine._extension_rules(a["osd_order"], a["precision"], a["decimation"], a["schedule"], a["layers"], a["window"], a["decoder"], a["relay_params"],
                                   a["alpha_mode"], a["alvarado_alpha"], a["use_dynamic_alpha"], a["scopt"], 50, None, lsd=a["lsd"], correlated=a["correlated"],
                                   erasure=a["erasure"], soft=soft)


OTHER_PATHS = (dict(precision="f32"), dict(decimation={}), dict(schedule="layered"), dict(window=(4, 2)), dict(decoder="relay_bp"), dict(correlated={}),
               dict(erasure={"rates": 0.01}))


def test_extension_rules(S):
    from qldpc_amd.simulation import engine
    r = rules(engine, {"sigma": 0.4})
    assert r.path == "soft" and r.soft["aware"] is True and r.soft["alpha"] == 1.0 and r.soft["readout"].levels == 8 and r.soft_tables is None
    assert r.soft["readout"].cut == S.SoftReadout.gaussian(0.4, 8).cut
    own = S.SoftReadout.hard(0.02)
    r = rules(engine, {"readout": own, "aware": True, "alpha": 0.875})
    assert r.path == "soft" and r.soft["alpha"] == 0.875 and r.soft["readout"] is own
    assert rules(engine, {"sigma": 0.4, "levels": 4, "edges": [0, 0.3, 0.6, 0.9]}).soft["readout"].levels == 4
    for other in OTHER_PATHS:                                              # aware is a path: it goes with none of the others ...
        with pytest.raises(ValueError, match="does not go with"):
            rules(engine, {"sigma": 0.4, "aware": True}, **other)
    for other in OTHER_PATHS[:-1]:                                         # ... unaware is the sampler axis: it goes with each decode path
        u = rules(engine, {"sigma": 0.4, "aware": False}, **other)
        assert u.path != "soft" and u.path != "flooding" and u.soft["aware"] is False
    with pytest.raises(ValueError, match="does not go with erasure"):      # (but not with the other samplers)
        rules(engine, {"sigma": 0.4, "aware": False}, erasure={"rates": 0.01, "aware": False})
    for decoder, order, lsd in (("bp_osd", 0, None), ("bp_osd_cs", 7, None), ("bp_lsd", 0, {"max_rows": 64})):
        assert rules(engine, {"sigma": 0.4}, decoder=decoder, osd_order=order, lsd=lsd).path == "soft"
        assert rules(engine, {"sigma": 0.4, "aware": False}, decoder=decoder, osd_order=order, lsd=lsd).path == "flooding"
    assert rules(engine, None).soft is None and rules(engine, None).path == "flooding"
    assert rules(engine, {"sigma": 0.4, "aware": False}, osd_order=3).path == "flooding"       # the OSD-w pass samples through the plan
    for bad in ({"sigma": 0.4, "readout": own}, {"aware": True}, 0.4, {"sigma": -1.0}, {"sigma": 0.4, "levels": 17}, {"sigma": 0.4, "alpha": 0.0},
                {"sigma": 0.4, "aware": 1}, {"readout": ([0.1], [0.9])}, {"sigma": 0.4, "rates": 0.1}, {"readout": own, "levels": 8}):
        with pytest.raises(ValueError):
            rules(engine, bad)
    for kw in (dict(alpha_mode="alvarado"), dict(alvarado_alpha=0.9), dict(use_dynamic_alpha=False), dict(scopt=True), dict(osd_order=3)):
        with pytest.raises(ValueError):
            rules(engine, {"sigma": 0.4}, **kw)                             # the path's alpha is its own constant; no OSD-w pass behind it
    from qldpc_amd.simulation.noise_model import NoiseModel
    with pytest.raises(ValueError, match="does not go with soft"):
        engine._noise_model_rules("run_simulation", NoiseModel(0.001), True, None, None, {"sigma": 0.4})
    with pytest.raises(ValueError, match="matched_priors"):
        engine._noise_model_rules("run_simulation", None, 1, None, None, {"sigma": 0.4})
    engine._noise_model_rules("run_simulation", None, False, None, None, {"sigma": 0.4})


def test_strata_and_dem_entry_points_refuse_it(L, monkeypatch):
    import correlated_model as CM
    from qldpc_amd.simulation import dem, strata

    def no_gpu(*a, **k):
        raise AssertionError("GPU work started before the arguments were checked")
    monkeypatch.setattr(L, "Graph", no_gpu)
    for aware in (True, False):
        so = {"sigma": 0.4, "aware": aware}
        with pytest.raises(ValueError, match="soft"):
            strata.run_weight_strata(None, None, None, None, 0.003, weights=[1], soft=so)
        with pytest.raises(ValueError, match="soft"):
            strata.run_dem_weight_strata(CM.toy_dem(), weights=[1], soft=so)
        with pytest.raises(ValueError, match="soft"):
            dem.run_dem_simulation(CM.toy_dem(), num_trials=10, devices=[0], soft=so)


def test_binding_follows_the_header(L):
    names = L.exports()
    for fn in ("qldpc_soft_priors", "qldpc_soft_priors_dev", "qldpc_circuit_plan_use_soft_readout", "qldpc_circuit_plan_use_soft_aware",
               "qldpc_circuit_plan_sample_soft"):
        assert fn in names
        getattr(L.lib(), fn)
    assert L.lib().qldpc_version() == 101
    sig = L.signatures()
    assert len(sig["qldpc_soft_priors"][1]) == 10 and sig["qldpc_soft_priors"][1][3] == C.POINTER(C.c_uint8)
    dev = sig["qldpc_soft_priors_dev"][1]
    assert len(dev) == 11 and all(dev[i] is C.c_void_p for i in (3, 4, 5, 7, 8, 9, 10))
    assert sig["qldpc_circuit_plan_use_soft_readout"][1][2] == C.POINTER(C.c_double) and len(sig["qldpc_circuit_plan_use_soft_aware"][1]) == 11
    mass = np.ones(2)
    assert L.lib().qldpc_circuit_plan_use_soft_readout(None, 2, L.ptr(mass, C.c_double), L.ptr(mass, C.c_double)) == -1
    assert b"plan is NULL" in L.lib().qldpc_last_error()
    assert L.lib().qldpc_circuit_plan_use_soft_aware(None, 1.0, 3, *([None] * 8)) == -1 and b"plan is NULL" in L.lib().qldpc_last_error()
    assert L.lib().qldpc_circuit_plan_sample_soft(None, 1, 0, 1, *([None] * 7)) == -1
    text = open(L.HEADER_PATH).read()
    assert "prior[b][j] = lut[lut_ptr[j] + I_j]" in text and "#define QLDPC_SOFT_MAX_LEVELS 16" in text and "n <= 81920" in text
