"""Heralded erasures without a GPU: the decoder tables of simulation/erasure.py on hand-made signatures -- the conditional flip probabilities by
enumerating every Pauli of a class, the table properties, equality with the numpy model -- the prior rule on its edge cases, the table validation of
qldpc_erasure_priors (it runs before any device call), the argument rules of run_simulation(erasure=...) and the binding."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import erasure_model as EM  # noqa: E402
from fixed_weight_model import OP_CNOT, OP_IDLE, OP_MEAS_X, OP_PREP_Z  # noqa: E402


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    return _lib


# ---------------------------------------------------------------------------------------- a hand-made circuit: 8 locations, 3 detectors per sector, k = 1
OPS = [OP_MEAS_X, OP_IDLE, OP_CNOT, OP_CNOT, OP_CNOT, OP_PREP_Z, OP_MEAS_X, OP_CNOT]
E = ((), 0)
# (detectors, logical mask) of (slot 0, slot 1) per location
SIG_Z = [((0,), 0), E,   ((1,), 1), E,   ((0,), 0), ((1,), 1),   ((2,), 0), E,   ((0,), 0), ((2,), 0),   E, E,   E, E,   ((0,), 0), ((1,), 1)]
SIG_X = [E, E,   ((0,), 0), E,   ((0,), 0), ((0,), 0),   E, ((1,), 0),   E, E,   ((2,), 1), E,   E, E,   ((1,), 0), ((2,), 1)]
COLS_Z = [((0,), 0), ((1,), 1), ((0, 1), 1), ((2,), 0), ((1, 2), 0)]          # the last one: a column no location reaches
COLS_X = [((0,), 0), ((1,), 0), ((2,), 1), ((1, 2), 1)]
PROBS_Z, PROBS_X = np.array([0.01, 0.02, 0.004, 0.03, 0.005]), np.array([0.015, 0.002, 0.01, 0.007])


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


@pytest.fixture(scope="module")
def tables():
    from qldpc_amd.simulation.erasure import erasure_tables_from_circuit
    return erasure_tables_from_circuit({"base_ops": np.array(OPS)}, np.zeros((1, 2)), np.zeros((1, 2)), matrices(), signatures=(sig_table(SIG_Z), sig_table(SIG_X)))


def test_conditional_probabilities_by_enumeration(tables):
    """every Pauli of an erased location's class, equally likely: a column with an h = 1 entry flips under a quarter of them, one with INF under half"""
    masks = {OP_CNOT: [r & 15 for r in range(16)], OP_IDLE: [int(EM.ERASED_IDLE[r]) for r in range(4)], OP_MEAS_X: [0, 4], OP_PREP_Z: [0, 1]}
    for r in range(64):                                                     # the model's law gives those masks
        for op in masks:
            assert int(EM.erased_components(np.array([op]), np.array([r]))[0]) == masks[op][r % len(masks[op])]
    seen_inf_pair = seen_inf_empty = seen_quarter = 0
    for s, (sig, cols, bits) in enumerate(((SIG_Z, COLS_Z, (4, 8)), (SIG_X, COLS_X, (1, 2)))):
        for l, op in enumerate(OPS):
            flips = {}
            for mask in masks[op]:
                dets, lm = set(), 0
                for slot in range(2):
                    if mask & bits[slot]:
                        dets ^= set(sig[2 * l + slot][0])
                        lm ^= sig[2 * l + slot][1]
                key = (tuple(sorted(dets)), lm)
                if key in cols:
                    flips[cols.index(key)] = flips.get(cols.index(key), 0) + 1
            want = {c: len(masks[op]) // (4 if h == 1 else 2) for c, h in tables[s].contributions(l)}
            assert flips == want, (s, l)
            seen_quarter += sum(h == 1 for _, h in tables[s].contributions(l))
            if op == OP_CNOT and sig[2 * l] == sig[2 * l + 1] != E:
                seen_inf_pair += 1
            if op == OP_CNOT and (sig[2 * l] == E) != (sig[2 * l + 1] == E):
                seen_inf_empty += 1
    assert seen_quarter >= 6 and seen_inf_pair == 1 and seen_inf_empty == 2        # a == b, and b empty / a empty, were among them


def test_tables_by_hand_and_their_properties(tables):
    tz, tx = tables
    INF = EM.H_INF
    assert [tz.contributions(l) for l in range(8)] == [[(0, INF)], [(1, INF)], [(0, 1), (1, 1), (2, 1)], [(3, INF)], [(0, 1), (3, 1)], [], [], [(0, 1), (1, 1), (2, 1)]]
    assert [tx.contributions(l) for l in range(8)] == [[], [(0, INF)], [(0, INF)], [(1, INF)], [], [(2, INF)], [], [(1, 1), (2, 1), (3, 1)]]
    assert tz.unmatched == 1 and tx.unmatched == 0                          # location 4's a ^ b = ({0, 2}, 0) is no column of sector Z
    assert tz.n_locs == tx.n_locs == 8 and tz.n == 5 and tx.n == 4
    assert np.diff(tz.lut_ptr).tolist() == [4, 3, 3, 2, 1] and np.diff(tx.lut_ptr).tolist() == [1, 2, 2, 2]
    from qldpc_amd.simulation.engine import prior_llrs
    for t, probs in ((tz, PROBS_Z), (tx, PROBS_X)):
        assert np.array_equal(t.lut[t.lut_ptr[:-1]], prior_llrs(probs))     # entry 0: the prior verbatim
        for j in range(t.n):
            run = t.lut[t.lut_ptr[j]:t.lut_ptr[j + 1]]
            assert (np.diff(run) < 0).all() and (run > 0).all()             # strictly down towards 0
            for H in range(1, run.size):
                q = (1 - (1 - 2 * probs[j]) * 0.5 ** H) / 2
                assert abs(run[H] - math.log((1 - q) / q)) <= 1e-12       # (the model pins the bits; this pins the formula)
        for l in range(t.n_locs):
            cols = [c for c, _ in t.contributions(l)]
            assert cols == sorted(set(cols))


def test_tables_equal_the_model(tables):
    for s, (sig, cols, probs) in enumerate(((SIG_Z, COLS_Z, PROBS_Z), (SIG_X, COLS_X, PROBS_X))):
        M = matrices()
        name = "ZX"[s]
        want = EM.build_tables(OPS, sig_table(sig), bool(s), EM.columns_of(M[f"Hdec{name}"], M[f"H{name}_logical"][0]), len(cols), probs, EM.prior_llrs(probs))
        for k in ("loc_ptr", "loc_col", "loc_h", "lut_ptr", "lut"):
            assert np.array_equal(getattr(tables[s], k), want[k]), (s, k)
        assert tables[s].unmatched == want["unmatched"]


def test_prior_rule_on_the_model(tables):
    tz = tables[0]
    erased = np.zeros((5, 8), bool)
    erased[1, [2, 7]] = True                                               # two h = 1 entries on columns 0, 1, 2
    erased[2, [0, 2, 4, 7]] = True                                         # column 0: INF and three h = 1; column 3: one h = 1
    erased[3, :] = True
    erased[4, [5, 6]] = True                                               # locations with no contribution in this sector
    P = EM.priors(erased, tz)
    lut, up = tz.lut, tz.lut_ptr
    assert np.array_equal(P[0], lut[up[:-1]]) and np.array_equal(P[4], P[0])
    assert P[1].tolist() == [lut[up[0] + 2], lut[up[1] + 2], lut[up[2] + 2], lut[up[3]], lut[up[4]]]
    assert P[2].tolist() == [0.0, lut[up[1] + 2], lut[up[2] + 2], lut[up[3] + 1], lut[up[4]]]
    assert P[3].tolist() == [0.0, 0.0, lut[up[2] + 2], 0.0, lut[up[4]]]
    words = EM.pack_heralds(erased)
    assert words.shape == (5, 1) and words[3, 0] == 0xFF and np.array_equal(EM.unpack_heralds(words, 8), erased)


def test_rates_argument():
    from qldpc_amd.simulation.erasure import erasure_rates
    assert erasure_rates(0.01).tolist() == [0, 0.01, 0.01, 0.01, 0.01, 0.01, 0.01]
    assert erasure_rates({"CNOT": 0.02, "IDLE": 0.5}).tolist() == [0, 0.02, 0, 0, 0, 0, 0.5]
    assert np.array_equal(erasure_rates({"MeasX": 0.25, "PrepZ": 0.125}), EM.rates_by_op({"MeasX": 0.25, "PrepZ": 0.125}))
    for bad in ({"CX": 0.1}, 1.0, -0.1, {"CNOT": 1.5}, float("nan"), "0.1", [0.1], True):
        with pytest.raises(ValueError):
            erasure_rates(bad)


# ---------------------------------------------------------------------------------------- the library's table validation: no device is touched
def test_malformed_tables_are_refused_with_the_index_named(L, tables):
    lp, lc, lh, up, lu = EM.as_tuple(tables[0])
    erased = np.zeros((1, 1), np.uint32)

    def refused(t, text):
        with pytest.raises(L.QldpcError, match="error -1") as ei:
            L.erasure_priors(erased, t)
        assert text in str(ei.value), str(ei.value)

    def put(a, i, v):
        a = a.copy()
        a[i] = v
        return a
    refused((put(lp, 0, 1), lc, lh, up, lu), "loc_ptr[0] = 1")
    refused((put(lp, 3, 1), lc, lh, up, lu), "loc_ptr[3] = 1 is below loc_ptr[2] = 2")
    refused((lp, put(lc, 4, 5), lh, up, lu), "loc_col[4] = 5 is outside 0..4")
    refused((lp, put(lc, 3, 2), lh, up, lu), "loc_col[4] = 2 does not ascend inside the run of location 2")
    refused((lp, lc, put(lh, 2, 2), up, lu), "loc_h[2] = 2")
    refused((lp, lc, lh, put(up, 0, 1), lu), "lut_ptr[0] = 1")
    refused((lp, lc, put(lh, 2, EM.H_INF), up, lu), "column 0 has 2 contributions with h = 1")      # lut_ptr no longer matches the counts
    refused((lp, lc, lh, up, put(lu, 5, np.inf)), "lut[5] is not finite")
    with pytest.raises(ValueError):
        L.erasure_priors(np.zeros((1, 2), np.uint32), (lp, lc, lh, up, lu))                          # one herald word expected for 8 locations
    with pytest.raises(ValueError):
        L.erasure_table_args((lp, lc[:3], lh[:3], up, lu))


# ---------------------------------------------------------------------------------------- argument rules
def rules(engine, erasure, **kw):
    a = dict(osd_order=0, precision="f64", decimation=None, schedule="flooding", layers=None, window=None, decoder="bp_osd", relay_params=None,
             alpha_mode=None, alvarado_alpha=None, use_dynamic_alpha=True, scopt=False, lsd=None, correlated=None)
    a.update(kw)
    return engine._extension_rules(a["osd_order"], a["precision"], a["decimation"], a["schedule"], a["layers"], a["window"], a["decoder"], a["relay_params"],
                                   a["alpha_mode"], a["alvarado_alpha"], a["use_dynamic_alpha"], a["scopt"], 50, None, lsd=a["lsd"], correlated=a["correlated"],
                                   erasure=erasure)


OTHER_PATHS = (dict(precision="f32"), dict(decimation={}), dict(schedule="layered"), dict(window=(4, 2)), dict(decoder="relay_bp"), dict(correlated={}))


def test_extension_rules():
    from qldpc_amd.simulation import engine
    r = rules(engine, {"rates": 0.01})
    assert r.path == "erasure" and r.erasure["aware"] is True and r.erasure["alpha"] == 1.0 and r.erasure["rates"].tolist() == [0] + [0.01] * 6
    r = rules(engine, {"rates": {"CNOT": 0.02}, "aware": True, "alpha": 0.875})
    assert r.path == "erasure" and r.erasure["alpha"] == 0.875 and r.erasure["rates"][1] == 0.02 and r.erasure_tables is None
    for other in OTHER_PATHS:                                              # aware is a path: it goes with none of the others ...
        with pytest.raises(ValueError, match="does not go with"):
            rules(engine, {"rates": 0.01, "aware": True}, **other)
        u = rules(engine, {"rates": 0.01, "aware": False}, **other)         # ... unaware is the sampler axis: it goes with each
        assert u.path != "erasure" and u.path != "flooding" and u.erasure["aware"] is False
    for decoder, order, lsd in (("bp_osd", 0, None), ("bp_osd_cs", 7, None), ("bp_lsd", 0, {"max_rows": 64})):
        assert rules(engine, {"rates": 0.01}, decoder=decoder, osd_order=order, lsd=lsd).path == "erasure"
        assert rules(engine, {"rates": 0.01, "aware": False}, decoder=decoder, osd_order=order, lsd=lsd).path == "flooding"
    assert rules(engine, None).erasure is None and rules(engine, None).path == "flooding"
    assert rules(engine, {"rates": 0.01, "aware": False}, osd_order=3).path == "flooding"      # the OSD-w pass samples through the plan
    for bad in ({"rates": 0.01, "aware": True, "osd_order": 0}, {"aware": True}, 0.01, {"rates": 1.5}, {"rates": {"H": 0.1}}, {"rates": 0.01, "alpha": 0.0},
                {"rates": 0.01, "aware": 1}):
        with pytest.raises(ValueError):
            rules(engine, bad)
    for kw in (dict(alpha_mode="alvarado"), dict(alvarado_alpha=0.9), dict(use_dynamic_alpha=False), dict(scopt=True), dict(osd_order=3)):
        with pytest.raises(ValueError):
            rules(engine, {"rates": 0.01}, **kw)                            # the path's alpha is its own constant; no OSD-w pass behind it


def test_strata_and_dem_entry_points_refuse_it(L, monkeypatch):
    import correlated_model as CM
    from qldpc_amd.simulation import dem, strata

    def no_gpu(*a, **k):
        raise AssertionError("GPU work started before the arguments were checked")
    monkeypatch.setattr(L, "Graph", no_gpu)
    for aware in (True, False):
        er = {"rates": 0.01, "aware": aware}
        with pytest.raises(ValueError, match="erasure"):
            strata.run_weight_strata(None, None, None, None, 0.003, weights=[1], erasure=er)
        with pytest.raises(ValueError, match="erasure"):
            strata.run_dem_weight_strata(CM.toy_dem(), weights=[1], erasure=er)
        with pytest.raises(ValueError, match="erasure"):
            dem.run_dem_simulation(CM.toy_dem(), num_trials=10, devices=[0], erasure=er)


def test_binding_follows_the_header(L):
    names = L.exports()
    for fn in ("qldpc_erasure_priors", "qldpc_erasure_priors_dev", "qldpc_circuit_plan_use_erasure_noise", "qldpc_circuit_plan_use_erasure_aware",
               "qldpc_circuit_plan_sample_erasures"):
        assert fn in names
        getattr(L.lib(), fn)
    assert L.lib().qldpc_version() == 101
    sig = L.signatures()
    assert len(sig["qldpc_erasure_priors"][1]) == 10 and sig["qldpc_erasure_priors"][1][2] == C.POINTER(C.c_uint32)
    dev = sig["qldpc_erasure_priors_dev"][1]
    assert len(dev) == 11 and all(dev[i] is C.c_void_p for i in (2, 3, 4, 5, 7, 8, 9, 10))
    assert sig["qldpc_circuit_plan_use_erasure_noise"][1][1] == C.POINTER(C.c_double) and len(sig["qldpc_circuit_plan_use_erasure_aware"][1]) == 12
    rate = np.zeros(7)
    assert L.lib().qldpc_circuit_plan_use_erasure_noise(None, L.ptr(rate, C.c_double)) == -1 and b"plan is NULL" in L.lib().qldpc_last_error()
    assert L.lib().qldpc_circuit_plan_use_erasure_aware(None, 1.0, *([None] * 10)) == -1 and b"plan is NULL" in L.lib().qldpc_last_error()
    assert L.lib().qldpc_circuit_plan_sample_erasures(None, 1, 0, 1, *([None] * 7)) == -1
    text = open(L.HEADER_PATH).read()
    assert "prior[b][j] = 0.0 if one of them is QLDPC_ERASURE_H_INF, else lut[lut_ptr[j] + H]" in text and "#define QLDPC_ERASURE_H_INF 255" in text
