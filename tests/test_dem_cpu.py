"""Detector error models without a GPU: the numpy model of the sampler (tests/dem_model.py), the text parser, the derived decoder view, the shipped
decoding matrices as a model, and every argument rule of run_dem_simulation (all raise before a device call)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dem_model as DM  # noqa: E402

import qldpc_amd  # noqa: E402,F401
from qldpc_amd import _lib  # noqa: E402
from qldpc_amd.data import load_precomputed_matrices  # noqa: E402
from qldpc_amd.simulation.dem import DetectorErrorModel, run_dem_simulation  # noqa: E402
from qldpc_amd.simulation.engine import prior_llrs  # noqa: E402


# ---- the numpy model of the sampler ---------------------------------------------------------------------------------------------------------------
def test_threshold_rule():
    p = np.array([0.0, 2.0 ** -32, 0.5, 1.0 - 2.0 ** -53])
    assert DM.thresholds(p).tolist() == [0, 1, 1 << 31, (1 << 32) - 1]
    f = DM.fires(p, seed=7, trial_begin=0, count=4096)
    assert not f[:, 0].any()                                    # thr = 0: no word is below it
    assert f[:, 3].sum() >= 4095                                # thr = 2^32 - 1: fires unless the word is 0xFFFFFFFF
    assert abs(int(f[:, 2].sum()) - 2048) <= 5 * np.sqrt(4096 * 0.25)


def test_model_rate_and_law():
    f = DM.fires([0.25] * 6, seed=20260301, trial_begin=0, count=65536)
    sd = np.sqrt(65536 * 0.25 * 0.75)
    for l in range(6):
        assert abs(int(f[:, l].sum()) - 16384) <= 5 * sd, (l, int(f[:, l].sum()))
    # the law, spelled out for one (trial, mechanism): word l & 3 of block l >> 2, domain 3, counter = the 64-bit global trial index
    from relay_model import philox4x32_10
    seed, g, l = (5 << 32) | 9, (1 << 32) + 3, 5
    o = philox4x32_10(g & 0xFFFFFFFF, g >> 32, l >> 2, 3, seed & 0xFFFFFFFF, seed >> 32)
    want = int(o[l & 3]) < (1 << 30)
    assert bool(DM.fires([0.25] * 6, seed, g, 1)[0, l]) == want
    # independent of how a range is cut
    a = DM.fires([0.25] * 6, 3, (1 << 32) - 10, 20)
    b = np.concatenate([DM.fires([0.25] * 6, 3, (1 << 32) - 10, 7), DM.fires([0.25] * 6, 3, (1 << 32) - 3, 13)])
    assert np.array_equal(a, b)


def test_tiny_model_sample():
    dem = DM.tiny_dem(DetectorErrorModel)
    assert dem.n_mech == 37 and dem.n_det == (37, 5) and dem.k == (64, 3)
    (s0, t0), (s1, t1) = DM.sample(dem, 11, (1 << 32) - 100, 512)
    assert s0.shape == (512, 37) and t0.shape == (512, 64) and s1.shape == (512, 5) and t1.shape == (512, 3)
    f = DM.fires(dem.prob, 11, (1 << 32) - 100, 512)
    assert not f[:, 0].any() and not f[:, 1].any()              # p = 0 and thr = 1
    only5 = np.flatnonzero(f[:, 5] & ~f[:, 4])
    assert only5.size and (t0[only5, 63] == 1).all()            # bit 63 comes from mechanism 5 alone
    t = int(np.flatnonzero(f.sum(axis=1) >= 3)[0])                # one trial by hand: XOR of the firing mechanisms' detector lists
    want = np.zeros(37, np.int8)
    for l in np.flatnonzero(f[t]):
        want[dem.mechanism(l, 0)[0]] ^= 1
    assert np.array_equal(s0[t], want)


# ---- from_text --------------------------------------------------------------------------------------------------------------------------------------
TEXT = """
# a hand-written model: D0 D1 D3 live in sector 0, D2 D4 D5 in sector 1
error(0.1) D0 D1 ^ D1 L0        # D1 cancels
error(0.2) D2 D3                # touches both sectors
error(0.25) L1                  # only a logical
detector(1, 2.5, 0) D5          # declared, never used
logical_observable L2
error(0.3) D0 L0

error(0.05) D4 ^ D0 L1 L1       # L1 cancels
"""
SOD = [0, 0, 1, 0, 1, 1]


def test_from_text_two_sectors():
    d = DetectorErrorModel.from_text(TEXT, sector_of_detector=SOD)
    assert d.n_sectors == 2 and d.n_mech == 5 and d.n_det == (3, 3) and d.k == (3, 3)
    assert d.prob.tolist() == [0.1, 0.2, 0.25, 0.3, 0.05]
    m = lambda l, s: (d.mechanism(l, s)[0].tolist(), d.mechanism(l, s)[1])      # noqa: E731
    assert m(0, 0) == ([0], 1) and m(0, 1) == ([], 0)           # D0 D1 D1 -> D0; L0 counts where the mechanism flips a detector
    assert m(1, 0) == ([2], 0) and m(1, 1) == ([0], 0)          # D3 is detector 2 of sector 0, D2 detector 0 of sector 1
    assert m(2, 0) == ([], 2) and m(2, 1) == ([], 0)            # no detector: an undetectable flip, counted in sector 0
    assert m(3, 0) == ([0], 1)
    assert m(4, 0) == ([0], 0) and m(4, 1) == ([1], 0)          # D4 is detector 1 of sector 1; L1 L1 cancels


def test_from_text_one_sector_and_rejections():
    d = DetectorErrorModel.from_text(TEXT)
    assert d.n_sectors == 1 and d.n_det == (6,) and d.k == (3,)  # D5 and L2 are declared only
    assert d.mechanism(1)[0].tolist() == [2, 3] and d.mechanism(2)[1] == 2
    for bad in ("repeat 3 {\n error(0.1) D0\n}", "error(0.1) D0\nshift_detectors 2", "error(0.1) D0\nshift_detectors(1, 0) 4"):
        with pytest.raises(ValueError, match="flatten"):
            DetectorErrorModel.from_text(bad)
    with pytest.raises(ValueError, match="cannot parse"):
        DetectorErrorModel.from_text("eror(0.1) D0")
    with pytest.raises(ValueError, match="bad target"):
        DetectorErrorModel.from_text("error(0.1) D0 X3")
    with pytest.raises(ValueError, match="0 <= p < 1"):
        DetectorErrorModel.from_text("error(1.0) D0")
    with pytest.raises(ValueError, match="sector_of_detector"):
        DetectorErrorModel.from_text(TEXT, sector_of_detector=[0, 1])


# ---- the derived decoder view ----------------------------------------------------------------------------------------------------------------------
def test_decoder_view_merge_order_and_drops():
    p = [0.1, 0.0, 0.2, 0.3, 0.05, 0.4, 0.15]
    cols = [[([0, 2], 1)],      # column 0
            [([1], 0)],         # p = 0: not in the view at all
            [([1], 0)],         # column 1
            [([0, 2], 1)],      # merges into column 0
            [([], 3)],          # no detector: dropped
            [([0, 2], 2)],      # the detectors of column 0 with another logical: a column of its own
            [([2, 0], 1)]]      # merges into column 0 (third)
    d = DetectorErrorModel.from_columns(p, cols, (3,), (2,))
    v = d.decoder_view(0)
    assert v.shape == (3, 3) and v.logmask.tolist() == [1, 0, 2]
    H = np.zeros(v.shape, np.int8)
    for i in range(3):
        H[i, v.indices[v.indptr[i]:v.indptr[i + 1]]] = 1
        assert np.all(np.diff(v.indices[v.indptr[i]:v.indptr[i + 1]]) > 0)         # canonical: sorted inside a row
    assert H.tolist() == [[1, 0, 1], [0, 1, 0], [1, 0, 1]]
    q = 0.1
    for x in (0.3, 0.15):                                         # folded in mechanism order
        q = q * (1.0 - x) + x * (1.0 - q)
    assert np.array_equal(v.prior, prior_llrs(np.array([q, 0.2, 0.4])))
    other = 0.1
    for x in (0.15, 0.3):
        other = other * (1.0 - x) + x * (1.0 - other)
    assert q == pytest.approx(other, rel=1e-14)                   # (the fold commutes up to rounding; the order pins the bits)


# ---- the shipped matrices as a model ---------------------------------------------------------------------------------------------------------------
def test_from_decoding_matrices_circ72():
    m = load_precomputed_matrices("circ72")
    d = DetectorErrorModel.from_decoding_matrices("circ72", layer_rows=36)
    assert d.n_mech == 2232 + 2268 and d.n_det == (288, 288) and d.k == (12, 12) and d.layer_rows == (36, 36)
    first = 0
    for s, name in enumerate("ZX"):
        ip, ix, shape = _lib.canonical_csr(m[f"Hdec{name}"])
        v = d.decoder_view(s)
        assert v.shape == tuple(shape) and np.array_equal(v.indptr, ip) and np.array_equal(v.indices, ix)
        assert np.array_equal(v.prior, prior_llrs(np.asarray(m[f"channel_probs{name}"], np.float64)))
        mask = _lib.logical_column_masks(m[f"H{name}_logical"], shape[1])
        assert np.array_equal(v.logmask, mask)
        H = m[f"Hdec{name}"].tocsc()
        empty = np.flatnonzero((np.diff(H.indptr) == 0) & (mask == 0))
        assert empty.size == 1                                    # the one "nothing detectable" column: left out of the sampler
        kept = np.setdiff1d(np.arange(shape[1]), empty)
        assert np.array_equal(d.prob[first:first + kept.size], np.asarray(m[f"channel_probs{name}"])[kept])
        for l, j in list(enumerate(kept))[::97]:                  # mechanism = column, in its own sector only
            det, lm = d.mechanism(first + l, s)
            assert np.array_equal(det, np.sort(H.indices[H.indptr[j]:H.indptr[j + 1]])) and lm == int(mask[j])
            other, olm = d.mechanism(first + l, 1 - s)
            assert other.size == 0 and olm == 0
        first += kept.size
    # a dict works like the tag; a bad probability on a column that can fire is refused by name, on the empty column it is not
    m2 = dict(m)
    assert DetectorErrorModel.from_decoding_matrices(m2).n_mech == 4500
    cp = np.array(m["channel_probsZ"], np.float64)
    j = int(np.flatnonzero(np.diff(m["HdecZ"].tocsc().indptr) > 0)[5])
    cp[j] = 1.0
    m2["channel_probsZ"] = cp
    with pytest.raises(ValueError, match=f"column {j} of HdecZ"):
        DetectorErrorModel.from_decoding_matrices(m2)


# ---- run_dem_simulation: every refused combination raises before a device call ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def circ72():
    return DetectorErrorModel.from_decoding_matrices("circ72")


@pytest.mark.parametrize("kw, match", [
    (dict(osd_order=2), "bp_osd_cs"),
    (dict(osd_order=-1), "osd_order must be >= 0"),
    (dict(alpha_mode="alvarado"), "explicit alvarado_alpha"),
    (dict(alpha_mode="alvarado-autoregressive"), "alpha estimator"),
    (dict(alpha_mode="nope"), "alpha_mode"),
    (dict(alvarado_alpha=0.8), "alvarado_alpha is for"),
    (dict(decoder="union_find"), "Unsupported decoder"),
    (dict(relay_params={"gamma0": 0.1}), "relay_params is for decoder='relay_bp'"),
    (dict(decoder="relay_bp", osd_order=1), "does not use osd_order"),
    (dict(decoder="relay_bp", alpha_mode="dynamical"), "does not use alpha_mode"),
    (dict(decoder="bp_osd_cs", osd_order=65), "combination-sweep order"),
    (dict(window=(3, 1)), "layer_rows"),
    (dict(window=(3, 1), decoder="bp_osd_cs"), "window=\\(W, C\\) goes with"),
    (dict(schedule="zigzag"), "Unsupported schedule"),
    (dict(layers=(None, None)), "layers is for schedule='layered'"),
    (dict(schedule="layered", decoder="relay_bp"), "schedule='layered' goes with"),
    (dict(schedule="layered", alpha_mode="alvarado"), "no alpha estimator"),
    (dict(decimation={"alpha": 0.9}, schedule="layered"), "decimation=... does not go with schedule"),
    (dict(decimation={"alpha": 0.9}, alpha_mode="dynamical"), "does not use alpha_mode"),
    (dict(precision="f16"), "Unsupported precision"),
    (dict(precision="f32", decoder="relay_bp"), "precision='f32' goes with"),
    (dict(precision="f32", decimation={}), "precision='f32' does not go with decimation"),
    (dict(num_workers=0), "num_workers must be >= 1"),
])
def test_run_dem_simulation_argument_rules(circ72, kw, match):
    with pytest.raises(ValueError, match=match):
        run_dem_simulation(circ72, num_trials=16, **kw)


def test_run_dem_simulation_wants_a_model():
    with pytest.raises(ValueError, match="DetectorErrorModel"):
        run_dem_simulation({"HdecZ": None})


def test_binding_declares_the_entry_point():
    assert "qldpc_circuit_plan_create_dem" in _lib.exports()
    restype, argtypes = _lib.signatures()["qldpc_circuit_plan_create_dem"]
    assert len(argtypes) == 21 and argtypes[0]._type_ is _lib.DemDesc
    assert hasattr(_lib.lib(), "qldpc_circuit_plan_create_dem")               # the built library exports it
    assert issubclass(_lib.DemPlan, _lib.CircuitPlan)
    for name in ("use_relay", "use_osd_cs", "use_window", "use_layered", "use_decimation", "use_f32", "run", "run_outcomes", "read", "sample", "close"):
        assert name not in _lib.DemPlan.__dict__                                # inherited, not copied
