"""Recorded detection events without a GPU: the numpy model of the record format (tests/events_model.py) against the library's pack helpers, the
detector maps a DetectorErrorModel keeps, the argument rules of DemDecoder (all raise before a device call), and the plan calls _run_trials makes
after the switch helper was factored out."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dem_model as DM  # noqa: E402
import events_model as EM  # noqa: E402

import qldpc_amd  # noqa: E402,F401
from qldpc_amd import _lib  # noqa: E402
from qldpc_amd.simulation import engine  # noqa: E402
from qldpc_amd.simulation.dem import DemDecoder, DetectorErrorModel, read_b8  # noqa: E402

TEXT = """
error(0.1) D0 D1 L0
error(0.05) D1 D2
error(0.1) D2 D3 L1
error(0.02) D3 D4 ^ D5
error(0.1) D5 D6 L2
error(0.03) D6 D7
error(0.1) D7 D8 L0 L2
error(0.04) D8 D9
error(0.1) D9 D10
error(0.06) D10 D11 L1
error(0.05) D0 D11
detector(1, 2) D11
logical_observable L2
"""


# ---- the record format ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_bits", [1, 7, 8, 9, 37, 42, 61, 64, 65])
def test_pack_round_trip(n_bits):
    rng = np.random.default_rng(n_bits)
    bits = (rng.random((33, n_bits)) < 0.5).astype(np.uint8)
    rec = EM.pack(bits)
    assert rec.shape == (33, (n_bits + 7) // 8) and rec.dtype == np.uint8
    assert np.array_equal(EM.unpack(rec, n_bits), bits)
    for d in (0, n_bits // 2, n_bits - 1):                       # the format, spelled out
        assert np.array_equal((rec[:, d >> 3] >> (d & 7)) & 1, bits[:, d])
    if n_bits % 8:                                              # the unused high bits of the last byte are 0 when packed and ignored when unpacked
        assert not (rec[:, -1] >> (n_bits % 8)).any()
        dirty = rec.copy()
        dirty[:, -1] |= np.uint8((0xFF << (n_bits % 8)) & 0xFF)
        assert np.array_equal(EM.unpack(np.hstack([dirty, np.full((33, 3), 0xFF, np.uint8)]), n_bits), bits)
    assert np.array_equal(_lib.pack_events(bits), rec) and np.array_equal(_lib.pack_events(bits.astype(bool)), rec)      # the library's helpers are the model
    assert np.array_equal(_lib.unpack_bits(rec, n_bits), bits)


def test_gather_and_embed():
    rng = np.random.default_rng(5)
    n_bits, tabs = 20, [np.array([3, -1, 7, 7, 19]), np.array([0, 18])]
    rec = EM.pack(rng.random((64, 24)) < 0.5)
    s0, s1 = EM.gather(rec, n_bits, tabs)
    bits = EM.unpack(rec, n_bits)
    assert np.array_equal(s0[:, 0], bits[:, 3]) and not s0[:, 1].any() and np.array_equal(s0[:, 2], s0[:, 3]) and np.array_equal(s0[:, 4], bits[:, 19])
    assert np.array_equal(s1, bits[:, [0, 18]]) and s0.dtype == np.int8
    n, dflt = EM.default_layout((5, 2))
    assert n == 7 and dflt[0].tolist() == [0, 1, 2, 3, 4] and dflt[1].tolist() == [5, 6]
    syn = [(rng.random((16, 5)) < 0.5).astype(np.int8), (rng.random((16, 2)) < 0.5).astype(np.int8)]
    for stride, fill in ((1, 0), (4, 1)):
        back = EM.gather(EM.embed(syn, n, dflt, stride=stride, fill=fill), n, dflt)
        assert np.array_equal(back[0], syn[0]) and np.array_equal(back[1], syn[1])
    assert (EM.embed(syn, n, dflt, stride=4, fill=1)[:, 1:] == 0xFF).all() and (EM.embed(syn, n, dflt, stride=4, fill=1)[:, 0] >> 7).all()
    lm = np.array([1, 1 << 63, 6, 0], np.uint64)
    assert EM.predict(np.array([[1, 1, 0, 0], [0, 0, 0, 1], [1, 0, 1, 0]], np.int8), lm).tolist() == [(1 << 63) | 1, 0, 7]
    assert EM.pred_bits(np.array([5], np.uint64), 3).tolist() == [[1, 0, 1]]
    assert EM.flags_of([[1, 0]], [[0, 1]], [[1, 1]]).tolist() == [0x11, 0x14]
    assert EM.flags_of([[1], [1]], [[0], [1]], [[0], [1]]).tolist() == [0x2B]


def test_read_b8(tmp_path):
    bits = np.random.default_rng(2).random((50, 13)) < 0.5
    path = tmp_path / "shots.b8"
    _lib.pack_events(bits).tofile(path)
    rec = read_b8(path, 13)
    assert rec.shape == (50, 2) and np.array_equal(_lib.unpack_bits(rec, 13), bits)


# ---- the detector maps ----------------------------------------------------------------------------------------------------------------------------
def test_detector_map():
    sod = np.arange(12) % 2
    dem = DetectorErrorModel.from_text(TEXT, sector_of_detector=sod)
    assert dem.n_det == (6, 6) and dem.k == (3, 3) and dem.n_detectors == 12
    assert dem.detector_map[0].tolist() == [0, 2, 4, 6, 8, 10] and dem.detector_map[1].tolist() == [1, 3, 5, 7, 9, 11]
    for s in range(2):                                          # row r of sector s is the text's detector detector_map[s][r]: mechanism 0 flips D0 and D1
        assert dem.mechanism(0, s)[0].tolist() == [0] and dem.detector_map[s][0] == s
    one = DetectorErrorModel.from_text(TEXT)
    assert one.n_sectors == 1 and one.detector_map[0].tolist() == list(range(12)) and one.n_detectors == 12
    longer = DetectorErrorModel.from_text(TEXT, sector_of_detector=[0, 1] * 7)      # two detectors the text never uses
    assert longer.n_detectors == 14 and longer.detector_map[1].tolist() == list(range(1, 14, 2))
    z = dem.sector(1)
    assert z.n_sectors == 1 and z.detector_map[0].tolist() == dem.detector_map[1].tolist() and z.n_detectors == 12
    tiny = DM.tiny_dem(DetectorErrorModel)                      # from_columns (and a model rebuilt from its sectors): the concatenated default
    assert tiny.detector_map[0].tolist() == list(range(37)) and tiny.detector_map[1].tolist() == list(range(37, 42)) and tiny.n_detectors == 42
    assert tiny.sector(1).detector_map[0].tolist() == list(range(37, 42)) and tiny.sector(1).n_detectors == 42
    circ = DetectorErrorModel.from_decoding_matrices("circ72", layer_rows=36)
    n0, n1 = circ.n_det
    assert circ.detector_map[0].tolist() == list(range(n0)) and circ.detector_map[1].tolist() == list(range(n0, n0 + n1)) and circ.n_detectors == n0 + n1
    with pytest.raises(ValueError, match="detector_map"):
        DetectorErrorModel(tiny.prob, [tuple(S) for S in tiny.sectors], detector_map=[np.arange(37), np.arange(4)])
    with pytest.raises(ValueError, match="detector_map"):
        DetectorErrorModel(tiny.prob, [tuple(S) for S in tiny.sectors], detector_map=[np.arange(37), np.arange(40, 45)], n_detectors=42)


# ---- DemDecoder: every argument rule raises before a device call ------------------------------------------------------------------------------------
def test_dem_decoder_argument_rules():
    dem = DetectorErrorModel.from_text(TEXT, sector_of_detector=np.arange(12) % 2)
    with pytest.raises(ValueError, match="DemDecoder: osd_order=2"):
        DemDecoder(dem, osd_order=2)
    with pytest.raises(ValueError, match="layer_rows"):
        DemDecoder(dem, window=(3, 1))
    with pytest.raises(ValueError, match="does not go with"):
        DemDecoder(dem, decoder="relay_bp", precision="f32")
    with pytest.raises(ValueError, match="alvarado_alpha"):
        DemDecoder(dem, alpha_mode="alvarado")
    with pytest.raises(ValueError, match="DetectorErrorModel"):
        DemDecoder("circ72")
    with pytest.raises(ValueError, match="batch"):
        DemDecoder(dem, batch=0)
    for kw in (dict(), dict(decoder="bp_osd_cs", osd_order=4), dict(decoder="relay_bp", relay_params=dict(t0=20, tr=10, max_legs=6)),
               dict(schedule="layered"), dict(precision="f32"), dict(decimation=dict(alpha=0.9))):
        dec = DemDecoder(dem, maxIter=12, **kw)                 # accepted, and no plan yet: nothing touched a device
        assert dec._plan is None
    dec = DemDecoder(dem)
    with pytest.raises(ValueError, match="12 detectors"):       # wrong width
        dec.decode_batch(np.zeros((4, 11), bool))
    with pytest.raises(ValueError, match="12 detectors"):
        dec.decode_batch(np.zeros((4, 3), np.uint8))
    with pytest.raises(ValueError, match="need 2"):
        dec.decode_batch(np.zeros((4, 1), np.uint8), bit_packed=True)
    with pytest.raises(ValueError, match="bool or uint8"):
        dec.decode_batch(np.zeros((4, 12), np.int64))
    with pytest.raises(ValueError, match="0 or 1"):
        dec.decode_batch(np.full((4, 12), 2, np.uint8))
    with pytest.raises(ValueError, match="shape"):
        dec.decode_batch(np.zeros(12, bool))
    with pytest.raises(ValueError, match="bool array"):
        dec.decode_batch(np.zeros((4, 12), bool), bit_packed=True)
    with pytest.raises(ValueError, match="shot_begin"):
        dec.decode_batch(np.zeros((4, 12), bool), shot_begin=-1)
    assert dec._plan is None
    lone = DemDecoder(DetectorErrorModel.from_text("error(0.1) D0 L0"))      # one detector: one byte either way
    with pytest.raises(ValueError, match="bit_packed=True or False"):
        lone.decode_batch(np.zeros((4, 1), np.uint8))
    assert lone._plan is None


# ---- _run_trials makes the plan calls it made before the helper was factored out ----------------------------------------------------------------------
class _StubPlan:
    def __init__(self, log):
        self.log = log

    def __getattr__(self, name):
        if not name.startswith("use_"):
            raise AttributeError(name)
        return lambda *a, **kw: self.log.append((name, a, kw))

    def phase_times(self):
        return {k: 0.0 for k in _lib.CIRCUIT_PHASES}, 0

    def close(self):
        self.log.append(("close", (), {}))


class _StubStream:
    def __init__(self, device=0):
        self.ptr = 0

    def close(self):
        pass


H = (np.array([0, 2, 4, 6], np.int32), np.array([0, 1, 1, 2, 2, 3], np.int32), 4)      # a 3 x 4 chain: rows 0 and 2 share no column
LAYERS = np.array([0, 1, 0], np.int32)
RELAY = dict(t0=20, tr=10, max_legs=6)
DECIM = dict(alpha=0.9, t_round=10, max_rounds=6, per_round=8)


def _rules(**kw):
    a = dict(osd_order=0, precision="f64", decimation=None, schedule="flooding", layers=None, window=None, decoder="bp_osd", relay_params=None, alpha_mode=None,
             alvarado_alpha=None, use_dynamic_alpha=True, scopt=False, maxIter=12, num_workers=None)
    a.update(kw)
    return engine._extension_rules(**a), a


PATHS = [(dict(), []),
         (dict(decoder="bp_osd_cs", osd_order=4), [("use_osd_cs", (4,), {})]),
         (dict(decoder="relay_bp", relay_params=RELAY), [("use_relay", (), _lib.relay_params(dict(RELAY), with_clip=False))]),
         (dict(window=(3, 1)), [("use_window", (3, 1), {})]),
         (dict(schedule="layered", layers=(LAYERS, None)), [("use_layered", "layers", {})]),
         (dict(decimation=DECIM), [("use_decimation", (), _lib.decim_params(dict(DECIM), with_clip=False))]),
         (dict(precision="f32"), [("use_f32", (), {})]),
         (dict(precision="f32", decoder="bp_osd_cs", osd_order=2), [("use_osd_cs", (2,), {}), ("use_f32", (), {})]),
         (dict(decimation=DECIM, decoder="bp_osd_cs", osd_order=3), [("use_osd_cs", (3,), {}), ("use_decimation", (), _lib.decim_params(dict(DECIM), with_clip=False))])]


@pytest.mark.parametrize("kw, want", PATHS, ids=[",".join(sorted(k)) or "flooding" for k, _ in PATHS])
def test_run_trials_plan_calls(monkeypatch, kw, want):
    monkeypatch.setattr(_lib, "Stream", _StubStream)
    rules, a = _rules(**kw)
    graphs = [type("G", (), dict(indptr=H[0], indices=H[1], n=H[2]))() for _ in range(2)]
    log, made = [], []

    def make_plan(own_graphs, dev):
        made.append((own_graphs, dev))
        return _StubPlan(log)

    res = engine._run_trials(make_plan, graphs, [None, None], [None, None], (1.0, 1.0), (1, 1), rules, 0, 1, [0], 1, 0, None, None, 12, a["osd_order"], "dynamical", 64,
                             a["decoder"], a["schedule"], a["precision"], {})
    assert made == [(graphs, 0)] and log[-1][0] == "close"
    calls = log[:-1]
    assert [c[0] for c in calls] == [w[0] for w in want]
    for got, exp in zip(calls, want):
        if exp[1] == "layers":                                  # the validated row_layer of sector 0, the greedy colouring of sector 1
            assert len(got[1]) == 2 and np.array_equal(got[1][0], LAYERS) and np.array_equal(got[1][1], [0, 1, 0]) and got[2] == {}
        else:
            assert got[1] == exp[1] and got[2] == exp[2]
    assert res["num_trials"] == 0 and res["num_workers"] == 1
    # the helper by itself: the same calls, which is what DemDecoder makes on its plan
    switch, layers = engine._plan_switch(rules, [H, H], a["osd_order"])
    again = []
    switch(_StubPlan(again))
    assert [c[0] for c in again] == [w[0] for w in want] and (layers is None) == (rules.path != "layered")
