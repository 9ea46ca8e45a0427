"""LSD cluster statistics, the confidence score and post-selection without a GPU: the model (tests/lsd_stats_model.py) against the identities its
definition implies on the seeded shots of tests/lsd_shapes.py, the score combination, the binning rule and the curve arithmetic (the model against
simulation/postselect.py and against hand-worked cases), and the argument rules of the Python layers."""
import math

import numpy as np
import pytest

import lsd_shapes as LS
import lsd_stats_model as SM

NONE = SM.NONE


def _weights(n, seed=7):
    """a seeded uint16 table that holds 0 and 65535"""
    w = np.random.default_rng([seed, n]).integers(0, 65536, n).astype(np.uint16)
    w[0], w[n // 2] = 0, 65535
    return w


def _model(key, name, shots, bps, max_rows=128, weight=None):
    f, G = LS.matrix(key)
    _, info, traces = LS.answers(key, name, shots, bps, max_rows)
    return G, info, traces, SM.stats_from_traces(G, shots, info, traces, weight)


@pytest.mark.parametrize("bps", (1, 2, 64))
@pytest.mark.parametrize("key", sorted(LS.MATRICES))
def test_model_identities_on_the_general_shots(key, bps):
    """word 1 == info[3], the rows of the clusters add up to info[2], the words are consistent with one another, zero residual gives eight zeros and
    a flag other than 0 eight all-ones words"""
    shots = LS.general(key)
    w = _weights(LS.matrix(key)[0].n)
    G, info, traces, st = _model(key, "general", shots, bps, 128, w)
    bare = SM.stats_from_traces(G, shots, info, traces, None)
    for b in range(shots.synd.shape[0]):
        row = [int(v) for v in st[b]]
        if info[b, 0] != 0:
            assert row == [NONE] * 8 and [int(v) for v in bare[b]] == [NONE] * 8
            continue
        cl = SM.clusters(G, shots.synd[b], shots.hard[b], traces[b].get("A", []))
        assert row[1] == info[b, 3] and sum(len(rows) for rows, _ in cl) == info[b, 2], (key, bps, b)
        assert row[0] == len(cl) and all(cols for _, cols in cl)                  # a cluster that is valid holds a column: its seed has b = 1
        assert row[3] <= row[1] <= row[2] <= row[1] ** 2 and row[6] <= row[4] and row[5] <= row[4] ** 2 < 1 << 64
        assert row[7] <= info[b, 2] and (row[0] > 0) == (info[b, 2] > 0)
        assert [int(v) for v in bare[b]] == row[:4] + [0, 0, 0] + row[7:]         # without weights the words 4 .. 6 are 0
        if info[b, 2] == 0:
            assert row == [0] * 8
    zero = ~(shots.synd ^ np.stack([G.parity(h) for h in shots.hard])).any(axis=1)
    assert zero.sum() >= 3 and not st[zero].any()


def test_the_inputs_exercise_what_can_go_wrong():
    n_clusters = lambda key, bps: _model(key, "general", LS.general(key), bps)[3][:, 0]      # noqa: E731
    G, info, _, st = _model("ident", "general", LS.general("ident"), 1)
    assert (info[:, 0] == 0).all() and sorted(set(st[:, 0].tolist())) == [0, 1, 2, 3, 4] and (st[:, 0] >= 2).sum() == 11
    tiny = n_clusters("tiny", 1)
    assert tiny[tiny != np.uint64(NONE)].max() == 7
    assert set(_model("dep", "general", LS.general("dep"), 1)[1][:, 0]) == {0, 1, 2}
    st = _model("ident", "apart", LS.apart(), 1)[3]
    w = _weights(LS.matrix("ident")[0].n)
    assert (st == np.array([2, 2, 2, 1, 0, 0, 0, 1], np.uint64)).all()                        # two clusters of one row and one column each
    f = LS.matrix("ident")[0]
    stw = _model("ident", "apart", LS.apart(), 1, weight=w)[3]
    _, _, traces = LS.answers("ident", "apart", LS.apart(), 1, 128)
    for b, tr in enumerate(traces):
        wa, wb = (int(w[j]) for j in tr["A"])
        assert [int(v) for v in stw[b, 4:7]] == [wa + wb, wa * wa + wb * wb, max(wa, wb)] and all(j >= f.n - f.m for j in tr["A"])
    st = _model("dep", "merging", LS.merging(), 1)[3]
    assert (st[:, 0] == 1).all() and (st[:, 2] == st[:, 1] ** 2).all() and (st[:, 3] == st[:, 1]).all()      # one cluster: the norms coincide
    st = _model("tiny", "empty_rows", LS.empty_rows(), 1)[3]
    assert (st == np.uint64(NONE)).all()                                                     # flag 2: no statement
    # a weight table of all 65535 on the largest cluster keeps sum W_i^2 below 2^64
    G, info, traces, st = _model("doubled", "duplicates", LS.duplicates(), 2, weight=np.full(LS.matrix("doubled")[0].n, 65535, np.uint16))
    ok = info[:, 0] == 0
    assert (st[ok, 4] == st[ok, 1] * np.uint64(65535)).all() and (st[ok, 0] == 1).all()
    assert [int(v) for v in st[ok, 5]] == [(int(a) * 65535) ** 2 for a in st[ok, 1]]


def test_score_combination():
    z = [3, 10, 40, 6, 1000, 400000, 700, 9]
    x = [1, 4, 16, 4, 50, 2500, 50, 2]
    assert [SM.score(k, z, x) for k in SM.KINDS] == [14, 56, 6, 1050, 402500, 700]
    assert [SM.score(k, x, z) for k in range(6)] == [14, 56, 6, 1050, 402500, 700]
    assert [SM.score(k, z, [0] * 8) for k in range(6)] == z[1:7] == [SM.score(k, z) for k in range(6)]      # a converged sector; a one-sector plan
    assert [SM.score(k, [0] * 8, [0] * 8) for k in range(6)] == [0] * 6
    for k in range(6):                                                            # no statement in either sector
        assert SM.score(k, [NONE] * 8, x) == NONE and SM.score(k, z, [NONE] * 8) == NONE and SM.score(k, [NONE] * 8, [NONE] * 8) == NONE
    big = [1] + [NONE - 1] * 7
    for k in (0, 1, 3, 4):                                                        # the sums saturate one below "no statement"
        assert SM.score(k, big, x) == NONE - 1 and SM.score(k, big, big) == NONE - 1
        assert SM.score(k, [1] + [NONE - 5] * 7, [1] + [4] * 7) == NONE - 1 and SM.score(k, [1] + [NONE - 5] * 7, [1] + [3] * 7) == NONE - 2
    for k in (2, 5):
        assert SM.score(k, big, x) == NONE - 1
    got = SM.scores("llr_2", np.array([z, [NONE] * 8], np.uint64), np.array([x, x], np.uint64))
    assert got.dtype == np.uint64 and got.tolist() == [402500, NONE]


def test_binning_and_histogram():
    edges = [1, 5, 6, 1 << 40, NONE]
    assert [SM.bin_of(s, edges) for s in (0, 1, 4, 5, 6, 7, (1 << 40) - 1, 1 << 40, NONE - 1, NONE)] == [0, 1, 1, 2, 3, 3, 3, 4, 4, 5]      # score == edge goes up
    assert SM.bin_of(0, []) == 0 and SM.bin_of(NONE, []) == 0
    hist = SM.histogram([0, 0, 5, 5, 7, NONE], [0, 1, 2, 3, 0, 3], [1, 6])
    assert hist.tolist() == [[1, 1, 0, 0], [0, 0, 1, 1], [1, 0, 0, 1]]
    import qldpc_amd  # noqa: F401
    from qldpc_amd.simulation.postselect import KINDS, default_edges
    assert KINDS == SM.KINDS
    for kind in KINDS:
        e = [int(v) for v in default_edges(kind)]
        assert e[0] == 1 and e == sorted(set(e)) and len(e) + 1 <= 4096 and e[-1] < NONE
        assert SM.bin_of(0, e) == 0 and SM.bin_of(1, e) == 1 and SM.bin_of(NONE, e) == len(e)      # bin 0: no cluster at all; the last: no statement
    assert default_edges("cols_1", steps_per_octave=1, top_bits=5).tolist() == [1, 2, 4, 8, 16, 32]
    assert default_edges("llr_1", steps_per_octave=2, top_bits=4).tolist() == [1, 2, 3, 4, 6, 8, 12, 16]          # ceil(2^(i / 2))
    assert default_edges("llr_inf", top_bits=3).tolist() == [1, 2, 3, 4, 5, 6, 7, 8]                             # ceil(2^(i / 4)) without repeats

    def ceil_root(i, s):                                                          # the least e with e^s >= 2^i, searched from the float estimate
        e = int(2 ** (i / s))
        while e ** s < 1 << i:
            e += 1
        while e > 1 and (e - 1) ** s >= 1 << i:
            e -= 1
        return e
    assert [int(v) for v in default_edges("llr_1")] == sorted({ceil_root(i, 4) for i in range(32 * 4 + 1)})
    assert [int(v) for v in default_edges("llr_2")] == sorted({ceil_root(i, 2) for i in range(62 * 2 + 1)})
    with pytest.raises(ValueError):
        default_edges("llr_3")
    with pytest.raises(ValueError):
        default_edges("llr_1", steps_per_octave=3)


def test_curve_identities():
    import qldpc_amd  # noqa: F401
    from qldpc_amd.simulation.postselect import PostSelection
    rng = np.random.default_rng(5)
    hist = rng.integers(0, 50, (9, 4)).astype(np.uint64)
    hist[3] = 0                                                                   # an empty bin: two cuts with the same working point
    edges = np.array([1, 2, 3, 5, 8, 13, 21, 34], np.uint64)
    ps = PostSelection(hist, edges, "llr_2")
    c, want = ps.curve(), SM.curve(hist)
    total, fails = int(hist.sum()), int(hist[:, 1:].sum())
    assert len(want) == 10 and ps.trials == total
    for k, w in enumerate(want):
        for name in ("accepted", "failures", "failures_z", "failures_x"):
            assert int(c[name][k]) == w[name], (k, name)
        for name in ("abort_rate", "ler", "std_error"):
            assert (math.isnan(w[name]) and math.isnan(c[name][k])) or c[name][k] == pytest.approx(w[name], rel=1e-14, abs=0), (k, name)
    assert want[0]["accepted"] == 0 and math.isnan(want[0]["ler"]) and want[0]["abort_rate"] == 1.0          # cut 0 accepts nothing
    assert want[9]["accepted"] == total and want[9]["failures"] == fails and want[9]["abort_rate"] == 0.0 and want[9]["ler"] == fails / total
    assert want[9]["failures_z"] == int(hist[:, 1].sum() + hist[:, 3].sum()) and want[9]["failures_x"] == int(hist[:, 2].sum() + hist[:, 3].sum())
    assert all(a["accepted"] <= b["accepted"] and a["failures"] <= b["failures"] for a, b in zip(want, want[1:]))
    assert c["threshold"] == [0, 1, 2, 3, 5, 8, 13, 21, 34, 1 << 64]
    # the working point of an abort budget: of the cuts within it, the one that aborts most
    assert ps.at_abort_rate(0.0)["accepted"] == total and ps.at_abort_rate(1.0)["cut"] == 0
    for x in (0.01, 0.05, 0.3, 0.77):
        at = ps.at_abort_rate(x)
        k = at["cut"]
        assert at["abort_rate"] <= x and (k == 0 or want[k - 1]["abort_rate"] > x) and at["ler"] == pytest.approx(want[k]["ler"], nan_ok=True)
    assert ps.no_statement() == int(hist[-1].sum())
    assert (ps + ps).hist.tolist() == (2 * hist).tolist()
    with pytest.raises(ValueError):
        ps + PostSelection(hist, edges, "llr_1")
    with pytest.raises(ValueError):
        PostSelection(hist[:-1], edges, "llr_2")
    with pytest.raises(ValueError):
        ps.at_abort_rate(1.5)
    empty = PostSelection(np.zeros((1, 4)), [], "cols_1")
    assert empty.trials == 0 and empty.at_abort_rate(0.1)["accepted"] == 0 and SM.curve(np.zeros((1, 4)))[1]["accepted"] == 0


def test_quantise_weights_and_exports():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    q = _lib.quantise_weights([0.0, -0.0, 0.5 / 256, 1.5 / 256, 2.5 / 256, 1.0, -3.25, 255.998, 256.0, 1e9, np.inf, -np.inf, np.nan])
    assert q.dtype == np.uint16 and q.tolist() == [0, 0, 0, 2, 2, 256, 832, 65535, 65535, 65535, 65535, 65535, 65535]      # rint: half-way cases to even
    assert _lib.quantise_weights(np.full(3, 255.99)).tolist() == [65533] * 3
    new = {"qldpc_lsd_stats_batch", "qldpc_lsd_stats_batch_dev", "qldpc_circuit_plan_use_confidence", "qldpc_circuit_plan_confidence_read",
           "qldpc_circuit_plan_run_scores", "qldpc_circuit_plan_decode_events_scored", "qldpc_circuit_plan_decode_events_scored_dev"}
    assert new <= set(_lib.exports())
    import ctypes as C
    sig = _lib.signatures()
    assert sig["qldpc_lsd_stats_batch"][1][7:] == [C.POINTER(C.c_uint16), C.POINTER(C.c_int8), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)]
    assert sig["qldpc_lsd_stats_batch_dev"][1][9:] == [C.c_void_p] * 5 and len(sig["qldpc_lsd_stats_batch_dev"][1]) == 14
    assert sig["qldpc_circuit_plan_use_confidence"][1] == [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint16), C.POINTER(C.c_uint16)]
    assert sig["qldpc_circuit_plan_run_scores"][1][-2:] == [C.POINTER(C.c_uint8), C.POINTER(C.c_uint64)]
    assert len(sig["qldpc_circuit_plan_decode_events_scored"][1]) == len(sig["qldpc_circuit_plan_decode_events"][1]) + 1
    text = open(_lib.HEADER_PATH).read()
    for k, name in enumerate(("COLS_1", "COLS_2", "COLS_INF", "LLR_1", "LLR_2", "LLR_INF")):
        assert f"#define QLDPC_CONF_{name} {k}\n" in text and _lib.CONF_KINDS[name.lower()] == k == SM.KINDS.index(name.lower())
    assert f"#define QLDPC_CONF_MAX_BINS {_lib.CONF_MAX_BINS}\n" in text and len(_lib.LSD_STATS) == 8
    assert int(_lib.NO_STATEMENT) == NONE


def test_python_argument_rules():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    from qldpc_amd.simulation import engine
    from qldpc_amd.simulation.dem import DemDecoder, DetectorErrorModel, run_dem_simulation
    from qldpc_amd.simulation.postselect import default_edges, post_select_rules
    assert _lib.conf_kind("llr_2") == 4 == _lib.conf_kind(4)
    for bad in ("llr", 6, -1, True, None, 1.0):
        with pytest.raises(ValueError):
            _lib.conf_kind(bad)
    assert _lib.conf_edges(None).size == 0 and _lib.conf_edges([1, 2, NONE]).dtype == np.uint64
    for bad in ([2, 2], [3, 1], [-1, 4], [0.5, 2.0], [[1, 2]], list(range(4096))):
        with pytest.raises(ValueError):
            _lib.conf_edges(bad)
    assert _lib.conf_edges(list(range(4095))).size == 4095
    for bad in (np.zeros(4, np.uint16), [0, 1, 70000], [0.5, 1.0, 2.0], [-1, 0, 1]):
        with pytest.raises(ValueError):
            _lib._weights(bad, 3)
    assert _lib._weights([0, 65535, 7], 3).dtype == np.uint16 and _lib._weights(None, 3) is None
    r = post_select_rules("t", {"kind": "llr_2"}, "bp_lsd")
    assert r["kind"] == "llr_2" and np.array_equal(r["edges"], default_edges("llr_2"))
    assert post_select_rules("t", {"kind": "cols_inf", "edges": [1, 4]}, "bp_lsd")["edges"].tolist() == [1, 4]
    assert post_select_rules("t", None, "bp_osd") is None and post_select_rules("t", {"kind": "cols_1"}, "bp_lsd", target_logical_errors=0) is not None
    for ps, decoder, target in (({"kind": "llr_2"}, "bp_osd", None), ({"kind": "llr_2"}, "bp_osd_cs", None), ({"kind": "llr_2"}, "relay_bp", None),
                                ({"kind": "llr_2"}, "bp_lsd", 10), ({"kind": "llr_9"}, "bp_lsd", None), ({"kind": 4}, "bp_lsd", None), ({}, "bp_lsd", None),
                                ("llr_2", "bp_lsd", None), ({"kind": "llr_2", "bins": 4}, "bp_lsd", None), ({"kind": "llr_2", "edges": [2, 1]}, "bp_lsd", None)):
        with pytest.raises(ValueError):
            post_select_rules("t", ps, decoder, target)
    # run_dem_simulation and DemDecoder raise before any device call
    dem = DetectorErrorModel.from_decoding_matrices("circ72", layer_rows=36)
    for kw in (dict(decoder="bp_osd", post_select={"kind": "llr_2"}), dict(decoder="bp_lsd", post_select={"kind": "llr_2"}, target_logical_errors=5),
               dict(decoder="bp_lsd", post_select={"kind": "nope"})):
        with pytest.raises(ValueError):
            run_dem_simulation(dem, num_trials=8, **kw)
    with pytest.raises(ValueError):
        DemDecoder(dem, confidence="llr_2")                                       # (decoder="bp_osd")
    with pytest.raises(ValueError):
        DemDecoder(dem, decoder="bp_lsd", confidence="llr")
    d = DemDecoder(dem, decoder="bp_lsd")
    with pytest.raises(ValueError):
        d.decode_batch(np.zeros((1, dem.n_detectors), np.uint8), return_confidence=True)
    assert DemDecoder(dem, decoder="bp_lsd", confidence="cols_inf")._rules.post_select["edges"].size == 0
    # the switch: the confidence goes last, with the weights the caller put into the rules
    base = dict(osd_order=0, precision="f64", decimation=None, schedule="flooding", layers=None, window=None, decoder="bp_lsd", relay_params=None, alpha_mode=None,
                alvarado_alpha=None, use_dynamic_alpha=True, scopt=False, maxIter=12, num_workers=None)
    rules = engine._extension_rules(**dict(base, precision="f32"))
    assert rules.post_select is None
    rules.post_select = dict(post_select_rules("t", {"kind": "cols_2", "edges": [1, 9]}, "bp_lsd"), weights=["wz", "wx"])
    calls = []

    class Plan:
        def __getattr__(self, name):
            return lambda *a, **k: calls.append((name, a, k))
    engine._plan_switch(rules, [], 0)[0](Plan())
    assert [c[0] for c in calls] == ["use_lsd", "use_f32", "use_confidence"] and calls[2][1][0] == "cols_2" and calls[2][1][2:] == ("wz", "wx")
    # LsdDecoder: weights without statistics are refused before the library is touched
    from qldpc_amd.decoding.lsd import LsdDecoder
    dec = LsdDecoder.__new__(LsdDecoder)
    dec.graph = type("G", (), {"n": 3, "m": 2})()
    with pytest.raises(ValueError):
        dec.decode(np.zeros(2, np.int8), np.zeros(3), np.zeros(3, np.int8), weights=[1, 2, 3])
