"""Soft-readout noise and soft-aware decoding on a circuit plan, on circ72 -- the small plan of tests/test_plan_switch_gpu.py -- and on hand-made
tables: the sampler and the prior kernel equal the numpy model of tests/soft_model.py bit for bit, batching and position do not matter, the plan
equals the chain of its parts verdict for verdict, the levels help, the switch rules gain one row and one column and the sampler axis its refusals,
and run_simulation(soft=...) equals the plan driven by hand."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import correlated_model as CM  # noqa: E402
import soft_model as SM  # noqa: E402
from test_correlated_gpu import logical_bits  # noqa: E402
from test_erasure_gpu import assert_aware_tally, aware_chain  # noqa: E402
from test_plan_switch_gpu import BASE_SWITCHES as SWITCHES, refused, run64, BATCH  # noqa: E402
from test_relay_gpu import _bb_params, circuit_setup  # noqa: E402

pytestmark = pytest.mark.gpu

SEED, COUNT, P = 2031, 384, 0.005                                          # (P: what circuit_setup's plans sample at)
HELP_SIGMA, HELP_SEED = 0.5, 2031                                         # test_the_levels_help: fixed with the model chain, see its docstring
_CACHE = {}


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


def channels():
    from qldpc_amd.simulation.soft import SoftReadout
    if "ch" not in _CACHE:
        _CACHE["ch"] = {"gaussian": SoftReadout.gaussian(0.5, 8), "three": SoftReadout([0.02, 0.0, 0.005], [0.1, 0.3, 0.575]), "hard": SoftReadout.hard(0.02),
                        "help": SoftReadout.gaussian(HELP_SIGMA, 8)}
    return _CACHE["ch"]


def setup(L):
    """circuit_setup of circ72 plus, once: the fault signatures, the sampler model, and per channel the soft tables and marginal priors of both sectors"""
    if "s" not in _CACHE:
        from qldpc_amd.simulation.soft import marginal_priors, soft_tables_from_circuit
        c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, "circ72")
        sigs = (L.circuit_fault_signatures(compiled, c["Lx"], c["Lz"], False), L.circuit_fault_signatures(compiled, c["Lx"], c["Lz"], True))
        model = SM.SamplerModel(sigs[0], sigs[1], np.asarray(compiled.base_ops), (graphs[0].m, graphs[1].m), np.asarray(c["Lx"]).shape[0])
        tables = {k: soft_tables_from_circuit(compiled, c["Lx"], c["Lz"], M, r, signatures=sigs) for k, r in channels().items()}
        marg = {k: marginal_priors(M, tables[k], r) for k, r in channels().items()}

        def plan_with(prior, batch=128, **kw):
            """circuit_setup's plan with other priors for the same columns"""
            return L.CircuitPlan(compiled, c["Lx"], c["Lz"], graphs[0], graphs[1], prior[0], prior[1], masks[0], masks[1], P, batch=batch, **kw)
        _CACHE["s"] = (c, compiled, M, graphs, priors, masks, plan, sigs, model, tables, marg, plan_with)
    return _CACHE["s"]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


# ---------------------------------------------------------------------------------------- 1. the sampler equals the model
@pytest.mark.parametrize("which", ["gaussian", "three", "hard"])
def test_sample_soft_equals_the_model(L, which):
    c, compiled, M, graphs, priors, masks, plan, sigs, model, tables, marg, plan_with = setup(L)
    assert graphs[0].m == graphs[1].m == 288 and (graphs[0].n, graphs[1].n) == (2233, 2269)
    r = channels()[which]
    p = plan(batch=128)                                                    # three batches
    assert p.n_meas == model.meas.size == 432
    today = p.sample(SEED, 0, COUNT)
    p.use_soft_readout(r)
    spz, tz, spx, tx, lv = p.sample_soft(SEED, 0, COUNT)
    wz, wtz, wx, wtx, wlv, wflip = model.sample(P, r.cut, SEED, 0, COUNT)
    assert lv.shape == (COUNT, 432) and lv.dtype == np.uint8
    assert np.array_equal(lv, wlv)
    assert np.array_equal(spz, wz) and np.array_equal(tz, wtz) and np.array_equal(spx, wx) and np.array_equal(tx, wtx)
    w = np.diff([0] + r.cut)
    assert set(np.unique(lv).tolist()) == {k for k in range(r.levels) if w[k] + w[r.levels + k] > 0}      # every level with mass occurs
    # the flipped readouts: against the plain sample the syndromes differ by exactly the signatures of the model's flipped readouts, and their number
    # is the marginal rate's (within six standard deviations of Binomial(384 * 432, qbar))
    ty = model.loc_type[model.meas]
    for s, (got, base, op) in enumerate(((spz, today[0], SM.OP_MEAS_X), (spx, today[2], SM.OP_MEAS_Z))):
        D = model.tabs[s][0][2 * model.meas[ty == op]].astype(np.int64)
        assert np.array_equal((got ^ base).astype(np.int64), (wflip[:, ty == op].astype(np.int64) @ D) & 1)
    n = COUNT * 432
    assert abs(int(wflip.sum()) - n * r.qbar) <= 6 * np.sqrt(n * r.qbar * (1 - r.qbar)) and wflip.sum() > 0
    assert same(p.sample(SEED, 0, COUNT), (spz, tz, spx, tx))              # sample() honours the switch too
    assert same(p.sample_erasures(SEED, 0, COUNT)[:4], (spz, tz, spx, tx)) and not p.sample_erasures(SEED, 0, COUNT)[4].any()
    p.close()


def test_switch_off_is_todays_sampler(L):
    plan = setup(L)[6]
    p = plan(batch=128)
    today = p.sample(SEED, 0, COUNT)
    off = p.sample_soft(SEED, 0, COUNT)                                    # never switched on
    assert same(off[:4], today) and not off[4].any() and off[4].shape == (COUNT, 432)
    p.use_soft_readout(channels()["gaussian"])
    on = p.sample_soft(SEED, 0, COUNT)
    assert on[4].any() and not np.array_equal(on[0], today[0])
    p.use_soft_readout(None)                                               # two-way
    again = p.sample_soft(SEED, 0, COUNT)
    assert same(again[:4], today) and not again[4].any() and same(p.sample(SEED, 0, COUNT), today) and p.soft_readout is None
    p.close()


# ---------------------------------------------------------------------------------------- 2. batching and position
def test_batching_and_position_independence(L):
    plan = setup(L)[6]
    outs = {}
    for batch in (64, 512):
        p = plan(batch=batch)
        p.use_soft_readout(channels()["gaussian"])
        outs[batch] = p.sample_soft(SEED, 0, COUNT)
        if batch == 64:
            part = p.sample_soft(SEED, 100, 64)
        p.close()
    assert same(outs[64], outs[512])
    assert same(part, [x[100:164] for x in outs[512]])


# ---------------------------------------------------------------------------------------- 3. the prior kernel equals the model
@pytest.mark.parametrize("which", ["gaussian", "three", "hard"])
def test_soft_priors_on_the_circuit_tables(L, which):
    c, compiled, M, graphs, priors, masks, plan, sigs, model, tables, marg, plan_with = setup(L)
    r, t = channels()[which], tables[which]
    for s in range(2):
        name = "ZX"[s]
        probs = np.asarray(M[f"channel_probs{name}"], np.float64)
        want = SM.build_tables(model.loc_type, sigs[s], bool(s), SM.columns_of(M[f"Hdec{name}"].toarray(), masks[s]), graphs[s].n, probs, r.cut)
        assert same(SM.as_tuple(t[s])[:4], SM.as_tuple(want)[:4]) and t[s].unmatched == want["unmatched"] == 0 and t[s].levels == r.levels
        assert (t[s].meas_col >= 0).sum() == 216 and (t[s].meas_col < 0).sum() == 216          # the sector's own class, each on a column
        assert np.array_equal(marg[which][s], SM.marginal_priors(probs, t[s].meas_col, r.qbar))
        free = np.bincount(t[s].meas_col[t[s].meas_col >= 0], minlength=graphs[s].n) == 0
        assert np.array_equal(marg[which][s][free], priors[s][free]) and np.array_equal(t[s].lut[t[s].lut_ptr[:-1][free]], priors[s][free])
    p = plan_with(marg[which])
    p.use_soft_aware(1.0, t)
    p.use_soft_readout(r)
    *_, lv, pz, px = p.sample_soft(SEED, 0, 96, want_priors=True)
    for s, got in enumerate((pz, px)):
        want = SM.priors(lv, t[s])
        assert np.array_equal(got, want) and np.array_equal(L.soft_priors(lv, t[s]), want)
        measured = np.bincount(t[s].meas_col[t[s].meas_col >= 0], minlength=graphs[s].n) > 0
        assert np.array_equal(got[:, ~measured], np.tile(priors[s][~measured], (96, 1)))
        if r.levels > 1:
            assert (got[:, measured].max(axis=0) > got[:, measured].min(axis=0)).all()            # every measured column saw two levels in 96 shots
    p.close()


def hand_tables(n_meas, n, K, seed):
    """random tables: column 0 has no measurement, column 1 one, column 2 two, column 3 three, column 4 four where K = 16 (a run of exactly 65536
    entries); the rest 0 .. 3 as far as the measurements go, the last measurement touches no column; lut values arbitrary (the kernel only looks up)"""
    rng = np.random.default_rng(seed)
    want = [0, 1, 2, 3] + ([4] if K == 16 else []) + [int(rng.integers(0, 4)) for _ in range(n)]
    col_of = []
    for j in range(n):
        take = min(want[j], n_meas - 1 - len(col_of))
        col_of += [j] * take
    col_of += [-1] * (n_meas - len(col_of))
    meas_col = np.array(col_of, np.int32)
    rng.shuffle(meas_col[:-1])
    assert meas_col[-1] == -1
    meas_w, c = np.ones(n_meas, np.int32), np.zeros(n, np.int64)
    for k, j in enumerate(meas_col):
        if j >= 0:
            meas_w[k] = K ** c[j]
            c[j] += 1
    assert c[:4].tolist() == [0, 1, 2, 3] and (K != 16 or c[4] == 4)
    lut_ptr = np.concatenate([[0], np.cumsum(K ** c)]).astype(np.int32)
    return meas_col, meas_w, lut_ptr, rng.normal(size=int(lut_ptr[-1])) * 7, K


@pytest.mark.parametrize("K", [1, 3, 16])
@pytest.mark.parametrize("n_meas,n,B", [(45, 37, 9), (97, 130, 33), (64, 32, 4200)])
def test_soft_priors_on_hand_made_tables(L, n_meas, n, B, K):
    """n off and on the two columns a counter word packs; columns with 0, 1, 2 and 3 measurements, and with K = 16 one of 4 (65536 entries, the
    largest run); a shot with every level K - 1 (the last entry of every run), one with all 0; more shots than the grid has workgroups"""
    t = hand_tables(n_meas, n, K, 5)
    meas_col, meas_w, lut_ptr, lut, _ = t
    rng = np.random.default_rng(B)
    levels = rng.integers(0, K, size=(B, n_meas)).astype(np.uint8)
    levels[0], levels[1] = K - 1, 0
    got = L.soft_priors(levels, t)
    want = SM.priors(levels, t)
    assert np.array_equal(got, want)
    assert np.array_equal(got[1], lut[lut_ptr[:-1]]) and np.array_equal(got[0], lut[lut_ptr[1:] - 1])
    assert np.diff(lut_ptr)[:4].tolist() == [1, K, K ** 2, K ** 3] and (K != 16 or lut_ptr[5] - lut_ptr[4] == 65536)


def test_malformed_tables_and_levels_are_refused(L):
    mc, mw, up, lu, K = hand_tables(45, 37, 3, 5)
    levels = np.zeros((2, 45), np.uint8)
    k2 = int(np.flatnonzero(mc == 2)[1])                                   # the second measurement of column 2: weight 3
    bad_col, bad_w, bad_ptr, bad_lut, bad_lv = mc.copy(), mw.copy(), up.copy(), lu.copy(), levels.copy()
    bad_col[3], bad_w[k2], bad_ptr[37], bad_lut[11], bad_lv[1, 7] = 37, 1, up[37] + 1, np.nan, 3
    for lv, t, text in ((levels, (bad_col, mw, up, lu, K), "meas_col[3] = 37"), (levels, (mc, bad_w, up, lu, K), f"meas_w[{k2}] = 1"),
                        (levels, (mc, mw, bad_ptr, np.append(lu, 0.0), K), "lut_ptr[37] - lut_ptr[36]"), (levels, (mc, mw, up, bad_lut, K), "lut[11] is not finite"),
                        (bad_lv, (mc, mw, up, lu, K), "level[1][7] = 3"), (levels, (mc, mw, up, lu, 17), "levels = 17"),
                        (np.zeros((1, 5), np.uint8), (np.zeros(5, np.int32), 16 ** np.arange(5, dtype=np.int32), np.array([0, 16 ** 5], np.int32), np.zeros(16 ** 5), 16),
                         "column 0: measurement 4 brings its run to 1048576 entries")):
        with pytest.raises(L.QldpcError, match="error -1") as ei:
            L.soft_priors(lv, t)
        assert text in str(ei.value), str(ei.value)


# ---------------------------------------------------------------------------------------- 4. the plan equals the chain of its parts
def truths_of(tz, tx):
    k = tz.shape[1]
    return [(t.astype(np.uint64) << np.arange(k, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint64) for t in (tz, tx)]


def verdicts(masks, dets, truths):
    truth = truths_of(*truths)
    return sum(((logical_bits(d, masks[s]) != truth[s]).astype(np.uint8) << s) for s, d in enumerate(dets)).astype(np.uint8)


@pytest.mark.parametrize("how", ["aware", "aware+osd_cs", "aware, readout off"])
def test_the_plan_equals_the_chain_of_its_parts(L, how):
    c, compiled, M, graphs, priors, masks, plan, sigs, model, tables, marg, plan_with = setup(L)
    r, t, mp = channels()["gaussian"], tables["gaussian"], marg["gaussian"]
    alpha = 0.875 if how == "aware" else 1.0
    p = plan_with(mp)
    if how.endswith("osd_cs"):
        p.use_osd_cs(5)
    p.use_soft_aware(alpha, t)
    if not how.endswith("off"):
        p.use_soft_readout(r)
    got = p.run_outcomes(SEED, 0, COUNT)
    tally = p.read(clear=True)
    spz, tz, spx, tx, lv, pz, px = p.sample_soft(SEED, 0, COUNT, want_priors=True)
    assert pz.shape == (COUNT, graphs[0].n) and px.shape == (COUNT, graphs[1].n)
    if how.endswith("off"):                                                # no levels: the plan decodes with its own prior at stride 0
        pz, px = np.tile(mp[0], (COUNT, 1)), np.tile(mp[1], (COUNT, 1))
    dets, convs = aware_chain(L, graphs, (spz, spx), (pz, px), alpha, (5, mp) if how.endswith("osd_cs") else None)      # the plan's prior scores: the documented limitation
    assert np.array_equal(got, verdicts(masks, dets, (tz, tx))), how
    assert_aware_tally(L, tally, COUNT, convs)
    assert 0 < convs[0].sum() < COUNT                                       # both stages took part
    if how.endswith("off"):
        assert not lv.any()
        q = plan_with(mp)
        q.use_correlated(alpha, None)
        assert np.array_equal(q.run_outcomes(SEED, 0, COUNT), got)
        q.close()
    else:
        assert lv.any() and np.array_equal(pz, SM.priors(lv, t[0]))
    p.close()


def test_the_unaware_plan_decodes_the_sampled_syndromes_as_ever(L):
    c, compiled, M, graphs, priors, masks, plan, sigs, model, tables, marg, plan_with = setup(L)
    p = plan(batch=128)
    p.use_soft_readout(channels()["gaussian"])
    got = p.run_outcomes(SEED, 0, COUNT)
    spz, tz, spx, tx, lv = p.sample_soft(SEED, 0, COUNT)
    p.close()
    q = plan(batch=128)                                                    # an untouched plan
    pred0, pred1, _ = q.decode_events(L.pack_events(np.hstack([spz, spx])))
    q.close()
    truth = truths_of(tz, tx)
    assert np.array_equal(got, (pred0 != truth[0]).astype(np.uint8) | ((pred1 != truth[1]).astype(np.uint8) << 1))
    assert lv.any() and np.count_nonzero(got) > 0


def test_the_levels_help(L):
    """Same trials, same noise, both plans with the marginal priors: the aware plan fails strictly less often than the unaware one.  The kernels
    equal the numpy models bit for bit, so the counts are deterministic.  sigma = 0.5 (8 levels, qbar = 0.0228) and seed 2031 were fixed with the
    model chain -- soft_model's sampler and priors, correlated_model.decode (alpha 1, clip 20, 50 iterations) and the oracle's OSD-0 on the BP
    failures -- which fails 186 of 384 trials unaware and 154 aware (sigma = 0.45: 150 and 137; sigma = 0.4: 139 and 129); the plans must give
    those counts."""
    c, compiled, M, graphs, priors, masks, plan, sigs, model, tables, marg, plan_with = setup(L)
    r, t, mp = channels()["help"], tables["help"], marg["help"]
    fails = {}
    for aware in (False, True):
        p = plan_with(mp)
        p.use_correlated(1.0, None) if not aware else p.use_soft_aware(1.0, t)      # the same kernel and alpha on both sides: only the prior differs
        p.use_soft_readout(r)
        fails[aware] = int(np.count_nonzero(p.run_outcomes(HELP_SEED, 0, COUNT)))
        p.close()
    print("levels help:", fails)
    assert fails[True] < fails[False], fails
    assert (fails[False], fails[True]) == (MODEL_UNAWARE, MODEL_AWARE), fails


MODEL_UNAWARE, MODEL_AWARE = 186, 154


# ---------------------------------------------------------------------------------------- 5. switch rules
ALL = dict(SWITCHES, lsd=("BP + LSD", lambda p: p.use_lsd(), lambda p: p.use_lsd(max_rows=128)),
           correlated=("correlated decoding", lambda p: p.use_correlated(), lambda p: p.use_correlated(0.875)))
GOES_WITH = {"osd_cs", "lsd"}


def test_the_new_row_and_column_of_the_switch_table(L):
    c, compiled, M, graphs, priors, masks, plan, sigs, model, tables, marg, plan_with = setup(L)
    from qldpc_amd.simulation.erasure import erasure_tables_from_circuit
    t, r = tables["gaussian"], channels()["gaussian"]
    era = erasure_tables_from_circuit(compiled, c["Lx"], c["Lz"], M, signatures=sigs)
    every = dict(ALL, erasure=("erasure-aware decoding", lambda p: p.use_erasure_aware(1.0, era), None))
    SOFT = ("soft-aware decoding", lambda p: p.use_soft_aware(1.0, t), lambda p: p.use_soft_aware(0.875, t))
    assert len(every) == 9
    for other, (name, call, _) in every.items():
        p = plan(batch=BATCH)                                              # the row: soft-aware first
        SOFT[1](p)
        if other in GOES_WITH:
            call(p)
            run64(L, p)
        else:
            refused(L, p, call, SOFT[0], name)
        p.close()
        p = plan(batch=BATCH)                                              # the column: soft-aware second
        call(p)
        if other in GOES_WITH:
            SOFT[1](p)
            run64(L, p)
        else:
            refused(L, p, SOFT[1], name, SOFT[0])
        p.close()
    p = plan(batch=BATCH)                                                  # asked again: new arguments
    SOFT[1](p)
    p.use_soft_readout(r)
    a = p.run_outcomes(7, 0, BATCH)
    SOFT[2](p)
    b = p.run_outcomes(7, 0, BATCH)
    SOFT[1](p)
    assert np.array_equal(p.run_outcomes(7, 0, BATCH), a) and a.shape == b.shape
    p.read(clear=True)
    before = run64(L, p)
    mc, mw, up, lu, K = SM.as_tuple(t[1])
    free = int(np.flatnonzero(np.diff(up) == 1)[5])                        # a column without measurements: its entry is the plan's prior
    shifted, w2 = lu.copy(), mw.copy()
    shifted[up[free]] += 1.0
    w2[int(np.flatnonzero(mc >= 0)[0])] = 2
    for bad, text in (((t[0], (mc, w2, up, lu, K)), "sector X: meas_w["), ((t[0], (mc, mw, up, shifted, K)), f"sector X: lut[lut_ptr[{free}]]"),
                      ((t[1], t[1]), "lut_ptr has"), ((t[0], tables["three"][1]), "levels"), (tables["three"], "8 levels")):
        with pytest.raises((L.QldpcError, ValueError)) as ei:
            p.use_soft_aware(1.0, bad)
        assert text in str(ei.value), str(ei.value)
    with pytest.raises(ValueError):
        p.use_soft_aware(0.0, t)
    with pytest.raises(L.QldpcError, match=r"error -1: .*tables for 8 levels"):  # ... and a readout with other levels than the tables in force
        p.use_soft_readout(channels()["three"])
    assert np.array_equal(run64(L, p), before) and p.soft_readout is r
    p.close()
    p = plan(batch=BATCH, damping=0.5)
    refused(L, p, SOFT[1], SOFT[0], "damping = 1", reason="damping")
    p.close()
    p = plan(batch=BATCH, use_osd=False)                                   # BP alone: no OSD stage is needed
    SOFT[1](p)
    tl = run64(L, p)
    assert tl[L.TALLY["osd_z"]] == 0 and tl[L.TALLY["osd_x"]] == 0
    p.close()


def test_the_sampler_axis_and_its_refusals(L):
    from qldpc_amd.simulation.noise_model import NoiseModel
    plan, tables = setup(L)[6], setup(L)[9]
    r = channels()["gaussian"]
    for name, (_, call, _) in ALL.items():                                 # it asks no switch rule: every path and OSD stage, either order
        q = plan(batch=BATCH)
        q.use_soft_readout(r)
        call(q)
        run64(L, q)
        q.close()
        q = plan(batch=BATCH)
        call(q)
        q.use_soft_readout(r)
        run64(L, q)
        q.close()
    p = plan(batch=BATCH)
    today = p.sample(3, 0, BATCH)
    others = (("fixed weight", lambda: p.use_fixed_weight(5), lambda: p.use_fixed_weight(None)),
              ("erasure noise", lambda: p.use_erasure_noise({"CNOT": 0.02}), lambda: p.use_erasure_noise(None)),
              ("noise model", lambda: p.use_noise_model(NoiseModel(0.004)), lambda: p.use_noise_model(None)))
    for text, on, off in others:
        on()                                                               # the other switch first: soft readout is refused
        theirs = p.sample(3, 0, BATCH)
        with pytest.raises(L.QldpcError, match=rf"error -1: .*{text}"):
            p.use_soft_readout(r)
        assert same(p.sample(3, 0, BATCH), theirs) and p.soft_readout is None
        off()
        p.use_soft_readout(r)                                              # soft readout first: the other is refused, switching it off is not
        noisy = p.sample_soft(3, 0, BATCH)
        with pytest.raises(L.QldpcError, match=r"error -1: .*soft readout"):
            on()
        off()
        assert same(p.sample_soft(3, 0, BATCH), noisy) and noisy[4].any()
        p.use_soft_readout(None)
        assert same(p.sample(3, 0, BATCH), today)
    p.use_soft_readout(r)
    noisy = p.sample_soft(3, 0, BATCH)
    import ctypes as C
    flip, keep = np.array([0.1, np.nan, 0.1]), np.array([0.5, 0.5, 0.5])
    lib = L.lib()
    assert lib.qldpc_circuit_plan_use_soft_readout(p._h, 3, L.ptr(flip, C.c_double), L.ptr(keep, C.c_double)) == -1 and b"flip_mass[1]" in lib.qldpc_last_error()
    flip[1], keep[2] = 0.1, -1.0
    assert lib.qldpc_circuit_plan_use_soft_readout(p._h, 3, L.ptr(flip, C.c_double), L.ptr(keep, C.c_double)) == -1 and b"keep_mass[2]" in lib.qldpc_last_error()
    flip[1], keep[1], keep[2] = 0.0, 0.0, 0.5
    assert lib.qldpc_circuit_plan_use_soft_readout(p._h, 3, L.ptr(flip, C.c_double), L.ptr(keep, C.c_double)) == -1 and b"level 1 has no mass" in lib.qldpc_last_error()
    assert lib.qldpc_circuit_plan_use_soft_readout(p._h, 17, L.ptr(flip, C.c_double), L.ptr(keep, C.c_double)) == -1 and b"levels = 17" in lib.qldpc_last_error()
    with pytest.raises(ValueError):
        p.use_soft_readout(([0.1], [0.9]))
    assert same(p.sample_soft(3, 0, BATCH), noisy)
    with pytest.raises(L.QldpcError, match=r"error -1: .*use_soft_aware"):     # the priors need the path's tables
        p.sample_soft(3, 0, BATCH, want_priors=True)
    p.use_soft_readout(None)
    assert same(p.sample(3, 0, BATCH), today)
    p.close()
    toy = CM.toy_dem()                                                     # a DEM plan has no measurement locations
    views = [toy.decoder_view(s) for s in range(2)]
    d = toy.plan([L.Graph(v.indptr, v.indices, v.shape[1]) for v in views], batch=BATCH)
    before, sampled = run64(L, d), d.sample(3, 0, BATCH)
    with pytest.raises(L.QldpcError, match=r"error -1: .*circuit plan"):
        d.use_soft_readout(r)
    with pytest.raises(L.QldpcError, match=r"error -1: .*circuit plan"):
        d.sample_soft(3, 0, BATCH)
    assert lib.qldpc_circuit_plan_use_soft_aware(d._h, 1.0, 8, *([None] * 8)) == -1 and b"circuit plan" in lib.qldpc_last_error()
    assert np.array_equal(run64(L, d), before) and same(d.sample(3, 0, BATCH), sampled)
    d.close()


# ---------------------------------------------------------------------------------------- 6. run_simulation
def test_run_simulation_soft(L):
    from qldpc_amd.data import load_code, load_precomputed_matrices
    from qldpc_amd.simulation.engine import run_simulation
    c, compiled, M, graphs, priors, masks, plan, sigs, model, tables, marg, plan_with = setup(L)
    code = load_code("bb72")
    kw = dict(num_cycles=6, precomputed_matrices=load_precomputed_matrices("circ72"), base_seed=SEED, batch=512, **_bb_params(code))
    args = (code["Hx"], code["Hz"], code["Lx"], code["Lz"], P)
    so = {"sigma": 0.5, "levels": 8, "aware": True, "alpha": 1.0}
    r1 = run_simulation(*args, num_trials=1500, devices=[0], soft=so, **kw)
    r2 = run_simulation(*args, num_trials=1500, num_workers=2, devices=[0, 0], soft=so, **kw)
    assert r1["tally"][L.TALLY["trials"]] == 1500 and np.array_equal(r1["tally"], r2["tally"]) and r2["num_workers"] == 2
    assert r1["soft"]["aware"] is True and r1["soft"]["alpha"] == 1.0 and r1["soft"]["readout"].cut == channels()["gaussian"].cut and r1["matched_priors"] is True
    p = plan_with(marg["gaussian"], batch=512)
    p.use_soft_aware(1.0, tables["gaussian"])
    p.use_soft_readout(channels()["gaussian"])
    p.run(SEED, 0, 1500)
    assert np.array_equal(p.read(), r1["tally"])
    p.close()
    un = {"readout": channels()["gaussian"], "aware": False}
    r3 = run_simulation(*args, num_trials=600, devices=[0], soft=un, decoder="bp_osd_cs", osd_order=5, **kw)
    r4 = run_simulation(*args, num_trials=600, devices=[0], soft=un, decoder="bp_osd_cs", osd_order=5, matched_priors=False, **kw)
    for res, prior in ((r3, marg["gaussian"]), (r4, priors)):
        p = plan_with(prior, batch=512)
        p.use_osd_cs(5)
        p.use_soft_readout(channels()["gaussian"])
        p.run(SEED, 0, 600)
        assert np.array_equal(p.read(), res["tally"]) and res["decoder"] == "bp_osd_cs" and res["soft"]["aware"] is False
        p.close()
    assert r3["matched_priors"] is True and r4["matched_priors"] is False and not np.array_equal(r3["tally"], r4["tally"])
    r0 = run_simulation(*args, num_trials=600, devices=[0], **kw)
    assert "soft" not in r0 and not np.array_equal(r0["tally"], r4["tally"])
