"""Heralded-erasure noise and erasure-aware decoding on a circuit plan, on circ72 -- the small plan of tests/test_plan_switch_gpu.py -- and on hand-made
tables: the sampler and the prior kernel equal the numpy model of tests/erasure_model.py bit for bit, batching and position do not matter, the plan
equals the chain of its parts verdict for verdict, the switch rules gain one row and one column and the sampler axis its refusals, and
run_simulation(erasure=...) equals the plan driven by hand."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import correlated_model as CM  # noqa: E402
import erasure_model as EM  # noqa: E402
from test_correlated_gpu import logical_bits  # noqa: E402
from test_plan_switch_gpu import BASE_SWITCHES as SWITCHES, refused, run64, BATCH  # noqa: E402
from test_relay_gpu import _bb_params, circuit_setup  # noqa: E402

pytestmark = pytest.mark.gpu

SEED, COUNT, P = 2031, 384, 0.005                                          # (P: what circuit_setup's plans sample at)
RATES = {"cnot": {"CNOT": 0.02}, "all": 0.01, "mixed": {"CNOT": 0.03, "PrepX": 0.02, "PrepZ": 0.0, "MeasX": 0.05, "MeasZ": 0.01, "IDLE": 0.004}}
_CACHE = {}


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


def setup(L):
    """circuit_setup of circ72 plus, once: the fault signatures, the sampler model and the erasure tables of both sectors"""
    if "s" not in _CACHE:
        from qldpc_amd.simulation.erasure import erasure_tables_from_circuit
        c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, "circ72")
        sigs = (L.circuit_fault_signatures(compiled, c["Lx"], c["Lz"], False), L.circuit_fault_signatures(compiled, c["Lx"], c["Lz"], True))
        model = EM.SamplerModel(sigs[0], sigs[1], np.asarray(compiled.base_ops), (graphs[0].m, graphs[1].m), np.asarray(c["Lx"]).shape[0])
        tables = erasure_tables_from_circuit(compiled, c["Lx"], c["Lz"], M, signatures=sigs)
        _CACHE["s"] = (c, compiled, M, graphs, priors, masks, plan, sigs, model, tables)
    return _CACHE["s"]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


# ---------------------------------------------------------------------------------------- 1. the sampler equals the model
@pytest.mark.parametrize("which", list(RATES))
def test_sample_erasures_equals_the_model(L, which):
    c, compiled, M, graphs, priors, masks, plan, sigs, model, tables = setup(L)
    assert graphs[0].m == graphs[1].m == 288 and (graphs[0].n, graphs[1].n) == (2233, 2269)
    p = plan(batch=128)                                                    # three batches
    p.use_erasure_noise(RATES[which])
    spz, tz, spx, tx, er = p.sample_erasures(SEED, 0, COUNT)
    wz, wtz, wx, wtx, werased = model.sample(P, RATES[which], SEED, 0, COUNT)
    assert er.shape == (COUNT, (model.N + 31) // 32) and er.dtype == np.uint32
    assert np.array_equal(er, EM.pack_heralds(werased))
    assert np.array_equal(spz, wz) and np.array_equal(tz, wtz) and np.array_equal(spx, wx) and np.array_equal(tx, wtx)
    ty = model.loc_type
    by_op = EM.rates_by_op(RATES[which])
    for op in range(1, 7):                                                 # a class at rate 0 is never erased; the others are, somewhere in 384 trials
        assert bool(werased[:, ty == op].any()) == (by_op[op] > 0), op
    assert same(p.sample(SEED, 0, COUNT), (spz, tz, spx, tx))              # sample() honours the switch too
    p.close()


def test_rate_zero_and_switch_off_are_todays_sampler(L):
    plan = setup(L)[6]
    p = plan(batch=128)
    today = p.sample(SEED, 0, COUNT)
    off = p.sample_erasures(SEED, 0, COUNT)                                # never switched on
    assert same(off[:4], today) and not off[4].any()
    p.use_erasure_noise(0.0)
    zero = p.sample_erasures(SEED, 0, COUNT)
    assert same(zero[:4], today) and not zero[4].any()
    p.use_erasure_noise({"CNOT": 0.02})
    on = p.sample_erasures(SEED, 0, COUNT)
    assert on[4].any() and not np.array_equal(on[0], today[0])
    p.use_erasure_noise(None)                                              # two-way
    assert same(p.sample_erasures(SEED, 0, COUNT)[:4], today) and same(p.sample(SEED, 0, COUNT), today)
    p.close()


# ---------------------------------------------------------------------------------------- 2. batching and position
def test_batching_and_position_independence(L):
    plan = setup(L)[6]
    outs = {}
    for batch in (64, 512):
        p = plan(batch=batch)
        p.use_erasure_noise(RATES["mixed"])
        outs[batch] = p.sample_erasures(SEED, 0, COUNT)
        if batch == 64:
            part = p.sample_erasures(SEED, 100, 64)
        p.close()
    assert same(outs[64], outs[512])
    assert same(part, [x[100:164] for x in outs[512]])


# ---------------------------------------------------------------------------------------- 3. the prior kernel equals the model
def test_erasure_priors_on_the_circuit_tables(L):
    c, compiled, M, graphs, priors, masks, plan, sigs, model, tables = setup(L)
    for s in range(2):
        name = "ZX"[s]
        want = EM.build_tables(model.loc_type, sigs[s], bool(s), EM.columns_of(M[f"Hdec{name}"].toarray(), masks[s]), graphs[s].n,
                               np.asarray(M[f"channel_probs{name}"], np.float64), priors[s])
        assert same(EM.as_tuple(tables[s]), EM.as_tuple(want)) and tables[s].unmatched == want["unmatched"] == 0
        assert (tables[s].loc_h == 1).any() and (tables[s].loc_h == EM.H_INF).any() and np.diff(tables[s].lut_ptr).max() > 2
    p = plan(batch=128)
    p.use_erasure_aware(1.0, tables)
    p.use_erasure_noise(RATES["all"])
    *_, er, pz, px = p.sample_erasures(SEED, 0, 96, want_priors=True)
    erased = EM.unpack_heralds(er, model.N)
    for s, got in enumerate((pz, px)):
        want = EM.priors(erased, tables[s])
        assert np.array_equal(got, want) and np.array_equal(L.erasure_priors(er, tables[s]), want)
        assert (got == 0.0).any() and (got != priors[s][None, :]).sum() > (got == 0.0).sum()      # INF entries and h = 1 entries both took part
    p.close()


def hand_tables(n_locs, n, seed):
    """random tables: column 0 has no contribution, column 1 only h = 1 ones, column 2 both kinds; lut values arbitrary (the kernel only looks up)"""
    rng = np.random.default_rng(seed)
    loc_ptr, loc_col, loc_h = [0], [], []
    for l in range(n_locs):
        cols = sorted(rng.choice(np.arange(1, n), size=int(rng.integers(0, 4)), replace=False).tolist()) if l % 7 else [1, 2]
        for j in cols:
            loc_col.append(j)
            loc_h.append(1 if j == 1 or (j == 2 and l % 2) or rng.random() < 0.5 else EM.H_INF)
        loc_ptr.append(len(loc_col))
    loc_col, loc_h = np.array(loc_col, np.int32), np.array(loc_h, np.uint8)
    c = np.bincount(loc_col[loc_h == 1], minlength=n)
    lut_ptr = np.concatenate([[0], np.cumsum(c + 1)]).astype(np.int32)
    assert c[0] == 0 and not (loc_col == 0).any() and c[1] > 2 and not (loc_h[loc_col == 1] == EM.H_INF).any()
    assert (loc_h[loc_col == 2] == 1).any() and (loc_h[loc_col == 2] == EM.H_INF).any()
    return np.array(loc_ptr, np.int32), loc_col, loc_h, lut_ptr, rng.normal(size=int(lut_ptr[-1])) * 7


@pytest.mark.parametrize("n_locs,n,B", [(45, 37, 9), (97, 130, 33), (64, 32, 4200)])
def test_erasure_priors_on_hand_made_tables(L, n_locs, n, B):
    """n and n_locs off every multiple the kernel packs by (2 columns per counter word, 32 per bit word, 32 locations per herald word) and on them;
    a shot with every location erased (H = c_j in every column without an INF entry), one with none; more shots than the grid has workgroups"""
    t = hand_tables(n_locs, n, 5)
    rng = np.random.default_rng(B)
    erased = rng.random((B, n_locs)) < 0.15
    erased[0], erased[1] = True, False
    words = EM.pack_heralds(erased)
    if n_locs % 32:
        words[2, -1] |= np.uint32(0xFFFFFFFF) << np.uint32(n_locs % 32)    # bits at or above n_locs are not locations
    got = L.erasure_priors(words, t)
    want = EM.priors(erased, t)
    assert np.array_equal(got, want)
    lut_ptr, lut = t[3], t[4]
    assert np.array_equal(got[1], lut[lut_ptr[:-1]])                        # no herald: the base row, bit for bit
    assert got[0, 1] == lut[lut_ptr[2] - 1] and got[0, 2] == 0.0 and got[0, 0] == lut[0]      # H = c_j; INF beside h = 1; no contribution


def test_malformed_tables_are_refused(L):
    lp, lc, lh, up, lu = hand_tables(45, 37, 5)
    words = np.zeros((2, 2), np.uint32)
    bad_col, bad_h, bad_lut = lc.copy(), lh.copy(), up.copy()
    bad_col[3], bad_h[4], bad_lut[37] = 37, 7, up[37] + 1
    for t, text in (((lp, bad_col, lh, up, lu), "loc_col[3] = 37"), ((lp, lc, bad_h, up, lu), "loc_h[4] = 7"),
                    ((lp, lc, lh, bad_lut, np.append(lu, 0.0)), "lut_ptr[37] - lut_ptr[36]")):
        with pytest.raises(L.QldpcError, match="error -1") as ei:
            L.erasure_priors(words, t)
        assert text in str(ei.value)


# ---------------------------------------------------------------------------------------- 4. the plan equals the chain of its parts
def verdicts(masks, dets, truths):
    k = truths[0].shape[1]
    truth = [(t.astype(np.uint64) << np.arange(k, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint64) for t in truths]
    return sum(((logical_bits(d, masks[s]) != truth[s]).astype(np.uint8) << s) for s, d in enumerate(dets)).astype(np.uint8)


def aware_chain(L, graphs, synds, shot_priors, alpha, cs=None, max_iter=50):
    """what a plan on a per-shot-prior path does with a batch, from its parts: per sector shotprior_decode_batch with prior[B][n] (stride n, no links),
    then on the BP failures OSD-0 or, with cs = (order, the scoring weights per sector), OSD-CS.  -> (corrections per sector, converged per sector)"""
    dets, convs = [], []
    for s, (synd, prior) in enumerate(zip(synds, shot_priors)):
        assert prior.shape == (synd.shape[0], graphs[s].n)
        det, llr, conv, _ = L.shotprior_decode_batch(graphs[s], synd, prior, alpha, 20.0, max_iter)
        failed = np.flatnonzero(conv == 0)
        if failed.size and cs is not None:
            det[failed] = L.osdcs_batch(graphs[s], synd[failed], llr[failed], det[failed], cs[1][s], cs[0])[0]
        elif failed.size:
            det[failed] = L.osd0_batch(graphs[s], synd[failed], llr[failed], det[failed])
        dets.append(det)
        convs.append(conv)
    return dets, convs


def assert_aware_tally(L, tally, count, convs):
    """the slots such a plan fills: every trial, the BP successes per sector, an OSD call per BP failure, no legs"""
    T = L.TALLY
    assert tally[T["trials"]] == count and tally[T["bp_conv_z"]] == convs[0].sum() and tally[T["bp_conv_x"]] == convs[1].sum()
    assert tally[T["osd_z"]] == count - convs[0].sum() and tally[T["osd_x"]] == count - convs[1].sum() and tally[T["legs_z"]] == 0


@pytest.mark.parametrize("how", ["aware", "aware+osd_cs", "aware, noise off"])
def test_the_plan_equals_the_chain_of_its_parts(L, how):
    c, compiled, M, graphs, priors, masks, plan, sigs, model, tables = setup(L)
    alpha = 0.875 if how == "aware" else 1.0
    p = plan(batch=128)
    if how.endswith("osd_cs"):
        p.use_osd_cs(5)
    p.use_erasure_aware(alpha, tables)
    if not how.endswith("off"):
        p.use_erasure_noise(RATES["cnot"])
    got = p.run_outcomes(SEED, 0, COUNT)
    tally = p.read(clear=True)
    spz, tz, spx, tx, er, pz, px = p.sample_erasures(SEED, 0, COUNT, want_priors=True)
    dets, convs = aware_chain(L, graphs, (spz, spx), (pz, px), alpha, (5, priors) if how.endswith("osd_cs") else None)      # the shared prior scores: the documented limitation
    assert np.array_equal(got, verdicts(masks, dets, (tz, tx))), how
    assert_aware_tally(L, tally, COUNT, convs)
    if how.endswith("off"):                                                # no heralds: the plan's prior, which is a correlated plan with no links
        assert 0 < convs[0].sum() < COUNT                                   # both stages took part
        assert not er.any() and np.array_equal(pz, np.tile(priors[0], (COUNT, 1))) and np.array_equal(px, np.tile(priors[1], (COUNT, 1)))
        q = plan(batch=128)
        q.use_correlated(alpha, None)
        assert np.array_equal(q.run_outcomes(SEED, 0, COUNT), got)
        q.close()
    else:
        assert er.any() and (pz == 0.0).any()
    p.close()


def test_the_heralds_help(L):
    """same trials, same noise: the aware plan fails no more often than the unaware one (384 trials at a CNOT erasure rate of 0.02: it fails far less)"""
    c, compiled, M, graphs, priors, masks, plan, sigs, model, tables = setup(L)
    fails = {}
    for aware in (False, True):
        p = plan(batch=128)
        if aware:
            p.use_erasure_aware(1.0, tables)
        p.use_erasure_noise(RATES["cnot"])
        fails[aware] = int(np.count_nonzero(p.run_outcomes(SEED, 0, COUNT)))
        p.close()
    assert fails[True] <= fails[False], fails


def test_the_unaware_plan_decodes_the_sampled_syndromes_as_ever(L):
    c, compiled, M, graphs, priors, masks, plan, sigs, model, tables = setup(L)
    p = plan(batch=128)
    p.use_erasure_noise(RATES["cnot"])
    got = p.run_outcomes(SEED, 0, COUNT)
    spz, tz, spx, tx, er = p.sample_erasures(SEED, 0, COUNT)
    p.close()
    q = plan(batch=128)                                                    # an untouched plan
    pred0, pred1, _ = q.decode_events(L.pack_events(np.hstack([spz, spx])))
    q.close()
    k = tz.shape[1]
    truth = [(t.astype(np.uint64) << np.arange(k, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint64) for t in (tz, tx)]
    assert np.array_equal(got, (pred0 != truth[0]).astype(np.uint8) | ((pred1 != truth[1]).astype(np.uint8) << 1))
    assert er.any() and np.count_nonzero(got) > 0


# ---------------------------------------------------------------------------------------- 5. switch rules
ALL = dict(SWITCHES, lsd=("BP + LSD", lambda p: p.use_lsd(), lambda p: p.use_lsd(max_rows=128)),
           correlated=("correlated decoding", lambda p: p.use_correlated(), lambda p: p.use_correlated(0.875)))
GOES_WITH = {"osd_cs", "lsd"}


def test_the_new_row_and_column_of_the_switch_table(L):
    plan, tables = setup(L)[6], setup(L)[9]
    ERA = ("erasure-aware decoding", lambda p: p.use_erasure_aware(1.0, tables), lambda p: p.use_erasure_aware(0.875, tables))
    assert len(ALL) == 8
    for other, (name, call, _) in ALL.items():
        p = plan(batch=BATCH)                                              # the row: erasure-aware first
        ERA[1](p)
        if other in GOES_WITH:
            call(p)
            run64(L, p)
        else:
            refused(L, p, call, ERA[0], name)
        p.close()
        p = plan(batch=BATCH)                                              # the column: erasure-aware second
        call(p)
        if other in GOES_WITH:
            ERA[1](p)
            run64(L, p)
        else:
            refused(L, p, ERA[1], name, ERA[0])
        p.close()
    p = plan(batch=BATCH)                                                  # asked again: new arguments
    ERA[1](p)
    p.use_erasure_noise(RATES["cnot"])
    a = p.run_outcomes(7, 0, BATCH)
    ERA[2](p)
    b = p.run_outcomes(7, 0, BATCH)
    ERA[1](p)
    assert np.array_equal(p.run_outcomes(7, 0, BATCH), a) and a.shape == b.shape
    p.read(clear=True)
    before = run64(L, p)
    lp, lc, lh, up, lu = EM.as_tuple(tables[1])
    shifted = lu.copy()
    shifted[up[5]] += 1.0
    for bad, text in (((tables[0], (lp, lc[::-1].copy(), lh, up, lu)), "loc_col["), ((tables[0], (lp, lc, lh, up, shifted)), "sector X: lut[lut_ptr[5]]"),
                      ((tables[1], tables[1]), "lut_ptr has")):
        with pytest.raises((L.QldpcError, ValueError)) as ei:
            p.use_erasure_aware(1.0, bad)
        assert text in str(ei.value), str(ei.value)
    with pytest.raises(ValueError):
        p.use_erasure_aware(0.0, tables)
    assert np.array_equal(run64(L, p), before)
    p.close()
    p = plan(batch=BATCH, damping=0.5)
    refused(L, p, ERA[1], ERA[0], "damping = 1", reason="damping")
    p.close()
    p = plan(batch=BATCH, use_osd=False)                                   # BP alone: no OSD stage is needed
    ERA[1](p)
    t = run64(L, p)
    assert t[L.TALLY["osd_z"]] == 0 and t[L.TALLY["osd_x"]] == 0
    p.close()


def test_the_sampler_axis_and_its_refusals(L):
    plan, tables = setup(L)[6], setup(L)[9]
    p = plan(batch=BATCH)
    for name, (_, call, _) in ALL.items():                                 # it asks no switch rule: every path and OSD stage, either order
        q = plan(batch=BATCH)
        q.use_erasure_noise(0.01)
        call(q)
        run64(L, q)
        q.close()
        q = plan(batch=BATCH)
        call(q)
        q.use_erasure_noise(0.01)
        run64(L, q)
        q.close()
    today = p.sample(3, 0, BATCH)
    p.use_fixed_weight(5)                                                  # fixed weight first: erasure noise is refused
    fixed = p.sample(3, 0, BATCH)
    with pytest.raises(L.QldpcError, match=r"error -1: .*fixed weight"):
        p.use_erasure_noise(0.01)
    assert same(p.sample(3, 0, BATCH), fixed) and p.erasure_rates is None
    p.use_fixed_weight(None)
    p.use_erasure_noise({"CNOT": 0.02})                                    # erasure noise first: a fixed weight is refused, switching it off is not
    noisy = p.sample_erasures(3, 0, BATCH)
    with pytest.raises(L.QldpcError, match=r"error -1: .*erasure noise"):
        p.use_fixed_weight(5)
    p.use_fixed_weight(None)
    assert same(p.sample_erasures(3, 0, BATCH), noisy) and noisy[4].any() and p.fixed_weight is None
    for bad in ({"CNOT": 1.0}, -0.5):
        with pytest.raises(ValueError):
            p.use_erasure_noise(bad)
    rate = np.array([0, 0.1, 0.1, np.nan, 0.1, 0.1, 0.1])
    import ctypes as C
    assert L.lib().qldpc_circuit_plan_use_erasure_noise(p._h, L.ptr(rate, C.c_double)) == -1 and b"rate[3]" in L.lib().qldpc_last_error()
    assert same(p.sample_erasures(3, 0, BATCH), noisy)
    with pytest.raises(L.QldpcError, match=r"error -1: .*use_erasure_aware"):  # the priors need the path's tables
        p.sample_erasures(3, 0, BATCH, want_priors=True)
    p.use_erasure_noise(None)
    assert same(p.sample(3, 0, BATCH), today)
    p.close()
    toy = CM.toy_dem()                                                     # a DEM plan has no gate locations
    views = [toy.decoder_view(s) for s in range(2)]
    d = toy.plan([L.Graph(v.indptr, v.indices, v.shape[1]) for v in views], batch=BATCH)
    before, sampled = run64(L, d), d.sample(3, 0, BATCH)
    with pytest.raises(L.QldpcError, match=r"error -1: .*circuit plan"):
        d.use_erasure_noise(0.01)
    with pytest.raises(L.QldpcError, match=r"error -1: .*circuit plan"):
        d.sample_erasures(3, 0, BATCH)
    assert L.lib().qldpc_circuit_plan_use_erasure_aware(d._h, 1.0, *([None] * 10)) == -1 and b"circuit plan" in L.lib().qldpc_last_error()
    assert np.array_equal(run64(L, d), before) and same(d.sample(3, 0, BATCH), sampled)
    d.close()


# ---------------------------------------------------------------------------------------- 6. run_simulation
def test_run_simulation_erasure(L):
    from qldpc_amd.data import load_code, load_precomputed_matrices
    from qldpc_amd.simulation.engine import run_simulation
    plan, tables = setup(L)[6], setup(L)[9]
    c = load_code("bb72")
    kw = dict(num_cycles=6, precomputed_matrices=load_precomputed_matrices("circ72"), base_seed=SEED, batch=512, **_bb_params(c))
    args = (c["Hx"], c["Hz"], c["Lx"], c["Lz"], P)
    er = {"rates": {"CNOT": 0.02}, "aware": True, "alpha": 1.0}
    r1 = run_simulation(*args, num_trials=1500, devices=[0], erasure=er, **kw)
    r2 = run_simulation(*args, num_trials=1500, num_workers=2, devices=[0, 0], erasure=er, **kw)
    assert r1["tally"][L.TALLY["trials"]] == 1500 and np.array_equal(r1["tally"], r2["tally"]) and r2["num_workers"] == 2
    assert r1["erasure"]["aware"] is True and r1["erasure"]["alpha"] == 1.0 and r1["erasure"]["rates"].tolist() == [0, 0.02, 0, 0, 0, 0, 0]
    p = plan(batch=512)
    p.use_erasure_aware(1.0, tables)
    p.use_erasure_noise({"CNOT": 0.02})
    p.run(SEED, 0, 1500)
    assert np.array_equal(p.read(), r1["tally"])
    p.close()
    un = dict(er, aware=False)
    r3 = run_simulation(*args, num_trials=600, devices=[0], erasure=un, decoder="bp_osd_cs", osd_order=5, **kw)
    p = plan(batch=512)
    p.use_osd_cs(5)
    p.use_erasure_noise({"CNOT": 0.02})
    p.run(SEED, 0, 600)
    assert np.array_equal(p.read(), r3["tally"]) and r3["decoder"] == "bp_osd_cs" and r3["erasure"]["aware"] is False
    p.close()
    r0 = run_simulation(*args, num_trials=600, devices=[0], **kw)
    assert "erasure" not in r0 and not np.array_equal(r0["tally"], r3["tally"])
