"""BP+LSD and its confidence behind every decode path of a plan, on the MI355X: the plan against the chain of tests/plan_pairs.py -- the path's batch
decoder per sector, qldpc_lsd_stats_batch on its failures, the judge and lsd_stats_model's scores in numpy -- outcome for outcome, slot for slot and
score for score, on hgp (sectors of 280 and 315 detectors and unequal width).  Then the dependency of correlated decoding on LSD's solution, the events
door, one-sector plans, the histogram sizes, a fixed-weight sampler in front of LSD, and run_simulation per path family.  Every comparison is exact.
Every case asserts that both stages worked in both sectors; the constants below were chosen so that they do, with the observed counts beside them."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lsd_stats_model as SM  # noqa: E402
import plan_pairs as PP  # noqa: E402
import test_circuit_shapes_cpu as TC  # noqa: E402
from test_circuit_shapes_gpu import AWARE_RATES  # noqa: E402
from test_lsd_stats_gpu import EDGES  # noqa: E402
from test_relay_gpu import _bb_params, circuit_setup  # noqa: E402

pytestmark = pytest.mark.gpu

NONE = np.uint64(SM.NONE)
SEED = TC.SEED
COUNT, BATCH = 300, 128                                                    # two full batches and a ragged third of 44
LSD_PARAMS = ((1, 512), (4, 24))                                           # (bits_per_step, max_rows): nothing capped; a cap that ends some shots with flag 1
# guided decimation: a first round and three more of ten iterations, eight columns frozen after each.  The posterior of a frozen column is
# s_j +- fix_llr with |s_j| <= (column degree) * alpha * clip_llr (include/qldpc_hip.h at qldpc_decim_decode_batch: "A frozen column is not immune"),
# not +-fix_llr itself; fix_llr = 500 puts every frozen column above every other, so the hand-over can be checked column for column.
DECIM = dict(alpha=0.9, t_round=10, max_rounds=3, per_round=8, fix_llr=500.0)
CLIP = 20.0                                                                # the plans' clip_llr (the default)
P_HGP = TC.P_HIGH["hgp"]
# case -> shape, sampling rate, max_iter.  Every path's switch takes hgp.  P_HIGH itself leaves BP no converged trial and P_HIGH / 2 next to none, so
# the rate is P_HIGH / 4 everywhere but under erasures, which come on top of P_LOW.  Observed, sector Z / sector X of 300 trials: BP converged;
# handed over; flags 0 / 1 at (4, 24) -- at (1, 512) every handed-over shot ends with flag 0, and flag 2 never occurs
CASES = {
    "flooding": dict(shape="hgp", p=P_HGP / 4, max_iter=50),              # 83 / 70; 217 / 230; 203, 14 / 186, 44
    "layered": dict(shape="hgp", p=P_HGP / 4, max_iter=50),               # 79 / 79; 221 / 221; 215, 6 / 201, 20
    "decimation": dict(shape="hgp", p=P_HGP / 4, max_iter=50),            # 49 / 38; 251 / 262; 219, 32 / 205, 57 (max_iter is not read: DECIM)
    "f32": dict(shape="hgp", p=P_HGP / 4, max_iter=50),                   # 83 / 70; 217 / 230; 198, 19 / 185, 45
    "correlated:raise": dict(shape="hgp", p=P_HGP / 4, max_iter=50),      # 48 / 41; 252 / 259; 190, 62 / 187, 72 (sector X: 44 converged at (1, 512))
    "correlated:condition": dict(shape="hgp", p=P_HGP / 4, max_iter=50),  # 37 / 20; 263 / 280; 230, 33 / 199, 81 (sector X: 24 converged at (1, 512))
    "erasure_aware": dict(shape="hgp", p=TC.P_LOW, max_iter=50),          # 37 / 25; 263 / 275; 192, 71 / 164, 111 (AWARE_RATES on top of P_LOW)
    "soft_aware": dict(shape="hgp", p=P_HGP / 4, max_iter=50),            # 22 / 18; 278 / 282; 225, 53 / 206, 76 (at P_LOW the cap stops 1 / 2 shots)
}
# one-sector DEM plans (test_events_gpu.model): max_iter, (bits_per_step, max_rows) without and with capped shots.  tiny_z (37 detectors) converges in
# every trial at that module's max_iter = 12 and hands over 8 of 384 at 4, so it runs at 2, and its clusters stay below 24 rows, so its cap is 4.
# Observed of 384 trials: BP converged; handed over; flags 0 / 1 under the cap
ONE_SECTOR = {
    "tiny_z": dict(max_iter=2, lsd=((1, 512), (2, 4))),                    # 319; 65; 55, 10
    "circ72_z": dict(max_iter=12, lsd=((1, 512), (4, 24))),                # 134; 250; 58, 192
}
ONE_COUNT = 384
FIXED_W = TC.W_ODD["hgp"]                                                  # 30 faults per trial
HIST_COUNT = 300                                                           # not a multiple of 256
HIST_KIND = "cols_2"
_CHAINS = {}


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


def new_plan(L, case, lsd, sampler=None, batch=BATCH):
    """a plan of the case with LSD in its OSD stage (lsd None: the path alone, for its sampler)"""
    cfg = CASES[case]
    ctx = PP.context(L, cfg["shape"])
    p = PP.make_plan(L, ctx, case, batch, p=cfg["p"], max_iter=cfg["max_iter"])
    if lsd is not None:
        p.use_lsd(*lsd)
    PP.switch_path(p, ctx, case, DECIM, AWARE_RATES)
    if sampler is not None:
        sampler(p)
    return ctx, p


def by_chain(L, case, lsd, events=False, sampler=None, count=COUNT):
    """the case through the chain, once: the plan's own sampler, then tests/plan_pairs.py.  events: what the plan does with the same syndromes as
    recorded events -- no heralds and no levels, so the plan's prior for every shot.
    -> namespace(res, synds, truths, outcome, pred, tally)"""
    key = (case, lsd, events, sampler is not None, count)
    if key not in _CHAINS:
        ctx, p = new_plan(L, case, None, sampler)
        synds, truths, shot_priors = PP.sample_for(p, case, SEED, 0, count)
        p.close()
        links = ctx.links[case.split(":")[1]] if PP.path_of(case) == "correlated" else None
        priors = PP.priors_of(ctx, case)
        kw = dict(max_iter=CASES[case]["max_iter"], shot_priors=None if events else shot_priors, decim=DECIM, links=links, lsd=lsd)
        res = PP.chain(L, ctx.graphs, priors, synds, case, "lsd", **kw)
        outcome = PP.outcomes(res, ctx.masks, truths)
        h = PP.SimpleNamespace(ctx=ctx, res=res, synds=synds, truths=truths, outcome=outcome, pred=PP.predictions(res, ctx.masks), kw=kw, priors=priors,
                               tally=PP.expected_tally(L, res, outcome))
        _CHAINS[key] = h
    return _CHAINS[key]


def assert_both_stages_worked(what, res, lsd, capped):
    """the conditions every case asserts, with the counts printed: in each sector BP converged somewhere and handed at least eight shots to LSD; without a
    cap some of them end with flag 0, with the small cap some end with flag 1"""
    conv = [int(c.sum()) for c in res.conv]
    handed = [int((c == 0).sum()) for c in res.conv]
    print(f"{what}, LSD {lsd}: converged {conv}, handed over {handed}, flags 0/1/2 per sector {res.flags[:len(conv)].tolist()}")
    assert min(conv) >= 1 and min(handed) >= 8, (what, conv, handed)
    assert res.flags[:len(conv), 1 if capped else 0].min() > 0, (what, res.flags.tolist())


def weights_of(L, h):
    return [L.quantise_weights(p) for p in h.priors]


# ---------------------------------------------------------------------------------------- a. LSD behind each path
@pytest.mark.parametrize("lsd", LSD_PARAMS)
@pytest.mark.parametrize("case", PP.ALL_CASES)
def test_lsd_behind_each_path(L, case, lsd):
    h = by_chain(L, case, lsd)
    ctx, p = new_plan(L, case, lsd)
    got = p.run_outcomes(SEED, 0, COUNT)
    tally, counts = p.read(clear=True), p.lsd_counts()
    p.close()
    assert_both_stages_worked(case, h.res, lsd, capped=lsd != LSD_PARAMS[0])
    assert np.array_equal(got, h.outcome), (case, np.flatnonzero(got != h.outcome)[:8].tolist())
    PP.assert_tally(L, tally, h.tally)
    assert np.array_equal(counts, h.res.flags), (counts.tolist(), h.res.flags.tolist())
    if case == "decimation":                                               # the hand-over holds the frozen columns: s_j +- fix_llr, far above every other key
        for s, g in enumerate(ctx.graphs):
            bad = h.res.conv[s] == 0
            reach = np.bincount(g.indices, minlength=g.n).max() * DECIM["alpha"] * CLIP       # |s_j| <= (column degree) * alpha * clip_llr
            assert np.abs(h.priors[s]).max() + reach < DECIM["fix_llr"] - reach
            frozen = (np.abs(h.res.llr[s][bad]) >= DECIM["fix_llr"] - reach).sum(axis=1)
            infinite = np.isinf(h.res.llr[s][bad]).sum(axis=1)             # (hgp has degree-1 checks: there s_j is unbounded, and such columns freeze first)
            print(f"decimation, sector {s}: rounds of the failures {np.bincount(h.res.legs[s][bad]).tolist()}, frozen columns per failure "
                  f"{np.bincount(frozen).nonzero()[0].tolist()}, infinite among them {int(infinite.min())} .. {int(infinite.max())}")
            assert np.array_equal(frozen, h.res.fixed[s][bad]) and (h.res.legs[s][bad] == 1 + DECIM["max_rounds"]).all()
            assert (frozen == DECIM["max_rounds"] * DECIM["per_round"]).all()
        assert h.tally["legs_z"] > COUNT and h.tally["legs_x"] > COUNT


# ---------------------------------------------------------------------------------------- b. the confidence behind each path
@pytest.mark.parametrize("lsd", LSD_PARAMS)
@pytest.mark.parametrize("case", PP.ALL_CASES)
def test_confidence_behind_each_path(L, case, lsd):
    h = by_chain(L, case, lsd)
    ctx, p = new_plan(L, case, lsd)
    T = L.TALLY
    informative = 0
    for kind in PP.KINDS:
        p.use_confidence(kind, EDGES, *weights_of(L, h))                   # (again with new arguments: the histogram starts at zero)
        out, score = p.run_scores(SEED, 0, COUNT)
        want = PP.scores(kind, h.res)
        assert np.array_equal(out, h.outcome), (case, kind)
        assert np.array_equal(score, want), (case, kind, np.flatnonzero(score != want)[:8].tolist())
        hist, tally = p.confidence_hist(), p.read(clear=True)
        assert np.array_equal(hist, SM.histogram(want, h.outcome, EDGES)), (case, kind)
        col = hist.sum(axis=0)
        assert int(col.sum()) == tally[T["trials"]] == COUNT and int(col[1:].sum()) == tally[T["total_err"]]
        assert int(col[1] + col[3]) == tally[T["z_err"]] and int(col[2] + col[3]) == tally[T["x_err"]]
        PP.assert_tally(L, tally, h.tally)
        informative += int(((score != 0) & (score != NONE)).sum())
        silent = int((score == NONE).sum())
        assert ((score != 0) & (score != NONE)).any(), (case, kind)
        if lsd != LSD_PARAMS[0]:
            assert silent > 0, (case, kind)                                # the small cap: some trials carry no statement
    assert np.array_equal(p.lsd_counts(), len(PP.KINDS) * h.res.flags)
    p.close()
    print(f"{case}, LSD {lsd}: scores neither 0 nor 2^64 - 1: {informative} over {len(PP.KINDS)} kinds; 2^64 - 1: {silent}")


# ---------------------------------------------------------------------------------------- c. correlated behind LSD: the dependency itself
@pytest.mark.parametrize("case", ["correlated:raise", "correlated:condition"])
def test_sector_x_reads_the_cluster_solution(L, case):
    lsd = LSD_PARAMS[0]
    h = by_chain(L, case, lsd)
    lk = h.kw["links"]
    src = np.unique(lk.src)
    failed_z = h.res.conv[0] == 0
    by_lsd = failed_z & h.res.det[0][:, src].any(axis=1)                  # sector Z did not converge and LSD's solution sets a link's source
    base = h.priors[1] if lk.base is None else lk.base
    reweighted = (h.res.used_prior[1] != base[None, :]).any(axis=1)
    moved = (h.res.det[0] != h.res.handed[0])[:, src].any(axis=1)          # ... which the BP stage's own decision did not set (or the other way round)
    print(f"{case}: sector Z failed in {int(failed_z.sum())}, LSD's solution on a link's source in {int(by_lsd.sum())}, sector X reweighted in "
          f"{int((by_lsd & reweighted).sum())} of them, LSD changed a source in {int((failed_z & moved).sum())}")
    assert by_lsd.any() and (by_lsd & reweighted).any() and (failed_z & moved).any()
    # the mutant that reads sector Z's correction from before its OSD stage decodes sector X differently, so the plan's equality above excludes it
    stale = PP.chain(L, h.ctx.graphs, h.priors, h.synds, case, "lsd", **dict(h.kw, stale_links=True))
    assert not np.array_equal(stale.used_prior[1], h.res.used_prior[1])
    same = np.array_equal(PP.outcomes(stale, h.ctx.masks, h.truths), h.outcome) and PP.expected_tally(L, stale, h.outcome) == h.tally
    assert not same, "the stale chain gives the same outcomes and tally: the case does not exercise the dependency"


# ---------------------------------------------------------------------------------------- d. the events door
@pytest.mark.parametrize("lsd", LSD_PARAMS)
@pytest.mark.parametrize("case", PP.ALL_CASES)
def test_events_door(L, case, lsd):
    sampled = by_chain(L, case, lsd)
    h = by_chain(L, case, lsd, events=True)                                # the same syndromes; the plan's prior for every shot
    assert all(np.array_equal(a, b) for a, b in zip(h.synds, sampled.synds))
    records = L.pack_events(np.hstack(h.synds))
    ctx, p = new_plan(L, case, lsd)
    pred0, pred1, flags = p.decode_events(records, SEED, 0)
    assert np.array_equal(pred0, h.pred[0]) and np.array_equal(pred1, h.pred[1]), case
    assert np.array_equal(flags & 1, h.res.conv[0]) and np.array_equal((flags >> 1) & 1, h.res.conv[1]), case
    assert not (flags & 0xC).any()                                         # every correction reproduces its syndrome
    assert np.array_equal(p.lsd_counts(clear=True), h.res.flags)
    for kind in PP.KINDS:
        p.use_confidence(kind, EDGES, *weights_of(L, h))
        q0, q1, qf, score = p.decode_events(records, SEED, 0, scores=True)
        assert np.array_equal(q0, pred0) and np.array_equal(q1, pred1) and np.array_equal(qf, flags), (case, kind)
        assert np.array_equal(score, PP.scores(kind, h.res)), (case, kind)
        assert not p.confidence_hist().any() and not p.read().any()        # recorded events have no outcome: histogram and tally are left alone
    p.close()
    assert_both_stages_worked(case + ", events", h.res, lsd, capped=lsd != LSD_PARAMS[0])


# ---------------------------------------------------------------------------------------- e. one sector
@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("name", sorted(ONE_SECTOR))
def test_one_sector_plan(L, name, which):
    from qldpc_amd.simulation.dem import DemDecoder, DetectorErrorModel
    from test_events_gpu import model
    dem, graphs = model(L, DetectorErrorModel, name)
    cfg = ONE_SECTOR[name]
    lsd, max_iter = cfg["lsd"][which], cfg["max_iter"]
    view = dem.decoder_view(0)
    assert dem.n_sectors == 1
    p = dem.plan(graphs, max_iter=max_iter, batch=BATCH)
    spz, tz, spx, tx = p.sample(SEED, 0, ONE_COUNT)
    res = PP.chain(L, graphs, [view.prior], [spz], "flooding", "lsd", max_iter=max_iter, lsd=lsd)
    outcome, pred = PP.outcomes(res, [view.logmask], [tz]), PP.predictions(res, [view.logmask])[0]
    assert_both_stages_worked(name, res, lsd, capped=which == 1)
    p.use_lsd(*lsd)
    wz = L.quantise_weights(view.prior)
    records = L.pack_events(spz)
    for kind in PP.KINDS:
        p.use_confidence(kind, EDGES, wz, None)
        want = SM.scores(kind, res.stats[0], np.zeros_like(res.stats[0]))
        assert np.array_equal(want, PP.scores(kind, res))
        out, score = p.run_scores(SEED, 0, ONE_COUNT)
        assert np.array_equal(out, outcome) and np.array_equal(score, want), (name, kind, np.flatnonzero(score != want)[:8].tolist())
        assert np.array_equal(p.confidence_hist(), SM.histogram(want, outcome, EDGES)), (name, kind)
        PP.assert_tally(L, p.read(clear=True), PP.expected_tally(L, res, outcome))
        counts = p.lsd_counts(clear=True)
        assert np.array_equal(counts, res.flags) and not counts[1].any()
        q0, q1, qf, qs = p.decode_events(records, SEED, 0, scores=True)
        assert np.array_equal(q0, pred) and not q1.any() and np.array_equal(qf & 1, res.conv[0]) and not (qf & 0x2E).any() and np.array_equal(qs, want), (name, kind)
        p.lsd_counts(clear=True)
        assert ((want != 0) & (want != NONE)).any() and (which == 0 or (want == NONE).any())
        # the shipped surface: the records in the model's detector numbering
        events = np.zeros((ONE_COUNT, dem.n_detectors), np.uint8)
        events[:, dem.detector_map[0]] = spz
        dec = DemDecoder(dem, maxIter=max_iter, decoder="bp_lsd", lsd={"bits_per_step": lsd[0], "max_rows": lsd[1]}, batch=BATCH, confidence=kind)
        bits, conf = dec.decode_batch(events, bit_packed=False, return_confidence=True)
        dec.close()
        assert np.array_equal(bits, ((pred[:, None] >> np.arange(dem.k[0], dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)) and np.array_equal(conf, want)
    p.close()


# ---------------------------------------------------------------------------------------- f. histogram sizes
def test_histogram_sizes(L):
    lsd = LSD_PARAMS[0]
    h = by_chain(L, "flooding", lsd)
    assert HIST_COUNT % 256 and HIST_COUNT == COUNT
    ctx, p = new_plan(L, "flooding", lsd)
    want = PP.scores(HIST_KIND, h.res)
    for edges in (np.arange(1, L.CONF_MAX_BINS, dtype=np.uint64), np.array([int(np.median(want[want != NONE])) + 1], np.uint64), None):
        p.use_confidence(HIST_KIND, edges, *weights_of(L, h))
        out, score = p.run_scores(SEED, 0, HIST_COUNT)
        hist = p.confidence_hist()
        e = np.zeros(0, np.uint64) if edges is None else edges
        assert hist.shape == (e.size + 1, 4) and np.array_equal(score, want)
        assert np.array_equal(hist, SM.histogram(want, h.outcome, e)), e.size + 1
        assert int(hist.sum()) == HIST_COUNT
        if e.size + 1 == L.CONF_MAX_BINS:
            high = int((hist[65:].sum(axis=1) > 0).sum())
            print(f"4096 bins of {HIST_KIND}: {int((hist.sum(axis=1) > 0).sum())} non-empty, {high} of them above bin 64")
            assert high > 1
        if e.size == 1:
            assert hist[0].sum() > 0 and hist[1].sum() > 0
    p.close()


# ---------------------------------------------------------------------------------------- g. a fixed-weight sampler in front of LSD
def test_fixed_weight_in_front_of_lsd(L):
    lsd = LSD_PARAMS[0]
    fixed = lambda p: p.use_fixed_weight(FIXED_W)                          # noqa: E731
    h = by_chain(L, "flooding", lsd, sampler=fixed)
    assert not all(np.array_equal(a, b) for a, b in zip(h.synds, by_chain(L, "flooding", lsd).synds))      # another sampler drew these
    ctx, p = new_plan(L, "flooding", lsd, sampler=fixed)
    got = p.run_outcomes(SEED, 0, COUNT)
    tally, counts = p.read(clear=True), p.lsd_counts()
    p.close()
    assert_both_stages_worked(f"flooding, {FIXED_W} faults per trial", h.res, lsd, capped=False)
    assert np.array_equal(got, h.outcome) and np.array_equal(counts, h.res.flags)
    PP.assert_tally(L, tally, h.tally)


def test_weight_strata_with_lsd(L):
    from qldpc_amd.data import load_code, load_precomputed_matrices
    from qldpc_amd.simulation.strata import run_weight_strata
    c, M = load_code("bb72"), load_precomputed_matrices("circ72")
    weights, par = [7, 15], {"bits_per_step": 2, "max_rows": 256}
    ws = run_weight_strata(c["Hx"], c["Hz"], c["Lx"], c["Lz"], 0.005, weights=weights, trials_per_weight=256, num_cycles=M["num_cycles"], precomputed_matrices=M,
                           base_seed=3, batch=128, decoder="bp_lsd", lsd=par, **_bb_params(c))
    p = circuit_setup(L, "circ72")[6](batch=128)
    p.use_lsd(**par)
    T = L.TALLY
    for i, w in enumerate(weights):                                        # weight w runs the trials from w << 40
        p.use_fixed_weight(w)
        p.run(3, w << 40, 256)
        t = p.read(clear=True)
        assert (ws.trials[i], ws.failures[i], ws.failures_z[i], ws.failures_x[i]) == (256, t[T["total_err"]], t[T["z_err"]], t[T["x_err"]])
        assert ws.bp_converged[i].tolist() == [t[T["bp_conv_z"]], t[T["bp_conv_x"]]]
    assert p.lsd_counts().sum() == 2 * 2 * 256 - ws.bp_converged.sum() > 0
    p.close()


# ---------------------------------------------------------------------------------------- h. the Python surface, once per path family
@pytest.mark.parametrize("family", ["correlated", "erasure", "soft", "layered"])
def test_run_simulation_with_lsd_and_post_selection(L, family):
    from qldpc_amd.data import load_code, load_precomputed_matrices
    from qldpc_amd.simulation.engine import run_simulation
    from qldpc_amd.simulation.postselect import default_edges
    ctx = PP.context(L, "circ72")
    c = load_code("bb72")
    trials, seed, kind, par = 384, 2031, "llr_2", {"bits_per_step": 2, "max_rows": 256}
    more, case = {"correlated": (dict(correlated={"alpha": 1.0, "mode": "raise"}), "correlated:raise"),
                  "erasure": (dict(erasure={"rates": {"CNOT": 0.02}, "aware": True, "alpha": 1.0}), "erasure_aware"),
                  "soft": (dict(soft={"sigma": 0.5, "levels": 8, "aware": True, "alpha": 0.875}), "soft_aware"),
                  "layered": (dict(schedule="layered"), "layered")}[family]
    r = run_simulation(c["Hx"], c["Hz"], c["Lx"], c["Lz"], ctx.p, num_trials=trials, devices=[0], num_cycles=6, precomputed_matrices=load_precomputed_matrices("circ72"),
                       base_seed=seed, batch=128, decoder="bp_lsd", lsd=par, post_select={"kind": kind}, **more, **_bb_params(c))
    p = PP.make_plan(L, ctx, case, 128)
    p.use_lsd(**par)
    PP.switch_path(p, ctx, case, None, {"CNOT": 0.02})
    p.use_confidence(kind, default_edges(kind), *(L.quantise_weights(x) for x in PP.priors_of(ctx, case)))
    p.run(seed, 0, trials)
    tally, counts, hist = p.read(), p.lsd_counts(), p.confidence_hist()
    p.close()
    print(f"{family}: tally {tally.tolist()}, LSD counts {counts.tolist()}")
    assert np.array_equal(r["tally"], tally) and np.array_equal(r["lsd_counts"], counts) and np.array_equal(r["post_selection"].hist, hist)
    assert tally[L.TALLY["trials"]] == trials and counts.sum() > 0 and int(hist.sum()) == trials
