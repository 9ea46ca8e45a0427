"""CPU side of the regular kernel's domain sweep (tests/regular_shapes.py): the graphs are exactly regular and reach the team sizes they are named for,
every prior class is clean and has the property it is named for, the C oracle both converges and fails on every decode case the GPU module runs, and
the numpy model of the compare-free check update (tests/loo_messages_model.py) equals the oracle word for word on them -- priors with unique minima,
zero magnitudes (-0.0 messages), subnormals and sums that overflow included.  The oracle alone meets these conditions: nothing is skipped or filtered.

What the oracle does on the `huge` class, settled here with its literal arithmetic: the messages of iteration 0 read unclipped priors, so a column
whose checks carry 1.5e308 on every other edge receives three messages of 0.5 * 1.5e308 and its posterior is +-inf -- the "all operands finite" of the
header of csrc/minsum_regular.hip does not hold there.  Its conclusion does: every message stays finite (alpha * min <= 0.5 * 1.5e308 at iteration 0,
<= alpha * clip afterwards, for alpha <= 1), so V - R is never inf - inf, no NaN
arises, |inf| goes through the min chains like any magnitude and the clip brings it back to `clip`."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_minima_model as CM  # noqa: E402
import graph_shapes as GS  # noqa: E402
import loo_messages_model as LM  # noqa: E402
import regular_shapes as RS  # noqa: E402

CASES = RS.decode_cases()
T = {"trials": 0, "z_err": 1, "bp_conv_z": 4, "osd_z": 6, "iters_z": 8, "zero_synd_z": 10, "unsat_z": 12}      # slots of the tally (include/qldpc_hip.h)


def decode(oracle, g, synd, prior, c):
    return oracle.minsum_decode_batch(g.indptr, g.indices, g.n, synd, prior, max_iter=c.max_iter, alpha=c.alpha, alpha_mode=c.alpha_mode,
                                      damping=c.damping, clip_llr=c.clip, threads=0)


def model_equals(g, synd, prior, max_iter, clip, want, ctx):
    with np.errstate(over="ignore"):
        got = LM.LooModel(g.indptr, g.indices, g.n).decode(synd, prior, max_iter, clip)
    assert np.array_equal(got["hard"], want[0]), ctx
    assert np.array_equal(got["conv"], want[1]), ctx
    assert np.array_equal(got["iters"], want[3]), ctx
    assert np.array_equal(CM.words(got["llr"]), CM.words(want[2])), ctx


def test_graphs_reach_the_teams_they_are_named_for():
    G = {name: RS.graph(name) for name in RS.TABLE}
    for name, g in G.items():
        rd, cd = GS.degrees(g.indptr, g.indices, g.n)
        assert GS.regular_takes(rd, cd) and (rd.max(), cd.max()) == (g.cdeg, g.vdeg), name
        assert g.indptr.dtype == np.int32 and g.indices.dtype == np.int32 and (np.diff(g.cols, axis=1) > 0).all(), name
        pr = np.full(g.n, 3.0)
        assert GS.rule_path(g.indptr, g.indices, g.n, pr) == g.expected, name
        assert GS.rule_path(g.indptr, g.indices, g.n, pr, max_iter=1025) == "RESIDENT", name
        assert (g.S is not None) == (g.expected == "REGULAR"), name
    assert (G["r63_m36"].TS, G["r63_m36"].S) == (36, 14)
    assert (G["r63_m256"].S, G["r63_m256"].block) == (2, 2 * G["r63_m256"].TS)
    assert (G["r63_m257"].S, G["r63_m257"].block, G["r63_m257"].block - G["r63_m257"].TS) == (1, 320, 63)
    for name in ("r63_m512", "r42_m512", "r84_m512"):
        assert (G[name].TS, G[name].S, G[name].block) == (RS.LB_T, 1, 512), name
    assert G["r84_m512"].lds > 39 * 1024 >= G["r63_m512"].lds                                # S = 1 and still above the target of the loop
    assert G["r63_m513"].m == 513 and max(G["r63_m513"].m, (G["r63_m513"].n + 1) // 2) == RS.LB_T + 1
    g = G["r84_m24"]
    assert 1 < g.S < RS.LB_T // g.TS and g.lds <= 39 * 1024 and g.block % 64 == 0 and g.S * g.TS % 64 != 0    # cut back by the LDS loop; ends in the middle of a wave
    assert RS.plan(6, 36, 72, max_iter=1024) is not None and RS.plan(6, 36, 72, max_iter=1025) is None
    # the first-iteration pipeline's own bound
    assert (G["r63_m320"].m + G["r63_m320"].n) * 64 == RS.FIRST_ITERATION_BYTES and (G["r63_m321"].m + G["r63_m321"].n) * 64 > RS.FIRST_ITERATION_BYTES
    for name in RS.TEAM_GRAPHS + RS.MC_GRAPHS:
        assert name in G


@pytest.mark.parametrize("name", RS.PRIOR_GRAPHS + ("r63_m512",))
def test_prior_classes_are_clean_and_have_the_property_they_are_named_for(name):
    g = RS.graph(name)
    P = RS.priors(g)
    assert tuple(P) == RS.PRIOR_CLASSES
    for k, pr in P.items():
        assert pr.shape == (g.n,) and pr.dtype == np.float64 and GS.prior_is_clean(pr), k
        assert np.array_equal(CM.words(pr), CM.words(RS.priors(g)[k])), k                   # deterministic
    assert len(np.unique(P["uniform"])) == 1 and P["uniform"][0] > 0
    assert len(np.unique(np.abs(P["normal"]))) == g.n                                       # no two |prior| equal: no tie at iteration 0
    assert (P["negative class"] == -1.5).sum() == g.n // 9 and set(np.unique(P["negative class"])) == {-1.5, 4.0}
    z = P["zero class"]
    assert (z == 0).sum() == g.n // 9 and not np.signbit(z).any() and set(np.unique(z)) == {0.0, 4.0}
    assert (P["above clip"] == 27.0).sum() == g.n // 7 and 27.0 > max(RS.CLIPS)
    assert not P["all zero"].any() and not np.signbit(P["all zero"]).any()
    s = P["subnormal"]
    assert (s == 5e-324).sum() == 3 and (s == 1e-310).sum() == 3 and (s[s > 1e-300] == 3.0).all() and 0 < 1e-310 < np.finfo(np.float64).tiny
    h = P["huge"]
    j = RS.overflow_column(g)
    rows = np.flatnonzero((g.cols == j).any(axis=1))
    assert len(rows) == g.vdeg and h[j] == 4.0 and all((h[np.setdiff1d(g.cols[i], [j])] == 1.5e308).all() for i in rows)
    assert 0 < (h == 1.5e308).sum() <= g.vdeg * (g.cdeg - 1) and (0.5 * 1.5e308) * 3 == float("inf")


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_decode_case_has_both_outcomes_and_the_model_equals_the_oracle(oracle, case):
    g = RS.graph(case.graph)
    prior = RS.priors(g)[case.prior]
    synd = RS.syndromes(g, case.B, prior, case.salt)
    assert synd.shape == (case.B, g.m) and not synd[-1].any()
    err, conv, llr, iters = want = decode(oracle, g, synd, prior, case)
    print(f"{case.id}: {int(conv.sum())} of {case.B} shots converge, iterations up to {int(iters.max()) + 1}, {int((llr == 0).sum())} zero posteriors, "
          f"{int(np.isinf(llr).sum())} infinite ones")
    assert 0 < int(conv.sum()) < case.B, "the syndromes should hold converging and failing shots"
    assert not np.isnan(llr).any() and not (np.signbit(llr) & (llr == 0)).any()             # the header's claim: a posterior is never -0.0
    if case.prior in ("zero class", "all zero"):
        assert (llr == 0).any()
    if case.prior == "huge":
        assert np.isinf(llr[:, RS.overflow_column(g)]).any() and np.isfinite(np.delete(llr, RS.overflow_column(g), axis=1)).all()
    if case.modelled:
        model_equals(g, synd, prior, case.max_iter, case.clip, want, case.id)


def test_iteration_cap_shots_never_converge(oracle):
    g = RS.graph("r63_m36")
    prior = RS.priors(g)["uniform"]
    synd = RS.never_converging(g, oracle, prior)
    assert synd.shape == (RS.NEVER_CONVERGE, g.m)
    for max_iter in (1024, 1025):
        want = oracle.minsum_decode_batch(g.indptr, g.indices, g.n, synd, prior, max_iter=max_iter, threads=0)
        assert not want[1].any() and (want[3] == max_iter - 1).all()
    want = oracle.minsum_decode_batch(g.indptr, g.indices, g.n, synd, prior, max_iter=1024, threads=0)
    model_equals(g, synd, prior, 1024, 20.0, want, "max_iter 1024")


@pytest.mark.parametrize("name", sorted(RS.SECOND_TRIP))
def test_second_trip_differs_in_outcome_from_the_first(oracle, name):
    """A workgroup's second `base` reuses unsat, active, sres, lacc, Rprev and done: the shots a (workgroup, slot) decodes first and second must differ
    in outcome, both ways, for stale state to show."""
    g, B, trips = RS.second_trip(name)
    pc, clip = RS.SECOND_TRIP[name]
    prior = RS.priors(g)[pc]
    assert B > RS.GRID_CAP * g.S and len(trips) == B - RS.GRID_CAP * g.S and trips[0] == (0, RS.GRID_CAP * g.S)
    assert (g.S == 1) == (name == "r63_m257") and (g.S == 1 or len(trips) % g.S != 0)         # S > 1: the last group of the second trip is ragged
    synd = RS.syndromes(g, B, prior, salt=2)
    want = oracle.minsum_decode_batch(g.indptr, g.indices, g.n, synd, prior, max_iter=RS.MAX_ITER, clip_llr=clip, threads=0)
    conv, iters = np.asarray(want[1]).astype(bool), np.asarray(want[3])
    first, second = np.array(trips).T
    print(f"{name}: B {B}, {int(conv.sum())} converge; of {len(trips)} slots that decode twice {int((conv[first] & ~conv[second]).sum())} converge then fail, "
          f"{int((~conv[first] & conv[second]).sum())} fail then converge, {int((iters[first] != iters[second]).sum())} differ in iterations")
    assert (conv[first] & ~conv[second]).any() and (~conv[first] & conv[second]).any() and (iters[first] != iters[second]).any()
    both = np.concatenate([first, second])
    model_equals(g, synd[both], prior, RS.MAX_ITER, clip, tuple(np.asarray(w)[both] for w in want), name)


@pytest.mark.parametrize("name", RS.MC_GRAPHS)
def test_monte_carlo_inputs_with_nonpositive_priors(oracle, name):
    """p >= 0.5: the uniform prior log((1 - p) / p) is +0.0 at 0.5 and negative beyond; mc_first_table refuses it, so the closed form of iteration 0
    in the full kernel decodes every shot.  The oracle's tallies say what the GPU module then compares."""
    g = RS.graph(name)
    L = RS.logicals(g)
    for p in RS.MC_PS:
        thr = oracle.bernoulli_threshold(p)
        assert 0 < thr < 2 ** 32 and thr == int(np.floor(p * 2.0 ** 32)) and abs(thr / 2.0 ** 32 - p) < 2.0 ** -32
        errs = np.array([oracle.cc_sample_errors(RS.MC_SEED, b, g.n, p) for b in range(200)])
        assert abs(errs.mean() - p) < 0.02, (p, errs.mean())
    p0 = [np.log((1 - p) / p) for p in RS.MC_PS]
    assert p0[0] == 0 and not np.signbit(p0[0]) and -1.0 < p0[1] < 0 and p0[2] < -1.0 and RS.MC_PS == (0.5, 0.7, 0.93) and 1.0 in RS.MC_CLIPS
    for p in RS.MC_PS:
        for clip in RS.MC_CLIPS:
            for use_osd in (True, False):
                t = oracle.cc_sample_decode_tally(g.indptr, g.indices, g.n, L, p, RS.MC_SEED, 0, RS.MC_SHOTS, max_iter=RS.MAX_ITER, clip_llr=clip, use_osd=use_osd,
                                                  threads=0)
                print(f"{name} p {p} clip {clip} osd {use_osd}: {t[T['bp_conv_z']]} of {t[T['trials']]} converge, {t[T['zero_synd_z']]} zero syndromes, "
                      f"{t[T['z_err']]} logical errors, {t[T['osd_z']]} through OSD-0, {t[T['unsat_z']]} left unsatisfied")
                assert t[T["trials"]] == RS.MC_SHOTS and t[T["osd_z"]] == (RS.MC_SHOTS - t[T["bp_conv_z"]] if use_osd else 0)
                if p == 0.5:
                    # a zero prior makes every message +-0.0 and every posterior +0.0: the hard decision is 0 everywhere and BP converges exactly on
                    # the zero syndromes, of which a fair coin gives (almost) none
                    assert t[T["bp_conv_z"]] == t[T["zero_synd_z"]] <= RS.MC_SHOTS // 100 and t[T["iters_z"]] >= RS.MAX_ITER * (RS.MC_SHOTS - t[T["zero_synd_z"]])
                if p == 0.7:
                    assert 0 < t[T["bp_conv_z"]] < RS.MC_SHOTS


def test_monte_carlo_inputs_at_the_first_iteration_bound(oracle):
    for name in ("r63_m320", "r63_m321"):
        g = RS.graph(name)
        t = oracle.cc_sample_decode_tally(g.indptr, g.indices, g.n, RS.logicals(g), RS.MC_BOUND_P, RS.MC_SEED, 0, RS.MC_BOUND_SHOTS, max_iter=RS.MAX_ITER, threads=0)
        # some shots stop at the first iteration and some go on to the full decoder
        assert t[T["trials"]] == RS.MC_BOUND_SHOTS and 0 < t[T["zero_synd_z"]] < RS.MC_BOUND_SHOTS and RS.MC_BOUND_SHOTS < t[T["iters_z"]] < 2 * RS.MC_BOUND_SHOTS
    # second trip: BP fails on shots of a workgroup's first `base` and of its second one, and converges on others of both
    g = RS.graph("r63_m257")
    assert g.S == 1 and RS.MC_TRIP_SHOTS > RS.GRID_CAP
    for begin, count in ((0, RS.GRID_CAP), (RS.GRID_CAP, RS.MC_TRIP_SHOTS - RS.GRID_CAP)):
        t = oracle.cc_sample_decode_tally(g.indptr, g.indices, g.n, RS.logicals(g), RS.MC_TRIP_P, RS.MC_SEED, begin, count, max_iter=RS.MAX_ITER, threads=0)
        print(f"r63_m257 p {RS.MC_TRIP_P} shots {begin} .. {begin + count}: {count - t[T['bp_conv_z']]} BP failures exported")
        assert 0 < t[T["bp_conv_z"]] < count and t[T["osd_z"]] == count - t[T["bp_conv_z"]]
