"""Fixed-weight sampling and the stratified LER(p) estimator without a GPU: the numpy model of the sampler's law (tests/fixed_weight_model.py) draws
w-subsets and draws them uniformly; the estimator against a binomial tail computed another way; the weight picker; the argument rules of the Python
layer before any device call; the binding."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fixed_weight_model as FM  # noqa: E402


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def S():
    import qldpc_amd  # noqa: F401
    from qldpc_amd.simulation import strata
    return strata


def pmf_by_recursion(n, p):
    """Binomial(n, p) pmf for w = 0 .. n by B_0 = (1 - p)^n, B_{w+1} = B_w (n - w) / (w + 1) p / (1 - p): no lgamma."""
    out = np.zeros(n + 1)
    out[0] = (1.0 - p) ** n
    for w in range(n):
        out[w + 1] = out[w] * (n - w) / (w + 1) * p / (1.0 - p)
    return out


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N, w", [(6, 3), (37, 36), (37, 37), (4320, 4096), (5, 0)])
def test_model_draws_a_w_subset(N, w):
    for seed, g in ((20260301, 0), ((0x9E3779B9 << 32) | 17, (1 << 32) - 1), (5, 1 << 40)):
        s = FM.floyd_set(N, w, seed, g)
        assert len(s) == w and len(set(s)) == w
        assert all(0 <= x < N for x in s)
    if w == N:
        assert sorted(s) == list(range(N))


def test_model_is_a_function_of_seed_trial_and_weight():
    a = FM.floyd_sets(4320, 30, 7, (1 << 32) - 3, 6)
    assert np.array_equal(a[3:], FM.floyd_sets(4320, 30, 7, 1 << 32, 3))                 # the trial index, not the position in a call
    assert not np.array_equal(a, FM.floyd_sets(4320, 30, 8, (1 << 32) - 3, 6))           # the seed
    assert not np.array_equal(a[:, :29], FM.floyd_sets(4320, 29, 7, (1 << 32) - 3, 6))   # the weight (j = N - w + i moves with it)


CHI2_19_1E6 = 63.677           # the 1 - 1e-6 quantile of chi-square with 19 degrees of freedom (scipy.stats.chi2.ppf(1 - 1e-6, 19) = 63.67705...)


def test_model_subsets_are_uniform():
    """(N, w) = (6, 3): 20 subsets, 20 000 trials at a fixed seed, expected 1000 each.  Pearson's statistic against the 1 - 1e-6 quantile of
    chi-square(19); the seed below was checked to pass (the statistic is printed)."""
    trials, seed = 20000, 20260301
    sets = np.sort(FM.floyd_sets(6, 3, seed, 0, trials), axis=1)
    code = sets[:, 0] * 36 + sets[:, 1] * 6 + sets[:, 2]
    vals, counts = np.unique(code, return_counts=True)
    assert vals.size == 20                                      # C(6, 3): every subset occurs
    stat = float(((counts - trials / 20.0) ** 2 / (trials / 20.0)).sum())
    print(f"chi-square statistic {stat:.3f} (19 degrees of freedom, critical {CHI2_19_1E6})")
    assert stat < CHI2_19_1E6
    # every element is in a subset with probability w / N = 1 / 2
    member = np.array([(sets == x).any(axis=1).mean() for x in range(6)])
    assert np.abs(member - 0.5).max() < 5 * math.sqrt(0.25 / trials)


# ---- the estimator -----------------------------------------------------------------------------------------------------------------------------------
def synthetic(S, n, weights, t, trials=1000):
    """f_w = [w >= t] exactly: k_w = n_w above the threshold, 0 below (all of it in sector Z)"""
    weights = np.asarray(weights, np.int64)
    k = np.where(weights >= t, trials, 0)
    return S.WeightStrata(n, weights, np.full(weights.size, trials), k, k, np.zeros_like(k), np.zeros((weights.size, 2), np.int64))


@pytest.mark.parametrize("n, t, ps", [(60, 7, (0.01, 0.05, 0.2)), (4320, 30, (0.001, 0.005, 0.01)), (17280, 40, (0.001, 0.003))])
def test_estimate_is_the_binomial_tail(S, n, t, ps):
    ws = synthetic(S, n, np.arange(min(n, 600) + 1), t)         # full coverage: the mass above 600 faults is below 1e-300 at these (n, p)
    r = ws.logical_error_rate(np.array(ps))
    for i, p in enumerate(ps):
        tail = pmf_by_recursion(n, p)[t:].sum()
        assert abs(r["estimate"][i] - tail) <= 1e-12 * tail, (p, r["estimate"][i], tail)
        assert abs(r["covered"][i] - 1.0) < 1e-12 and abs(r["upper"][i] - r["lower"][i]) < 1e-12
        assert r["estimate_z"][i] == r["estimate"][i] and r["estimate_x"][i] == 0.0
        assert r["lower"][i] == r["estimate"][i]
    scalar = ws.logical_error_rate(ps[0])
    assert np.shape(scalar["estimate"]) == () and scalar["estimate"] == r["estimate"][0]


def test_a_short_range_widens_the_bounds_by_what_it_leaves_out(S):
    n, p = 4320, 0.005
    ws = synthetic(S, n, np.arange(15, 27), 25)                 # mean 21.6, deviation 4.6: both tails are cut
    r = ws.logical_error_rate(p)
    pmf = pmf_by_recursion(n, p)
    assert abs(r["covered"] - pmf[15:27].sum()) < 1e-12
    assert abs((r["upper"] - r["lower"]) - (1.0 - r["covered"])) <= np.spacing(r["upper"])      # upper = lower + (1 - covered), one rounding
    assert 0.05 < 1.0 - r["covered"] < 0.95
    assert abs(r["estimate"] - pmf[25:27].sum()) <= 1e-12 * r["estimate"]
    # a stratum that was not run counts as not sampled
    ws.trials[ws.weights == 20] = 0
    ws.failures[ws.weights == 20] = 0
    assert abs(ws.logical_error_rate(p)["covered"] - (pmf[15:27].sum() - pmf[20])) < 1e-12


def test_std_error_of_an_empty_handed_stratum_is_not_zero(S):
    n, p = 60, 0.05
    ws = S.WeightStrata(n, [2, 3], [100, 400], [0, 100], [0, 100], [0, 0], np.zeros((2, 2)))
    r = ws.logical_error_rate(p)
    B = pmf_by_recursion(n, p)
    q0, q1 = 1 / 102, 101 / 402
    want = math.sqrt(B[2] ** 2 * q0 * (1 - q0) / 100 + B[3] ** 2 * q1 * (1 - q1) / 400)
    assert abs(r["std_error"] - want) < 1e-15 and r["std_error"] > 0
    assert abs(r["estimate"] - B[3] * 0.25) < 1e-15


def test_save_and_load(S, tmp_path):
    ws = S.WeightStrata(4320, [3, 4, 9], [10, 20, 30], [1, 2, 3], [1, 1, 1], [0, 1, 2], [[9, 8], [19, 18], [29, 28]])
    path = str(tmp_path / "strata.npz")
    ws.save(path)
    back = S.WeightStrata.load(path)
    assert back.n_locs == 4320
    for k in S.WeightStrata.FIELDS:
        assert np.array_equal(getattr(back, k), getattr(ws, k)) and getattr(back, k).dtype == np.int64
    with pytest.raises(ValueError):
        S.WeightStrata(10, [3, 3], [1, 1], [0, 0], [0, 0], [0, 0], np.zeros((2, 2)))
    with pytest.raises(ValueError):
        S.WeightStrata(10, [11], [1], [0], [0], [0], np.zeros((1, 2)))


def test_the_picker_leaves_at_most_coverage_uncovered(S):
    n, p, cov = 4320, 0.005, 1e-9
    lo, hi = S.weights_for(n, (p, p), cov)
    pmf = pmf_by_recursion(n, p)
    assert 0 <= lo <= hi <= 56                                  # the mass outside [0, 56] is 1.7e-10
    assert 1.6e-10 < pmf[57:].sum() < 1.7e-10
    assert pmf[:lo].sum() <= cov and pmf[hi + 1:].sum() <= cov
    assert pmf[:lo + 1].sum() > cov and pmf[hi:].sum() > cov    # and it is the tightest such range
    # a range of p: the low end from p_lo, the high end from p_hi; in between both tails lie further out
    lo2, hi2 = S.weights_for(n, (0.002, 0.005), cov)
    assert hi2 == hi and lo2 <= lo
    assert pmf_by_recursion(n, 0.002)[:lo2].sum() <= cov
    for q in (0.002, 0.003, 0.005):
        f = pmf_by_recursion(n, q)
        assert f[:lo2].sum() <= cov and f[hi2 + 1:].sum() <= cov
    ws = synthetic(S, n, np.arange(lo, hi + 1), 1000)
    assert 1.0 - ws.logical_error_rate(p)["covered"] <= 2 * cov
    for bad in ((0.0, 0.1), (0.2, 0.1), (0.1, 1.0)):
        with pytest.raises(ValueError):
            S.weights_for(n, bad)
    with pytest.raises(ValueError):
        S.weights_for(n, (0.001, 0.002), coverage=0.7)


def test_the_picker_walks_the_pmf_one_step_per_weight(S, monkeypatch):
    """The pmf recursion behind the picker equals the closed form, and the picker costs what it walks: it forms no binomial coefficient (each is a
    sum of min(w, N - w) logarithms, which made picking a range quadratic in N), takes O(hi) steps at the largest N the sampler accepts, and gives the
    range of the definition."""
    for n, p in ((60, 0.05), (4320, 0.005), (17280, 0.003), (17280, 0.4)):
        walk = list(S._log_pmf_walk(n, p))
        assert len(walk) == n + 1
        for w in sorted({0, 1, int(n * p), int(2 * n * p), n // 2, n - 1, n}):
            want = S.log_binomial_pmf(n, w, p)
            assert abs(walk[w] - want) <= 1e-12 * max(1.0, abs(want)), (n, p, w, walk[w], want)
    for n, pr, cov in ((60, (0.05, 0.2), 1e-6), (4320, (0.001, 0.003), 1e-9), (17280, (0.001, 0.003), 1e-9), (300, (0.3, 0.9), 1e-3), (7, (0.5, 0.5), 0.4)):
        lo, hi = S.weights_for(n, pr, cov)
        below, above = pmf_by_recursion(n, pr[0]), pmf_by_recursion(n, pr[1])
        assert below[:lo].sum() <= cov < below[:lo + 1].sum() and above[hi + 1:].sum() <= cov < above[hi:].sum(), (n, pr, cov, lo, hi)
    assert S.weights_for(17280, (0.001, 0.003)) == (0, 100)     # the circ144 sweep of DESIGN 4.13
    steps = []

    def counted(n, p, walk=S._log_pmf_walk):
        for x in walk(n, p):
            steps.append(1)
            yield x

    def no_coefficient(n, w):
        raise AssertionError("the picker formed a binomial coefficient")
    monkeypatch.setattr(S, "_log_pmf_walk", counted)
    monkeypatch.setattr(S, "log_binomial_coefficient", no_coefficient)
    n, cov = 524288, 1e-9                                       # the sampler's limit: mean 524 at p_lo, 1573 at p_hi
    lo, hi = S.weights_for(n, (0.001, 0.003), cov)
    monkeypatch.undo()
    assert 300 < lo < 524 and 1573 < hi < 2000 and len(steps) <= 2 * hi
    below = [math.exp(S.log_binomial_pmf(n, w, 0.001)) for w in range(lo - 150, lo + 1)]      # (beyond these windows the terms are below 1e-30)
    above = [math.exp(S.log_binomial_pmf(n, w, 0.003)) for w in range(hi, hi + 300)]
    assert math.fsum(below[:-1]) <= cov < math.fsum(below) and math.fsum(above[1:]) <= cov < math.fsum(above)


# ---- the argument rules, before any device call -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [-2, 1.5, "3", True, 2.0])
def test_use_fixed_weight_checks_its_argument_first(L, bad, monkeypatch):
    def no_lib():
        raise AssertionError("the library was called before the argument was checked")
    monkeypatch.setattr(L, "lib", no_lib)
    plan = L.CircuitPlan.__new__(L.CircuitPlan)                 # no handle: the check comes first
    plan._h = None
    with pytest.raises(ValueError):
        plan.use_fixed_weight(bad)
    dplan = L.DemPlan.__new__(L.DemPlan)                        # inherited
    dplan._h = None
    with pytest.raises(ValueError):
        dplan.use_fixed_weight(bad)
    assert L.check_fixed_weight(None) == -1 and L.check_fixed_weight(-1) == -1 and L.check_fixed_weight(np.int32(7)) == 7


@pytest.mark.parametrize("kw", [dict(), dict(weights=[3, -2]), dict(weights=[3, 4097]), dict(weights=[1.5]), dict(weights=[3, 3]), dict(weights=[]),
                                dict(weights=[3], p_range=(0.001, 0.002)), dict(p_range=(0.002, 0.001)), dict(p_range=(0.001, 0.002), coverage=0.0),
                                dict(weights=[3], trials_per_weight=0), dict(weights=[3], target_failures=0), dict(weights=[3], max_trials_per_weight=100),
                                dict(weights=[3], batch=0),
                                dict(weights=[3], osd_order=65, decoder="bp_osd_cs"), dict(weights=[3], osd_order=2), dict(weights=[3], relay_params=dict(t0=3)),
                                dict(weights=[3], window=(3, 1), precision="f32"), dict(weights=[3], decoder="nope"), dict(weights=[3], osd_order=-1)])
def test_run_weight_strata_rejects_bad_arguments(L, S, kw, monkeypatch):
    from qldpc_amd.simulation import engine

    def no_gpu(*a, **k):
        raise AssertionError("GPU work started before the arguments were checked")
    monkeypatch.setattr(engine, "BBCodeCircuit", no_gpu)
    monkeypatch.setattr(L, "Graph", no_gpu)
    monkeypatch.setattr(L, "lib", no_gpu)
    with pytest.raises(ValueError):
        S.run_weight_strata(None, None, None, None, 0.005, **kw)


@pytest.mark.parametrize("kw", [dict(), dict(weights=[38]), dict(weights=[-3]), dict(weights=[2], osd_order=2), dict(weights=[2], alpha_mode="alvarado"),
                                dict(weights=[2], window=(3, 1)), dict(weights=[2], uniform=False)])
def test_run_dem_weight_strata_rejects_bad_arguments(L, S, kw, monkeypatch):
    from qldpc_amd.simulation.dem import DetectorErrorModel

    def no_gpu(*a, **k):
        raise AssertionError("GPU work started before the arguments were checked")
    kw = dict(kw)
    dem = FM.uniform_tiny_dem(DetectorErrorModel)
    if not kw.pop("uniform", True):
        prob = dem.prob.copy()
        prob[11] = 0.2
        dem = DetectorErrorModel(prob, [tuple(s) for s in dem.sectors])
    monkeypatch.setattr(L, "Graph", no_gpu)
    monkeypatch.setattr(L, "lib", no_gpu)
    with pytest.raises(ValueError):
        S.run_dem_weight_strata(dem, **kw)
    with pytest.raises(ValueError):
        S.run_dem_weight_strata("circ72", weights=[2])


def test_nonuniform_dem_names_the_mechanism(L, S, monkeypatch):
    from qldpc_amd.simulation.dem import DetectorErrorModel
    dem = FM.uniform_tiny_dem(DetectorErrorModel)
    prob = dem.prob.copy()
    prob[11] = 0.2
    with pytest.raises(ValueError, match="mechanism 11"):
        S.run_dem_weight_strata(DetectorErrorModel(prob, [tuple(s) for s in dem.sectors]), weights=[2])


# ---- the binding ---------------------------------------------------------------------------------------------------------------------------------------
def test_binding_follows_the_header(L):
    import ctypes as C
    assert "qldpc_circuit_plan_use_fixed_weight" in L.exports()
    getattr(L.lib(), "qldpc_circuit_plan_use_fixed_weight")
    assert L.signatures()["qldpc_circuit_plan_use_fixed_weight"] == (C.c_int, [C.c_void_p, C.c_int])
    assert L.lib().qldpc_version() == 101
    assert L.lib().qldpc_circuit_plan_use_fixed_weight(None, 3) == -1
    assert L.lib().qldpc_circuit_plan_use_fixed_weight(None, -1) == -1
    hdr = open(L.HEADER_PATH).read()
    assert f"#define QLDPC_FIXED_WEIGHT_MAX {L.FIXED_WEIGHT_MAX}\n" in hdr and f"#define QLDPC_FIXED_WEIGHT_MAX_LOCS {L.FIXED_WEIGHT_MAX_LOCS}\n" in hdr
    assert (L.FIXED_WEIGHT_MAX, L.FIXED_WEIGHT_MAX_LOCS) == (4096, 524288)
    assert L.DemPlan.use_fixed_weight is L.CircuitPlan.use_fixed_weight
