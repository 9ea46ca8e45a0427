"""Fixed-weight fault sampling on the MI355X: the sampler against the numpy model bit for bit (F1), independence of batching (F2), the two-way switch
(F3), the fused pipeline against its parts under every decode switch (F4), refusals (F5), and the stratified estimator against direct sampling (F6)."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fixed_weight_model as FM  # noqa: E402
import test_dem_gpu as TD  # noqa: E402  (parts, assert_tally, the decode switches: the comparison that file makes)
from test_relay_gpu import _bb_params, circuit_setup  # noqa: E402

pytestmark = pytest.mark.gpu

SEEDS = [20260301, (0x9E3779B9 << 32) | 17]
BEGIN = 2 ** 32 - 32                                  # 64 trials from here cross the 32-bit counter word


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


@pytest.fixture(scope="module")
def DEM():
    from qldpc_amd.simulation.dem import DetectorErrorModel
    return DetectorErrorModel


@pytest.fixture(scope="module")
def circ72(L):
    """the circ72 plan factory of test_relay_gpu (N = 4320 locations) and the model of its sampler, built once"""
    c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, "circ72")
    p = plan(batch=64)
    n_det, k, n_locs = (p.nsx, p.nsz), p.k, p.n_locs
    p.close()
    sigs = [L.circuit_fault_signatures(compiled, c["Lx"], c["Lz"], x) for x in (0, 1)]
    model = FM.CircuitModel(sigs[0], sigs[1], compiled.base_ops, n_det, k)
    assert model.N == n_locs == 4320
    view = SimpleNamespace(n_sectors=2, decoder_view=lambda s: SimpleNamespace(prior=priors[s], logmask=masks[s]))      # what TD.parts reads of a model
    return SimpleNamespace(c=c, M=M, graphs=graphs, priors=priors, masks=masks, plan=plan, model=model, view=view)


_DEMS = {}


def tiny(L, DEM, nsec):
    """(the uniform tiny model with `nsec` sectors, its graphs), built once"""
    if nsec not in _DEMS:
        dem = FM.uniform_tiny_dem(DEM, 0.1, nsec)
        views = [dem.decoder_view(s) for s in range(dem.n_sectors)]
        _DEMS[nsec] = (dem, [L.Graph(v.indptr, v.indices, v.shape[1]) for v in views])
    return _DEMS[nsec]


def assert_same(got, want, what):
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape, (what, i, a.shape, b.shape)
        bad = np.flatnonzero((a != b).reshape(a.shape[0], -1).any(axis=1))
        assert bad.size == 0, f"{what}: output {i}: trials {bad[:8].tolist()} differ ({bad.size} of {a.shape[0]})"


# ---- F1 -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [0, 1, 2, 37, 300, 4096])
def test_f1_circuit_sampler_is_the_model(L, circ72, w):
    plan = circ72.plan(batch=48)                                # two launches (48 + 16 trials), one trial per workgroup
    plan.use_fixed_weight(w)
    for seed in SEEDS:
        got = plan.sample(seed, BEGIN, 64)
        want = circ72.model.sample(w, seed, BEGIN, 64)
        assert_same(got, want, f"w = {w}, seed {seed:#x}")
        if w >= 37:
            assert got[0].any() and got[2].any() and got[1].any() and got[3].any()      # both sectors' syndromes and truths are exercised
        if w == 0:
            assert not any(x.any() for x in got)
    plan.close()


# A launch has at most GRID workgroups, so a batch above GRID gives a workgroup a second and a third trial: the membership bit set (zeroed once, then
# cleared word by word from the list), the sector bit sets and the logical accumulators must come out of one trial empty for the next.  A bit left
# behind would still give a valid w-subset, only another one, so these are pinned bit for bit: every trial against a launch of one trial per
# workgroup (batch = GRID), and against the model -- all of them where the model is quick, else the trials around each round's first and last.
GRID = 4096
STRIDE_COUNT = 3 * GRID + 77                          # a launch of three trials per workgroup, then a ragged one
STRIDE_BEGIN = BEGIN - GRID                           # the second round crosses the 32-bit counter word


def _stride_pair(make_plan, w, seed):
    """(what a plan of batch 3 GRID samples, what a plan of batch GRID samples) over the same STRIDE_COUNT trials"""
    out = []
    for batch in (3 * GRID, GRID):
        plan = make_plan(batch)
        plan.use_fixed_weight(w)
        out.append(plan.sample(seed, STRIDE_BEGIN, STRIDE_COUNT))
        plan.close()
    return out


@pytest.mark.parametrize("w", [30, 4096])
def test_f1_circuit_workgroup_runs_several_trials(L, circ72, w):
    seed = SEEDS[1]
    got, single = _stride_pair(lambda b: circ72.plan(batch=b), w, seed)
    assert_same(got, single, f"w = {w}: three trials per workgroup against one")
    if w == 30:
        assert_same(got, circ72.model.sample(w, seed, STRIDE_BEGIN, STRIDE_COUNT), "w = 30 against the model")
    else:                                                       # (the model walks 4096 steps per trial in Python: 48 trials of the 12 365)
        for lo, n in ((0, 8), (GRID - 8, 16), (2 * GRID - 4, 8), (3 * GRID - 8, 16)):
            part = [a[lo:lo + n] for a in got]
            assert_same(part, circ72.model.sample(w, seed, STRIDE_BEGIN + lo, n), f"w = 4096 against the model, trials from {lo}")
    assert got[0][GRID:].any() and got[2][GRID:].any()


@pytest.mark.parametrize("w", [5, 36])
def test_f1_dem_workgroup_runs_several_trials(L, DEM, w):
    dem, graphs = tiny(L, DEM, 2)
    seed = SEEDS[0]
    got, single = _stride_pair(lambda b: dem.plan(graphs, batch=b), w, seed)
    assert_same(got, single, f"w = {w}: three trials per workgroup against one")
    want = FM.sample_dem(dem, w, seed, STRIDE_BEGIN, STRIDE_COUNT)
    for s in range(2):
        assert_same(got[2 * s:2 * s + 2], want[s], f"sector {s}, w = {w} against the model")
    assert got[0][GRID:].any() and got[2][GRID:].any()


@pytest.mark.parametrize("nsec", [1, 2])
@pytest.mark.parametrize("w", [0, 1, 36, 37])
def test_f1_dem_sampler_is_the_model(L, DEM, nsec, w):
    dem, graphs = tiny(L, DEM, nsec)
    plan = dem.plan(graphs, batch=48)
    plan.use_fixed_weight(w)
    for seed in SEEDS:
        got = plan.sample(seed, BEGIN, 64)
        want = FM.sample_dem(dem, w, seed, BEGIN, 64)
        for s in range(nsec):
            assert_same(got[2 * s:2 * s + 2], want[s], f"sector {s}, w = {w}")
        if nsec == 1:
            assert got[2].size == 0 and not got[3].any()
        if w == 37:                                             # every mechanism fires: one answer for all trials, the XOR of all of them
            every = FM.sample_dem(dem, 37, 0, 0, 1)
            for s in range(nsec):
                assert (got[2 * s] == every[s][0]).all() and (got[2 * s + 1] == every[s][1]).all()
            assert got[0].any()
    plan.close()


def test_f1_largest_location_count_takes_the_large_lds_path(L, DEM):
    """N = 524 288 mechanisms: a 64 KiB membership bit set, beyond the default dynamic-LDS size of a launch; one more mechanism is refused"""
    dem, graphs = tiny(L, DEM, 1)
    v = dem.decoder_view(0)
    for n, ok in ((L.FIXED_WEIGHT_MAX_LOCS, True), (L.FIXED_WEIGHT_MAX_LOCS + 1, False)):
        l = np.arange(n)
        big = DEM(np.full(n, 1e-6), [(37, 64, 0, np.arange(n + 1), l % 37, np.where(l % 3 == 0, np.uint64(1) << (l % 64).astype(np.uint64), np.uint64(0)))], [v])
        plan = big.plan(graphs, batch=8)
        if ok:
            for w in (3, 4096):
                plan.use_fixed_weight(w)
                got = plan.sample(SEEDS[0], BEGIN + 28, 8)
                assert_same(got[:2], FM.sample_dem(big, w, SEEDS[0], BEGIN + 28, 8)[0], f"N = {n}, w = {w}")
                assert got[0].any()
        else:
            before = plan.sample(5, 0, 8)
            assert L.lib().qldpc_circuit_plan_use_fixed_weight(plan._h, 3) == -4            # QLDPC_ERR_UNSUPPORTED
            assert str(L.FIXED_WEIGHT_MAX_LOCS).encode() in L.lib().qldpc_last_error()
            assert_same(plan.sample(5, 0, 8), before, "after the refusal")
        plan.close()


# ---- F2 -----------------------------------------------------------------------------------------------------------------------------------------------
def test_f2_result_does_not_depend_on_batching(L, circ72):
    seed, begin, w = 31337, 2 ** 32 - 150, 30
    plan = circ72.plan(batch=128, max_iter=12)
    plan.use_fixed_weight(w)
    whole = plan.sample(seed, begin, 300)
    pieces = [plan.sample(seed, begin + 100 * i, 100) for i in range(3)]
    assert_same([np.concatenate([p[i] for p in pieces]) for i in range(4)], whole, "three calls of 100")
    out = plan.run_outcomes(seed, begin, 300)
    tally = plan.read(clear=True)
    cut = np.concatenate([plan.run_outcomes(seed, begin + 100 * i, 100) for i in range(3)])
    assert np.array_equal(cut, out) and np.array_equal(plan.read(clear=True), tally)
    plan.close()
    other = circ72.plan(batch=77, max_iter=12)                  # another batch size, another grid
    other.use_fixed_weight(w)
    assert_same(other.sample(seed, begin, 300), whole, "batch 77")
    assert np.array_equal(other.run_outcomes(seed, begin, 300), out) and np.array_equal(other.read(clear=True), tally)
    other.close()
    assert tally[L.TALLY["trials"]] == 300 and whole[0].any()


# ---- F3 -----------------------------------------------------------------------------------------------------------------------------------------------
def test_f3_switch_is_two_way_and_leaks_nothing(L, circ72):
    seed, count, T = 99, 256, L.TALLY
    fresh = circ72.plan(batch=128, max_iter=12)
    want = fresh.sample(seed, 7, count)
    fresh.run(seed, 7, count)
    want_tally = fresh.read(clear=True)
    fresh.close()
    plan = circ72.plan(batch=128, max_iter=12)
    assert plan.fixed_weight is None                            # a fresh plan is on its own sampler
    plan.use_fixed_weight(5)
    assert plan.fixed_weight == 5
    five = plan.sample(seed, 7, count)
    assert not all(np.array_equal(a, b) for a, b in zip(five, want))
    plan.run(seed, 7, count)
    plan.read(clear=True)
    plan.use_fixed_weight(-1)
    assert plan.fixed_weight is None
    assert_same(plan.sample(seed, 7, count), want, "back to the independent draws")
    plan.run(seed, 7, count)
    assert np.array_equal(plan.read(clear=True), want_tally)
    plan.use_fixed_weight(5)                                    # and forth again, any number of times
    assert_same(plan.sample(seed, 7, count), five, "weight 5 again")
    plan.use_fixed_weight(None)
    assert_same(plan.sample(seed, 7, count), want, "None switches back too")
    # weight 0: nothing happens, so nothing fails
    plan.use_fixed_weight(0)
    assert not any(x.any() for x in plan.sample(seed, 7, count))
    out = plan.run_outcomes(seed, 7, count)
    t = plan.read(clear=True)
    assert not out.any() and t[T["total_err"]] == t[T["z_err"]] == t[T["x_err"]] == 0
    assert t[T["trials"]] == t[T["bp_conv_z"]] == t[T["bp_conv_x"]] == t[T["zero_synd_z"]] == t[T["zero_synd_x"]] == count
    assert t[T["osd_z"]] == t[T["osd_x"]] == 0
    plan.close()


# ---- F4 -----------------------------------------------------------------------------------------------------------------------------------------------
def _decoders(L, seed, begin, max_iter):
    sw = TD._switches(L, seed, begin, max_iter)

    def minsum(s, g, v, synd):
        det, conv, llr, it = L.minsum_decode_batch(g, synd, v.prior, max_iter, "dynamical", 1.0)
        return det, conv, llr, it + 1
    return {"plain": (lambda p: None, None), "relay": sw["relay"], "osd_cs": (lambda p: p.use_osd_cs(7), TD._bp_then_osd(L, minsum, cs_order=7)),
            "window": sw["window"]}


@pytest.mark.parametrize("switch, first", [("plain", "sampler")] + [(s, f) for s in ("relay", "osd_cs", "window") for f in ("decoder", "sampler")])
def test_f4_pipeline_is_its_parts(L, circ72, switch, first):
    seed, begin, count, max_iter, w = 777, 1000, 128, 12, 30
    use, decode = _decoders(L, seed, begin, max_iter)[switch]
    plan = circ72.plan(batch=64, max_iter=max_iter)
    if first == "decoder":
        use(plan)
        plan.use_fixed_weight(w)
    else:
        plan.use_fixed_weight(w)
        use(plan)
    verdict, want = TD.parts(L, circ72.view, circ72.graphs, plan, seed, begin, count, max_iter, decode)
    got = plan.run_outcomes(seed, begin, count)
    tally = plan.read(clear=True)
    assert_same(plan.sample(seed, begin, count), circ72.model.sample(w, seed, begin, count), "the sampler under the switch")
    plan.close()
    bad = np.flatnonzero(got != verdict)
    assert bad.size == 0, f"{switch}: verdicts of trials {bad[:8].tolist()} differ ({bad.size} of {count})"
    TD.assert_tally(L, tally, want, slots=set(L.TALLY) - {"legs_z", "legs_x"})
    assert tally[L.TALLY["zero_synd_z"]] < count                # 30 faults leave a syndrome: the decoders had work


# ---- F5 -----------------------------------------------------------------------------------------------------------------------------------------------
def test_f5_refusals_leave_the_plan_as_it_was(L, DEM, circ72):
    err = lambda: (L.lib().qldpc_last_error() or b"").decode()      # noqa: E731
    plan = circ72.plan(batch=64)
    plan.use_fixed_weight(9)
    before = plan.sample(3, 0, 64)
    assert L.lib().qldpc_circuit_plan_use_fixed_weight(plan._h, -2) == -1 and "negative" in err()
    with pytest.raises(ValueError):
        plan.use_fixed_weight(-2)
    assert L.lib().qldpc_circuit_plan_use_fixed_weight(plan._h, 4097) == -1 and "4096" in err()
    with pytest.raises(L.QldpcError, match="4096"):
        plan.use_fixed_weight(4097)
    assert plan.fixed_weight == 9
    assert_same(plan.sample(3, 0, 64), before, "after the refusals")
    plan.close()
    dem, graphs = tiny(L, DEM, 2)
    dplan = dem.plan(graphs, batch=64)
    before = dplan.sample(3, 0, 64)                             # (the independent draws)
    assert L.lib().qldpc_circuit_plan_use_fixed_weight(dplan._h, 38) == -1 and "37" in err()
    with pytest.raises(L.QldpcError, match="37 fault locations"):
        dplan.use_fixed_weight(38)
    assert_same(dplan.sample(3, 0, 64), before, "after w = N + 1")
    dplan.use_fixed_weight(37)                                  # w = N is fine
    dplan.close()
    import dem_model as DM
    mixed = DM.tiny_dem(DEM)                                    # mechanism 0 has p = 0, mechanism 1 has 2^-32
    mgraphs = [L.Graph(v.indptr, v.indices, v.shape[1]) for v in (mixed.decoder_view(0), mixed.decoder_view(1))]
    mplan = mixed.plan(mgraphs, batch=64)
    before = mplan.sample(3, 0, 64)
    assert L.lib().qldpc_circuit_plan_use_fixed_weight(mplan._h, 2) == -1 and "mechanism 1 " in err()
    with pytest.raises(L.QldpcError, match="mechanism 1 "):
        mplan.use_fixed_weight(2)
    assert_same(mplan.sample(3, 0, 64), before, "after the non-uniform refusal")
    assert L.lib().qldpc_circuit_plan_use_fixed_weight(mplan._h, -1) == 0       # switching back is always accepted
    mplan.close()


# ---- F6 -----------------------------------------------------------------------------------------------------------------------------------------------
def test_f6_estimator_reproduces_direct_sampling(L, circ72):
    """circ72, priors and sampler at p = 0.005, BP + OSD-0; strata w = 0 .. 56 of 512 trials against 32 768 trials of the plan's own Bernoulli sampler.
    Seeds are fixed, so the outcome is deterministic; the figures the run produced are in DESIGN 4.13."""
    from qldpc_amd.simulation import strata
    p, T = 0.005, L.TALLY
    plan = circ72.plan(batch=4096)
    stream = L.Stream(0)
    ws = strata._sweep(plan, stream, plan.n_locs, np.arange(57), 512, None, 4096, 20260302)
    assert plan.fixed_weight is None                            # the sweep hands the plan back on its own sampler
    plan.run(20260303, 0, 32768, stream.ptr)
    t = plan.read(stream.ptr, clear=True)
    plan.close()
    stream.close()
    assert t[T["trials"]] == 32768 and (ws.trials == 512).all() and ws.n_locs == 4320
    direct = t[T["total_err"]] / 32768.0
    direct_se = math.sqrt(direct * (1.0 - direct) / 32768.0)
    r = ws.logical_error_rate(p)
    print(f"stratified {float(r['estimate']):.6f} +- {float(r['std_error']):.6f} (uncovered {1.0 - float(r['covered']):.3e}); "
          f"direct {direct:.6f} +- {direct_se:.6f}; failures per weight {ws.failures.tolist()}")
    assert 1.0 - r["covered"] <= 1e-9
    assert abs(r["estimate"] - direct) <= 5.0 * math.sqrt(float(r["std_error"]) ** 2 + direct_se ** 2)
    for key, slot in (("estimate_z", "z_err"), ("estimate_x", "x_err")):
        d = t[T[slot]] / 32768.0
        assert abs(r[key] - d) <= 5.0 * math.sqrt(float(r["std_error" + key[8:]]) ** 2 + d * (1.0 - d) / 32768.0)
    assert ws.failures[0] == 0 and ws.failures[-1] > 0 and (ws.bp_converged[0] == 512).all()


def test_f6_public_entry_points_run_the_same_sweep(L, DEM, circ72):
    from qldpc_amd.simulation import strata
    c, M = circ72.c, circ72.M
    kw = dict(num_cycles=M["num_cycles"], precomputed_matrices=M, base_seed=5, batch=128, maxIter=12, **_bb_params(c))
    ws = strata.run_weight_strata(c["Hx"], c["Hz"], c["Lx"], c["Lz"], 0.005, weights=[0, 30, 45], trials_per_weight=256, **kw)
    plan = circ72.plan(batch=128, max_iter=12)
    for i, w in enumerate((0, 30, 45)):                         # weight w runs the trials from w << 40
        plan.use_fixed_weight(w)
        out = plan.run_outcomes(5, w << 40, 256)
        t = plan.read(clear=True)
        assert (ws.trials[i], ws.failures[i], ws.failures_z[i], ws.failures_x[i]) == (256, np.count_nonzero(out), np.count_nonzero(out & 1), np.count_nonzero(out & 2))
        assert ws.bp_converged[i].tolist() == [t[L.TALLY["bp_conv_z"]], t[L.TALLY["bp_conv_x"]]]
    plan.close()
    assert ws.n_locs == 4320 and ws.weights.tolist() == [0, 30, 45] and ws.failures[2] > 0
    # target_failures: whole batches until the target or the cap, all counted
    stop = strata.run_weight_strata(c["Hx"], c["Hz"], c["Lx"], c["Lz"], 0.005, weights=[0, 45], trials_per_weight=256, target_failures=1,
                                    max_trials_per_weight=512, **kw)
    assert stop.trials[0] == 512 and stop.failures[0] == 0      # never fails: runs to the cap, four batches
    assert stop.trials[1] in (128, 256, 384, 512) and (stop.failures[1] >= 1 or stop.trials[1] == 512)
    # p_range picks the weights; a decode switch rides along
    rel = strata.run_weight_strata(c["Hx"], c["Hz"], c["Lx"], c["Lz"], 0.005, p_range=(0.0049, 0.005), coverage=1e-3, trials_per_weight=64,
                                   decoder="relay_bp", relay_params=TD.RELAY, **kw)
    lo, hi = strata.weights_for(4320, (0.0049, 0.005), 1e-3)
    assert rel.weights.tolist() == list(range(lo, hi + 1)) and (rel.trials == 64).all()
    # a uniform detector error model
    dem, _ = tiny(L, DEM, 2)
    dws = strata.run_dem_weight_strata(dem, weights=range(0, 38), trials_per_weight=128, maxIter=12, base_seed=9, batch=64)
    assert dws.n_locs == 37 and dws.failures[0] == 0 and dws.failures.sum() > 0 and (dws.trials == 128).all()
    assert abs(float(dws.logical_error_rate(0.1)["covered"]) - 1.0) < 1e-12
