"""The sampler and the trial judge of DEM plans on the MI355X over the shape family of tests/dem_shapes.py: dem_sample_kernel against the numpy model
bit for bit (several passes of each of its strided loops, a second trial per workgroup, the LDS maximum), the fused pipeline against sample -> batch
decoder -> host judge on both judge forms (sparse up to 4096 rows per sector, dense beyond) through run_outcomes, the 16 tally slots and decode_events,
and the two forms against each other where their inputs coincide.  Every comparison is exact.  tests/test_dem_shapes_cpu.py shows that none of the
inputs is vacuous."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dem_model as DM  # noqa: E402
import dem_shapes as S  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    assert _lib.TALLY == S.TALLY
    return _lib


_GRAPHS = {}


def graphs_of(L, c):
    """one Graph per sector of a case's decoder views; built once (the common-ground twin of a case shares them: its views are the same objects)"""
    key = c.name.split("/")[0]
    if key not in _GRAPHS:
        views = [c.dem.decoder_view(s) for s in range(c.dem.n_sectors)]
        _GRAPHS[key] = [L.Graph(v.indptr, v.indices, v.shape[1]) for v in views]
    return _GRAPHS[key]


def sectors_of(dem, sampled):
    """plan.sample's four arrays -> [(syndromes, true) per sector]"""
    return [(sampled[2 * s], sampled[2 * s + 1]) for s in range(dem.n_sectors)]


def assert_sample(got, want, what):
    for s, ((gs, gt), (ws, wt)) in enumerate(zip(got, want)):
        assert gs.dtype == gt.dtype == np.int8 and gs.shape == ws.shape and gt.shape == wt.shape, (what, s, gs.shape, gt.shape)
        bad = np.flatnonzero((gs != ws).any(axis=1) | (gt != wt).any(axis=1))
        assert bad.size == 0, f"{what}, sector {s}: trials {bad[:8].tolist()} differ from the model ({bad.size} of {gs.shape[0]})"


def assert_tally(L, got, want, what):
    names = sorted(L.TALLY, key=L.TALLY.get)
    diff = {n: (int(got[i]), int(want[i])) for i, n in enumerate(names) if got[i] != want[i]}
    assert not diff, f"{what}: tally slots (plan, parts): {diff}"


def minsum_parts(L, graphs, max_iter, osd=False):
    """decode() of dem_shapes.pipeline: the batch decoder a plain plan stands for -- flooding min-sum, then OSD-0 on the non-converged when the plan has
    the stage"""
    def decode(s, v, synd):
        det, conv, llr, iters = L.minsum_decode_batch(graphs[s], synd, v.prior, max_iter, "dynamical", 1.0)
        bad = np.flatnonzero(conv == 0)
        if osd and bad.size:
            det[bad] = L.osd0_batch(graphs[s], synd[bad], llr[bad], det[bad])
        return det, conv, int((iters.astype(np.int64) + 1).sum()), int(bad.size) if osd else 0
    return decode


# ---- the sampler ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", S.SEEDS)
@pytest.mark.parametrize("name", S.SAMPLER_CASES)
def test_sampler_is_the_model(L, name, seed):
    c = S.case(name)
    graphs = graphs_of(L, c)
    plan = c.dem.plan(graphs, batch=c.batch)
    got = plan.sample(seed, c.begin, c.count)
    plan.close()
    assert_sample(sectors_of(c.dem, got), S.reference(name, seed), name)
    if c.dem.n_sectors == 1:
        assert got[2].size == 0 and got[3].size == 0
    if name == "stride":                                         # one launch of 4096 workgroups above; four launches of 1024 here: the same draws
        other = c.dem.plan(graphs, batch=1024)
        again = other.sample(seed, c.begin, c.count)
        other.close()
        assert all(np.array_equal(a, b) for a, b in zip(got, again))


# ---- the pipeline and its parts -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iter", S.ITERS)
@pytest.mark.parametrize("name", S.JUDGE_CASES)
def test_pipeline_is_its_parts(L, name, max_iter):
    c = S.case(name)
    dem, graphs, seed, T = c.dem, graphs_of(L, c), S.SEEDS[0], L.TALLY
    plan = dem.plan(graphs, max_iter=max_iter, batch=c.batch, use_osd=False)
    sampled = sectors_of(dem, plan.sample(seed, c.begin, c.count))
    assert_sample(sampled, S.reference(name), name)
    verdict, want, kept = S.pipeline(dem, sampled, minsum_parts(L, graphs, max_iter))
    got = plan.run_outcomes(seed, c.begin, c.count)
    tally = plan.read(clear=True)
    bad = np.flatnonzero(got != verdict)
    assert bad.size == 0, f"{name}: verdicts of trials {bad[:8].tolist()} differ ({bad.size} of {c.count}): plan {got[bad[:8]].tolist()}, parts {verdict[bad[:8]].tolist()}"
    assert_tally(L, tally, want, name)
    print(f"{name} max_iter={max_iter}: tally {tally.tolist()}")
    assert want[T["unsat_z"]] > 0 and want[T["zero_synd_z"]] > 0 and 0 < want[T["bp_conv_z"]] < c.count
    cut = c.batch // 2 + 5                                       # two calls, cut inside a batch: the same verdicts, the same tally
    a, b = plan.run_outcomes(seed, c.begin, cut), plan.run_outcomes(seed, c.begin + cut, c.count - cut)
    assert np.array_equal(np.concatenate([a, b]), verdict)
    assert_tally(L, plan.read(clear=True), tally, name + " in two calls")
    one = plan.run_outcomes(seed, c.begin + 5, 1)                # B = 1
    assert np.array_equal(one, verdict[5:6])
    single = plan.read(clear=True)
    assert single[T["trials"]] == 1 and single[T["total_err"]] == int(verdict[5] != 0) and single[T["unsat_z"]] == int(DM.judge(dem.decoder_view(0), sampled[0][0][5:6], kept[0][0][5:6], sampled[0][1][5:6])[1][0])
    plan.run(seed, c.begin, c.count)                             # and without the verdicts
    assert_tally(L, plan.read(clear=True), tally, name + " without verdicts")
    if dem.n_sectors == 1:
        assert not (got & 2).any() and all(tally[T[k]] == 0 for k in T if k.endswith("_x") or k == "x_err")
    plan.close()


OSD_TRIALS = 6


@pytest.mark.parametrize("name", S.JUDGE_CASES)
def test_osd_stage_rides_along(L, name):
    """OSD-0 takes every matrix of the family (osd_shapes.rule_path, checked on the CPU side): a handful of trials around a BP failure"""
    c = S.case(name)
    dem, graphs, seed, T = c.dem, graphs_of(L, c), S.SEEDS[0], L.TALLY
    ref = S.reference(name)
    s0 = S.big_sector(name)
    conv = L.minsum_decode_batch(graphs[s0], ref[s0][0], dem.decoder_view(s0).prior, 2, "dynamical", 1.0)[1]
    first = int(np.flatnonzero(conv == 0)[0])                    # (there is one: test_judge_cases_reach_every_verdict)
    lo = min(max(first - 2, 0), c.count - OSD_TRIALS)
    plan = dem.plan(graphs, max_iter=2, batch=8, use_osd=True)
    sampled = sectors_of(dem, plan.sample(seed, c.begin + lo, OSD_TRIALS))
    assert_sample(sampled, [(a[lo:lo + OSD_TRIALS], b[lo:lo + OSD_TRIALS]) for a, b in ref], name)
    verdict, want, kept = S.pipeline(dem, sampled, minsum_parts(L, graphs, 2, osd=True))
    got = plan.run_outcomes(seed, c.begin + lo, OSD_TRIALS)
    tally = plan.read(clear=True)
    plan.close()
    assert np.array_equal(got, verdict), (name, got.tolist(), verdict.tolist())
    assert_tally(L, tally, want, name + " with OSD-0")
    assert want[T["osd_" + "zx"[s0]]] > 0


# ---- pointed records through decode_events ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.JUDGE_CASES)
def test_pointed_records(L, name):
    c = S.case(name)
    dem, graphs = c.dem, graphs_of(L, c)
    synd, rows = S.pointed_syndromes(dem)
    count = synd[0].shape[0]
    plan = dem.plan(graphs, max_iter=1, batch=8, use_osd=False)   # (more records than a batch: the last batch is ragged)
    records = L.pack_events(np.concatenate(synd, axis=1))        # the default layout: sector 0's rows, then sector 1's
    pred0, pred1, flags = plan.decode_events(records, seed=3, shot_begin=0)
    unpacked = plan.unpack_events(records)
    plan.close()
    want_pred, want_flags = [np.zeros(count, np.uint64), np.zeros(count, np.uint64)], np.zeros(count, np.uint8)
    for s in range(dem.n_sectors):
        v = dem.decoder_view(s)
        assert np.array_equal(unpacked[s], synd[s])
        det, conv, llr, iters = L.minsum_decode_batch(graphs[s], synd[s], v.prior, 1, "dynamical", 1.0)
        err, unsat, zero = DM.judge(v, synd[s], det, np.zeros((count, dem.k[s]), np.int8))
        want_pred[s] = DM.predict(v, det)
        want_flags |= ((conv != 0).astype(np.uint8) << s) | (unsat.astype(np.uint8) << (2 + s)) | (zero.astype(np.uint8) << (4 + s))
        mine = np.array([False] + [t == s for t, _ in rows])      # the one set row alone leaves its sector unsatisfied
        assert np.array_equal(unsat, mine) and np.array_equal(zero, ~mine), (name, s)
    for r in range(count):
        what = (name, "empty record" if r == 0 else f"sector {rows[r - 1][0]} row {rows[r - 1][1]}")
        assert int(pred0[r]) == int(want_pred[0][r]) and int(pred1[r]) == int(want_pred[1][r]), (what, hex(int(pred0[r])), hex(int(pred1[r])))
        assert int(flags[r]) == int(want_flags[r]), (what, bin(int(flags[r])), bin(int(want_flags[r])))
    if name == "tail63":                                         # det[n - 1] = 1 in every shot: bit 63 comes from the scan's last byte alone
        assert (pred0 == np.uint64(1 << 63)).all()


# ---- dense = sparse on common ground -------------------------------------------------------------------------------------------------------------------
_COMMON = {}


def common_run(L, name, max_iter):
    if (name, max_iter) not in _COMMON:
        c = S.common_ground(name)
        plan = c.dem.plan(graphs_of(L, c), max_iter=max_iter, batch=c.batch, use_osd=False)
        out = plan.run_outcomes(S.SEEDS[0], c.begin, c.count)
        _COMMON[(name, max_iter)] = (out, plan.read(clear=True))
        plan.close()
    return _COMMON[(name, max_iter)]


@pytest.mark.parametrize("max_iter", S.ITERS)
@pytest.mark.parametrize("name", S.DENSE_CASES)
def test_dense_is_sparse_on_common_ground(L, name, max_iter):
    """rows_4096's sector 0 and the 4097-row sector of `name` hold the same mechanisms under the same numbers; with those on row 4096 silenced they
    draw and decode alike (dem_shapes.common_ground, test_common_ground_decodes_alike), so the sparse and the dense judge must agree"""
    T = L.TALLY
    (va, ta), (vb, tb) = common_run(L, "rows_4096", max_iter), common_run(L, name, max_iter)
    sa, sb = 0, S.big_sector(name)
    bad = np.flatnonzero(((va >> sa) & 1) != ((vb >> sb) & 1))
    assert bad.size == 0, f"{name}: the dense and the sparse judge differ on trials {bad[:8].tolist()}"
    for slot in S.SECTOR_SLOTS:
        assert ta[T[slot.format("zx"[sa])]] == tb[T[slot.format("zx"[sb])]], (name, slot, ta.tolist(), tb.tolist())
    assert ta[T["trials"]] == tb[T["trials"]] and 0 < ta[T["z_err"]] < ta[T["trials"]]


# ---- the circuit sampler across trial 2^32 --------------------------------------------------------------------------------------------------------------
def test_circuit_sampler_crosses_the_counter_word(L, oracle, golden):
    """no other test samples a circuit plan beyond trial 2^32 - 1: eight circ72 trials from 2^32 - 4 against the oracle's literal simulation"""
    from qldpc_amd.data import load_circuit_matrices
    g, d = golden("circ72_noise"), load_circuit_matrices("circ72")
    circ = oracle.make_circuit(g, g["Lx"], g["Lz"])
    graphs, priors, masks = [], [], []
    for s in "ZX":
        n = int(d[f"Hdec{s}_shape"][1])
        graphs.append(L.Graph(d[f"Hdec{s}_indptr"], d[f"Hdec{s}_indices"], n))
        priors.append(oracle.prior_llrs(d[f"channel_probs{s}"]))
        masks.append(L.logical_column_masks((d[f"H{s}_logical_indptr"], d[f"H{s}_logical_indices"]), n))
    p, seed, begin = 0.02, 4242, (1 << 32) - 4
    plan = L.CircuitPlan(g, g["Lx"], g["Lz"], graphs[0], graphs[1], priors[0], priors[1], masks[0], masks[1], p, batch=64)
    got = plan.sample(seed, begin, 8)
    plan.close()
    for t in range(8):
        want = oracle.circuit_sample(circ, p, seed, begin + t)
        assert all(np.array_equal(a[t], b) for a, b in zip(got, want)), t
    assert got[0].any() and got[2].any() and not np.array_equal(got[0][:4], got[0][4:])
