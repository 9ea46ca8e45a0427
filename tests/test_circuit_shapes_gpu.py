"""The circuit-side kernels on the circuits of tests/circuit_shapes.py -- locations off every multiple of 4 and 32, sectors of unequal size with
partial words and an odd word count, k = 1 and k = 64, a base circuit that ends in a measurement -- bit for bit: the fault signatures against the
numpy frame model, the plain sampler against the oracle's literal walk, the fixed-weight, erasure, noise-model and soft-readout samplers against
their numpy models on the MODEL's signatures, and on shor and hgp (decoding matrices of unequal width) the host table builders and the
erasure-aware, soft-aware and correlated paths against the chain of their parts.  Parameters and expected outputs come from
test_circuit_shapes_cpu.py, which asserts that the draws reach the edges; every plan's batch is smaller than the trial count."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import circuit_shapes as CS  # noqa: E402
import correlated_model as CM  # noqa: E402
import erasure_model as EM  # noqa: E402
import soft_model as SM  # noqa: E402
import test_circuit_shapes_cpu as TC  # noqa: E402  (the parameters and the models' outputs, computed once)
from test_correlated_gpu import chain, logical_bits  # noqa: E402
from test_erasure_gpu import assert_aware_tally, aware_chain, verdicts  # noqa: E402
from test_soft_gpu import channels  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = TC.NAMES
SEED, COUNT, BATCH, BEGIN = TC.SEED, TC.COUNT, TC.BATCH, TC.BEGIN
AWARE = ("shor", "hgp")
AWARE_COUNT, AWARE_BATCH = 256, 100
AWARE_RATES = {"CNOT": 0.02, "MeasZ": 0.05, "PrepX": 0.05}                 # erasures of both sectors, mild enough that BP and the OSD stage both work
SENTINEL = 0xA5
_CACHE = {}


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


def setup(L, name):
    """(shape, model signatures, decoding matrices at P_LOW, graphs [Z, X], priors, masks, plan factory(p, batch, prior=...)), once per shape"""
    if name not in _CACHE:
        from qldpc_amd.noise.builder import build_decoding_matrices
        from qldpc_amd.simulation.engine import prior_llrs
        S, sigs = CS.shape(name), CS.model_signatures(name)
        M = build_decoding_matrices(S.cb, S.Lx, S.Lz, TC.P_LOW, verbose=False)
        graphs, priors, masks = [], [], []
        for s in "ZX":
            ip, ix, shape = L.canonical_csr(M[f"Hdec{s}"])
            flr = int(M[f"first_logical_row{s}"])
            graphs.append(L.Graph(ip, ix, shape[1]))
            priors.append(prior_llrs(np.asarray(M[f"channel_probs{s}"], dtype=np.float64)))
            masks.append(L.logical_column_masks(np.asarray(M[f"H{s}_full"])[flr:flr + S.k], shape[1]))

        def plan(p=TC.P_LOW, batch=BATCH, prior=None, **kw):
            pr = priors if prior is None else prior
            return L.CircuitPlan(S.compiled, S.Lx, S.Lz, graphs[0], graphs[1], pr[0], pr[1], masks[0], masks[1], p, batch=batch, **kw)
        _CACHE[name] = (S, sigs, M, graphs, priors, masks, plan)
    return _CACHE[name]


def assert_same(got, want, what):
    assert len(got) == len(want), what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, (what, i, a.shape, b.shape, a.dtype, b.dtype)
        bad = np.flatnonzero((a != b).reshape(a.shape[0], -1).any(axis=1))
        assert bad.size == 0, f"{what}: output {i}: trials {bad[:8].tolist()} differ ({bad.size} of {a.shape[0]})"


# ---------------------------------------------------------------------------------------- 1. signatures
@pytest.mark.parametrize("name", NAMES)
def test_signatures_equal_the_model(L, name):
    S, sigs = CS.shape(name), CS.model_signatures(name)
    for x in (False, True):
        got = L.circuit_fault_signatures(S.compiled, S.Lx, S.Lz, x)
        for what, a, b in zip(("ptr", "idx", "logmask"), got, sigs[x]):
            assert a.dtype == b.dtype and np.array_equal(a, b), (name, "ZX"[x], what)
    if name == "k64":
        assert all((sig[2] >> np.uint64(63)).any() for sig in sigs)


@pytest.mark.parametrize("name", NAMES)
def test_the_library_walk_of_chosen_faults(L, name):
    """run_trial_with_randoms itself (the kernels of noise/kernels.py) on six of the fault sets the model was checked with on the CPU"""
    from qldpc_amd.noise.simulation import run_trial_with_randoms
    S, sigs = CS.shape(name), CS.model_signatures(name)
    for faults in CS.random_fault_sets(S, 6, 11):
        got = CS.literal_trial(S.compiled, S.Lx, S.Lz, faults, run=run_trial_with_randoms)
        for i, (a, b) in enumerate(zip(got, CS.xor_of_signatures(S, sigs, faults))):
            assert np.array_equal(a, b), (name, faults, i)


# ---------------------------------------------------------------------------------------- 2. the plain sampler and the whole pipeline
@pytest.mark.parametrize("name", NAMES)
def test_plain_sampler_is_the_literal_walk(L, oracle, name):
    S, sigs, M, graphs, priors, masks, plan = setup(L, name)
    assert (graphs[0].m, graphs[1].m) == (S.nsx, S.nsz)
    circ = oracle.make_circuit(S.compiled, S.Lx, S.Lz)
    secs = []
    for s, nm in enumerate("ZX"):
        flr = int(M[f"first_logical_row{nm}"])
        ip, ix, shape = L.canonical_csr(M[f"Hdec{nm}"])
        lip, lix, _ = L.canonical_csr(np.asarray(M[f"H{nm}_full"])[flr:flr + S.k])
        secs.append(oracle.make_sector(ip, ix, shape[1], priors[s], lip, lix))
    for p, begin in ((TC.P_LOW, 0), (TC.P_HIGH[name], BEGIN)):
        q = plan(p)
        assert (q.n_locs, q.nsx, q.nsz, q.k, q.n_meas) == (S.n_locs, S.nsx, S.nsz, S.k, S.n_meas)
        assert_same(q.sample(SEED, begin, COUNT), TC.literal_samples(name, p, begin), f"{name} at p = {p}")
        q.run(SEED, begin, COUNT)
        got = q.read(clear=True)
        want = oracle.circuit_sample_decode_tally(circ, secs[0], secs[1], p, SEED, begin, COUNT, max_iter=50, threads=0)
        print(f"{name} at p = {p}: tally {got.tolist()}")
        assert np.array_equal(got, want), (name, p, got.tolist(), want.tolist())
        q.close()


# ---------------------------------------------------------------------------------------- 3. the four other samplers
@pytest.mark.parametrize("name", NAMES)
def test_fixed_weight_sampler_is_the_model(L, name):
    S, sigs, M, graphs, priors, masks, plan = setup(L, name)
    q = plan()
    last = TC.weights(name)[-1]
    for w in TC.weights(name):
        q.use_fixed_weight(w)
        assert_same(q.sample(SEED, BEGIN, COUNT), TC.expected(name, "fixed", w), f"{name}, w = {w}")
    before = q.sample(SEED, BEGIN, COUNT)
    assert L.lib().qldpc_circuit_plan_use_fixed_weight(q._h, S.n_locs + 1) == -1 and str(S.n_locs).encode() in L.lib().qldpc_last_error()
    with pytest.raises(L.QldpcError, match=f"{S.n_locs} fault locations"):
        q.use_fixed_weight(S.n_locs + 1)
    assert q.fixed_weight == last
    assert_same(q.sample(SEED, BEGIN, COUNT), before, "after w = N + 1")
    q.close()


def raw_record(L, q, entry, count, dtype, width):
    """sample_erasures / sample_soft through the C entry with a record buffer one row too long and filled with a sentinel -> (outputs, buffer)"""
    spz, spx = np.zeros((count, q.nsx), np.int8), np.zeros((count, q.nsz), np.int8)
    tz, tx = np.zeros((count, q.k), np.int8), np.zeros((count, q.k), np.int8)
    rec = np.full((count + 1, width), SENTINEL if dtype == np.uint8 else 0xA5A5A5A5, dtype)
    ct = C.c_uint8 if dtype == np.uint8 else C.c_uint32
    L.check(getattr(L.lib(), entry)(q._h, C.c_uint64(SEED), C.c_int64(0), C.c_int64(count), L.ptr(spz, C.c_int8), L.ptr(tz, C.c_int8),
                                    L.ptr(spx, C.c_int8), L.ptr(tx, C.c_int8), L.ptr(rec, ct), None, None))
    return (spz, tz, spx, tx), rec


@pytest.mark.parametrize("name", NAMES)
def test_erasure_sampler_is_the_model(L, name):
    S, sigs, M, graphs, priors, masks, plan = setup(L, name)
    *want, werased = TC.expected(name, "erasure")
    q = plan(TC.P_HIGH[name])
    q.use_erasure_noise(TC.ERASURE_RATES)
    *got, er = q.sample_erasures(SEED, 0, COUNT)
    nw = (S.n_locs + 31) // 32
    assert er.shape == (COUNT, nw) and er.dtype == np.uint32
    words = EM.pack_heralds(werased)
    assert np.array_equal(er, words)                                       # the partial last word included
    assert words[:, -1].any() and (S.n_locs % 32 == 0 or int(words[:, -1].max()) >> (S.n_locs % 32) == 0)
    assert_same(got, tuple(want), name)
    out, rec = raw_record(L, q, "qldpc_circuit_plan_sample_erasures", COUNT, np.uint32, nw)
    assert np.array_equal(rec[:COUNT], words) and (rec[COUNT] == 0xA5A5A5A5).all()      # the words past the record are untouched
    assert_same(out, tuple(want), name + ", raw")
    assert_same(q.sample(SEED, 0, COUNT), tuple(want), name + ", sample()")
    q.close()


@pytest.mark.parametrize("name", NAMES)
def test_noise_model_sampler_is_the_model(L, name):
    from qldpc_amd.simulation.noise_model import NoiseModel
    S, sigs, M, graphs, priors, masks, plan = setup(L, name)
    want, _ = TC.expected(name, "noise")
    nm = NoiseModel(TC.NOISE_RATES, idle_weights=TC.NOISE_IDLE_W, cnot_weights=TC.NOISE_CNOT_W)
    assert np.array_equal(nm.rates_by_op(), EM.rates_by_op(TC.NOISE_RATES))
    q = plan()
    today = q.sample(SEED, 0, COUNT)
    q.use_noise_model(nm)
    assert_same(q.sample(SEED, 0, COUNT), want, name)
    q.use_noise_model(None)
    assert_same(q.sample(SEED, 0, COUNT), today, name + ", off again")
    q.close()


@pytest.mark.parametrize("name", NAMES)
def test_soft_sampler_is_the_model(L, name):
    S, sigs, M, graphs, priors, masks, plan = setup(L, name)
    n = TC.SOFT_COUNT
    q = plan(TC.P_HIGH[name])
    today = q.sample(SEED, 0, n)
    assert_same(today, TC.models(name)[3].sample(TC.P_HIGH[name], None, SEED, 0, n)[:4], name + ", plain")
    for which in TC.CHANNELS:
        r = channels()[which]
        assert list(r.cut) == TC.cuts(which)                               # the channel of test_soft_gpu is the one the CPU module drew with
        *want, wlv, wflip = TC.expected(name, "soft", which)
        q.use_soft_readout(r)
        *got, lv = q.sample_soft(SEED, 0, n)
        assert lv.shape == (n, S.n_meas) and lv.dtype == np.uint8 and np.array_equal(lv, wlv), (name, which)
        assert_same(got, tuple(want), f"{name}, {which}")
        out, rec = raw_record(L, q, "qldpc_circuit_plan_sample_soft", n, np.uint8, S.n_meas)
        assert np.array_equal(rec[:n], wlv) and (rec[n] == SENTINEL).all()     # exactly n_meas columns: the row after the record is untouched
        assert_same(out, tuple(want), f"{name}, {which}, raw")
        assert wflip[:, -1].any()
    q.use_soft_readout(None)                                               # off: the plain sampler's output again, and no levels
    *off, lv = q.sample_soft(SEED, 0, n)
    assert_same(off, today, name + ", off again")
    assert not lv.any() and lv.shape == (n, S.n_meas)
    assert_same(q.sample(SEED, 0, n), today, name + ", sample() off again")
    q.close()


def test_batch_size_does_not_matter(L):
    """shor, every sampler: batches of 7 (14 launches) and 33 against the expected output that the batch of 40 was compared with above"""
    from qldpc_amd.simulation.noise_model import NoiseModel
    name = "shor"
    S, sigs, M, graphs, priors, masks, plan = setup(L, name)
    for batch in (7, 33):
        q = plan(TC.P_HIGH[name], batch=batch)
        assert_same(q.sample(SEED, BEGIN, COUNT), TC.literal_samples(name, TC.P_HIGH[name], BEGIN), f"plain, batch {batch}")
        q.use_fixed_weight(TC.W_ODD[name])
        assert_same(q.sample(SEED, BEGIN, COUNT), TC.expected(name, "fixed", TC.W_ODD[name]), f"fixed weight, batch {batch}")
        q.use_fixed_weight(None)
        q.use_erasure_noise(TC.ERASURE_RATES)
        *want, werased = TC.expected(name, "erasure")
        *got, er = q.sample_erasures(SEED, 0, COUNT)
        assert_same(got, tuple(want), f"erasure, batch {batch}")
        assert np.array_equal(er, EM.pack_heralds(werased))
        q.use_erasure_noise(None)
        q.use_noise_model(NoiseModel(TC.NOISE_RATES, idle_weights=TC.NOISE_IDLE_W, cnot_weights=TC.NOISE_CNOT_W))
        assert_same(q.sample(SEED, 0, COUNT), TC.expected(name, "noise")[0], f"noise model, batch {batch}")
        q.use_noise_model(None)
        q.use_soft_readout(channels()["gaussian"])
        *want, wlv, _ = TC.expected(name, "soft", "gaussian")
        *got, lv = q.sample_soft(SEED, 0, TC.SOFT_COUNT)
        assert_same(got, tuple(want), f"soft, batch {batch}")
        assert np.array_equal(lv, wlv)
        q.close()


SEVERAL = 2 * 4096 + 37               # a launch has at most 4096 workgroups: in one batch of this size they run three trials each, some two


@pytest.mark.parametrize("which", ["plain", "erasure", "noise", "soft"])
def test_workgroup_runs_several_trials(L, which):
    """shor (1 + 2 words of detector bits: the pad before the accumulators is in play), the four samplers the tests above pin with one trial per
    workgroup only: one batch of SEVERAL trials, where a workgroup zeroes its LDS between its trials, against batches of 1024, where none has to --
    every output bit for bit, the herald words and the levels included; the first 40 trials against the expected output of the tests above"""
    from qldpc_amd.simulation.noise_model import NoiseModel
    name = "shor"
    S, sigs, M, graphs, priors, masks, plan = setup(L, name)

    def draw(batch):
        q = plan(TC.P_LOW if which in ("plain", "noise") else TC.P_HIGH[name], batch=batch)
        if which == "erasure":
            q.use_erasure_noise(TC.ERASURE_RATES)
            out = q.sample_erasures(SEED, 0, SEVERAL)
        elif which == "soft":
            q.use_soft_readout(channels()["gaussian"])
            out = q.sample_soft(SEED, 0, SEVERAL)
        else:
            if which == "noise":
                q.use_noise_model(NoiseModel(TC.NOISE_RATES, idle_weights=TC.NOISE_IDLE_W, cnot_weights=TC.NOISE_CNOT_W))
            out = q.sample(SEED, 0, SEVERAL)
        q.close()
        return tuple(out)

    one_batch = draw(SEVERAL)
    assert_same(one_batch, draw(1024), f"{which}: one batch of {SEVERAL} against batches of 1024")
    if which == "plain":
        want = TC.literal_samples(name, TC.P_LOW, 0)
    elif which == "erasure":
        *want, werased = TC.expected(name, "erasure")
        want.append(EM.pack_heralds(werased))
    elif which == "noise":
        want = TC.expected(name, "noise")[0]
    else:
        want = TC.expected(name, "soft", "gaussian")[:5]
    assert_same(tuple(a[:40] for a in one_batch), tuple(w[:40] for w in want), f"{which}: the first 40 trials")
    assert all(a[4096:].any() for a in one_batch), which                   # the second and third trials of the workgroups are not all zeros


# ---------------------------------------------------------------------------------------- 4. host table builders and the aware paths
def aware_setup(L, name):
    """setup plus, once: the erasure tables, the soft tables and marginal priors of the gaussian channel, the links of both modes -- all from the
    MODEL's signatures"""
    key = ("aware", name)
    if key not in _CACHE:
        from qldpc_amd.simulation.correlated import links_from_circuit
        from qldpc_amd.simulation.erasure import erasure_tables_from_circuit
        from qldpc_amd.simulation.soft import marginal_priors, soft_tables_from_circuit
        S, sigs, M, graphs, priors, masks, plan = setup(L, name)
        r = channels()["gaussian"]
        era = erasure_tables_from_circuit(S.compiled, S.Lx, S.Lz, M, signatures=sigs)
        soft = soft_tables_from_circuit(S.compiled, S.Lx, S.Lz, M, r, signatures=sigs)
        links = {mode: links_from_circuit(S.compiled, S.Lx, S.Lz, M, TC.P_LOW, mode=mode, signatures=sigs) for mode in ("raise", "condition")}
        _CACHE[key] = (era, soft, marginal_priors(M, soft, r), links)
    return _CACHE[key]


@pytest.mark.parametrize("name", AWARE)
def test_the_builder_counts_each_sectors_detectors(L, name):
    S, sigs, M, graphs, priors, masks, plan = setup(L, name)
    assert M["HdecZ"].shape[0] == S.nsx == M["first_logical_rowZ"] and M["HdecX"].shape[0] == S.nsz == M["first_logical_rowX"] and S.nsx != S.nsz
    assert M["HZ_full"].shape[0] == S.nsx + S.k and M["HX_full"].shape[0] == S.nsz + S.k
    assert graphs[0].n != graphs[1].n                                      # the per-shot prior stride differs between the sectors
    for s, nm in enumerate("ZX"):                                          # the builder merged equal columns: (detectors, logical mask) names a column
        assert len(EM.columns_of(np.asarray(M[f"Hdec{nm}"]), masks[s])) == graphs[s].n


@pytest.mark.parametrize("name", AWARE)
def test_host_table_builders_equal_their_models(L, name):
    S, sigs, M, graphs, priors, masks, plan = setup(L, name)
    era, soft, marg, links = aware_setup(L, name)
    r, ty = channels()["gaussian"], np.asarray(S.compiled.base_ops)
    cols = []
    for s, nm in enumerate("ZX"):
        H, probs = np.asarray(M[f"Hdec{nm}"]), np.asarray(M[f"channel_probs{nm}"], np.float64)
        cols.append(EM.columns_of(H, masks[s]))
        want = EM.build_tables(ty, sigs[s], bool(s), cols[s], graphs[s].n, probs, priors[s])
        assert all(np.array_equal(a, b) for a, b in zip(EM.as_tuple(era[s]), EM.as_tuple(want))) and era[s].unmatched == want["unmatched"] == 0, (name, nm)
        assert (era[s].loc_h == 1).any() and (era[s].loc_h == EM.H_INF).any()
        want = SM.build_tables(ty, sigs[s], bool(s), cols[s], graphs[s].n, probs, r.cut)
        assert all(np.array_equal(a, b) for a, b in zip(SM.as_tuple(soft[s])[:4], SM.as_tuple(want)[:4])), (name, nm)
        assert soft[s].unmatched == want["unmatched"] == 0 and soft[s].levels == r.levels == 8 and soft[s].meas_col.size == S.n_meas
        assert np.array_equal(marg[s], SM.marginal_priors(probs, soft[s].meas_col, r.qbar))
    for mode, lk in links.items():
        ptr, src, llr, base, unmatched = CM.circuit_links(ty, sigs[0], sigs[1], cols[0], cols[1], graphs[1].n, M["channel_probsZ"], TC.P_LOW, mode)
        assert np.array_equal(lk.ptr, ptr) and np.array_equal(lk.src, src) and np.array_equal(lk.llr, llr) and lk.unmatched == unmatched == 0, (name, mode)
        assert (lk.base is None and base is None) if mode == "raise" else np.array_equal(lk.base, base)
        assert lk.n == graphs[1].n and lk.n_src == graphs[0].n and lk.n_links > 0


@pytest.mark.parametrize("name", AWARE)
def test_erasure_aware_plan_is_the_chain_of_its_parts(L, name):
    S, sigs, M, graphs, priors, masks, plan = setup(L, name)
    era = aware_setup(L, name)[0]
    q = plan(batch=AWARE_BATCH)
    q.use_erasure_aware(1.0, era)
    q.use_erasure_noise(AWARE_RATES)
    got = q.run_outcomes(SEED, 0, AWARE_COUNT)
    tally = q.read(clear=True)
    spz, tz, spx, tx, er, pz, px = q.sample_erasures(SEED, 0, AWARE_COUNT, want_priors=True)
    q.close()
    erased = EM.unpack_heralds(er, S.n_locs)
    stray = er.copy()
    if S.n_locs % 32:
        stray[:, -1] |= np.uint32((0xFFFFFFFF << (S.n_locs % 32)) & 0xFFFFFFFF)      # bits at or above n_locs are not locations
    for s, prior in enumerate((pz, px)):
        want = EM.priors(erased, era[s])
        assert prior.shape == (AWARE_COUNT, graphs[s].n) and np.array_equal(prior, want), (name, s)
        assert np.array_equal(L.erasure_priors(stray, era[s]), want), (name, s)
        assert (prior == 0.0).any() and (prior != priors[s][None, :]).any()
    dets, convs = aware_chain(L, graphs, (spz, spx), (pz, px), 1.0)
    print(f"{name}: erasure-aware: BP converged {int(convs[0].sum())} / {int(convs[1].sum())} of {AWARE_COUNT}, verdicts {np.bincount(got, minlength=4).tolist()}")
    assert np.array_equal(got, verdicts(masks, dets, (tz, tx))), name
    assert_aware_tally(L, tally, AWARE_COUNT, convs)
    assert 0 < convs[0].sum() < AWARE_COUNT and 0 < convs[1].sum() < AWARE_COUNT      # BP and the OSD stage both took part, in both sectors
    assert er.any() and erased[:, S.n_locs - 32:].any()


@pytest.mark.parametrize("name", AWARE)
def test_soft_aware_plan_is_the_chain_of_its_parts(L, name):
    S, sigs, M, graphs, priors, masks, plan = setup(L, name)
    _, soft, marg, _ = aware_setup(L, name)
    r = channels()["gaussian"]
    q = plan(batch=AWARE_BATCH, prior=marg)
    q.use_soft_aware(0.875, soft)
    q.use_soft_readout(r)
    got = q.run_outcomes(SEED, 0, AWARE_COUNT)
    tally = q.read(clear=True)
    spz, tz, spx, tx, lv, pz, px = q.sample_soft(SEED, 0, AWARE_COUNT, want_priors=True)
    q.close()
    for s, prior in enumerate((pz, px)):
        want = SM.priors(lv, soft[s])
        assert prior.shape == (AWARE_COUNT, graphs[s].n) and np.array_equal(prior, want) and np.array_equal(L.soft_priors(lv, soft[s]), want), (name, s)
    dets, convs = aware_chain(L, graphs, (spz, spx), (pz, px), 0.875)
    print(f"{name}: soft-aware: BP converged {int(convs[0].sum())} / {int(convs[1].sum())} of {AWARE_COUNT}, verdicts {np.bincount(got, minlength=4).tolist()}")
    assert np.array_equal(got, verdicts(masks, dets, (tz, tx))), name
    assert_aware_tally(L, tally, AWARE_COUNT, convs)
    assert 0 < convs[0].sum() < AWARE_COUNT and 0 < convs[1].sum() < AWARE_COUNT
    assert lv[:, -1].any() and lv.shape == (AWARE_COUNT, S.n_meas)


@pytest.mark.parametrize("mode", ["raise", "condition"])
@pytest.mark.parametrize("name", AWARE)
def test_correlated_plan_is_the_chain_of_its_parts(L, name, mode):
    S, sigs, M, graphs, priors, masks, plan = setup(L, name)
    lk = aware_setup(L, name)[3][mode]
    alpha = 0.875 if mode == "condition" else 1.0
    q = plan(TC.P_HIGH[name] / 4, batch=AWARE_BATCH)                       # enough faults that sector Z's corrections fire links
    q.use_correlated(alpha, lk, lk.base)
    got = q.run_outcomes(SEED, 0, AWARE_COUNT)
    tally = q.read(clear=True)
    spz, tz, spx, tx = q.sample(SEED, 0, AWARE_COUNT)
    q.close()
    (dz, cz), (dx, cx) = chain(L, graphs, priors, masks, (spz, spx), alpha, lk, lk.base)
    k = S.k
    truth = [(t.astype(np.uint64) << np.arange(k, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint64) for t in (tz, tx)]
    want = (logical_bits(dz, masks[0]) != truth[0]).astype(np.uint8) | ((logical_bits(dx, masks[1]) != truth[1]).astype(np.uint8) << 1)
    print(f"{name}: correlated, {mode}: BP converged {int(cz.sum())} / {int(cx.sum())} of {AWARE_COUNT}, verdicts {np.bincount(got, minlength=4).tolist()}")
    assert np.array_equal(got, want), (name, mode)
    assert_aware_tally(L, tally, AWARE_COUNT, (cz, cx))
    assert 0 < cz.sum() < AWARE_COUNT and 0 < cx.sum() < AWARE_COUNT
    assert tally[L.TALLY["legs_x"]] == 0 and dz.any() and dz[:, np.unique(lk.src)].any()      # some correction of sector Z uses a link's source
