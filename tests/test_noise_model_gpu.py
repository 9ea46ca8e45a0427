"""The per-class, biased Pauli noise model of a circuit plan, on circ72 -- the small plan of tests/test_plan_switch_gpu.py (288 rows per sector): the
sampler equals the numpy model of tests/noise_model_model.py bit for bit, uniform(P) is today's sampler, position and batching do not matter, the
refusals leave the plan alone, the plan equals the chain of its parts on three decode paths, the matched priors follow their rule, and
run_simulation(noise_model=...) carries it through."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import correlated_model as CM  # noqa: E402
import erasure_model as EM  # noqa: E402
import noise_model_model as NM  # noqa: E402
from fixed_weight_model import OP_CNOT, OP_IDLE  # noqa: E402
from test_plan_switch_gpu import SWITCHES  # noqa: E402
from test_relay_gpu import _bb_params, circuit_setup  # noqa: E402

pytestmark = pytest.mark.gpu

SEED, COUNT, P = 4099, 384, 0.005                                          # (P: what circuit_setup's plans sample at)
_CNOT_W = np.random.default_rng(5).random(15)
_CNOT_W[[3, 9, 14]] = 0.0                                                  # three Paulis that are never drawn, the last one among them
_CNOT_W0 = np.ones(15)
_CNOT_W0[[0, 1, 7]] = 0.0                                                  # the first two cuts are 0: the kernel counts them instead of comparing
# name -> (rates, idle weights, CNOT weights)
MODELS = {
    "classes": ({"CNOT": 0.004, "PrepX": 0.01, "PrepZ": 0.0, "MeasX": 0.02, "MeasZ": 0.007, "IDLE": 0.003}, None, None),
    "biased idle": (P, (1.0, 1.0, 20.0), None),
    "cnot weights": (P, None, _CNOT_W),
    "zero first": (P, (0.0, 1.0, 3.0), _CNOT_W0),                              # a zero FIRST weight in both tables (cut 0), beside the zero last ones above
    "si1000": ({"CNOT": 0.005, "PrepX": 2 * 0.005, "PrepZ": 2 * 0.005, "MeasX": 5 * 0.005, "MeasZ": 5 * 0.005, "IDLE": 0.005 / 10}, None, None),
}
_CACHE = {}


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


def NoiseModel(name):
    from qldpc_amd.simulation.noise_model import NoiseModel as M
    if name == "si1000":
        return M.si1000(0.005)
    rates, iw, cw = MODELS[name]
    return M(rates, idle_weights=iw, cnot_weights=cw)


def setup(L):
    """circuit_setup of circ72 plus, once: the fault signatures and the sampler model"""
    if "s" not in _CACHE:
        c, compiled, M, graphs, priors, masks, plan = circuit_setup(L, "circ72")
        sigs = (L.circuit_fault_signatures(compiled, c["Lx"], c["Lz"], False), L.circuit_fault_signatures(compiled, c["Lx"], c["Lz"], True))
        model = NM.SamplerModel(sigs[0], sigs[1], np.asarray(compiled.base_ops), (graphs[0].m, graphs[1].m), np.asarray(c["Lx"]).shape[0])
        _CACHE["s"] = (c, compiled, M, graphs, priors, masks, plan, sigs, model)
    return _CACHE["s"]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


# ---------------------------------------------------------------------------------------- 1. the sampler equals the model
@pytest.mark.parametrize("which", list(MODELS))
def test_the_sampler_equals_the_model(L, which):
    c, compiled, M, graphs, priors, masks, plan, sigs, model = setup(L)
    assert graphs[0].m == graphs[1].m == 288
    rates, iw, cw = MODELS[which]
    nm = NoiseModel(which)
    assert np.array_equal(nm.rates_by_op(), NM.rates_by_op(rates))          # (si1000(0.005) is the dict above)
    want, (b, l, idx) = model.sample_model(rates, iw, cw, SEED, 0, COUNT)
    # what the model's own draws cover on these 384 trials
    ty, by_op = model.loc_type[l], NM.rates_by_op(rates)
    for op in range(1, 7):
        assert bool((ty == op).any()) == (by_op[op] > 0), op
    idle, cnot = set(idx[ty == OP_IDLE].tolist()), set(idx[ty == OP_CNOT].tolist())
    assert idle == ({0, 1, 2} if iw is None else {i for i in range(3) if iw[i] > 0})
    assert cnot == (set(range(15)) if cw is None else {i for i in range(15) if cw[i] > 0})
    if which == "cnot weights":
        assert not cnot & {3, 9, 14} and len(cnot) == 12
    p = plan(batch=128)                                                     # three batches
    p.use_noise_model(nm)
    got = p.sample(SEED, 0, COUNT)
    assert same(got, want)
    assert got[0].any() and got[2].any() and got[1].any() and got[3].any()
    er = p.sample_erasures(SEED, 0, COUNT)                                  # sample_erasures honours it; no herald
    assert same(er[:4], want) and not er[4].any()
    p.close()


# ---------------------------------------------------------------------------------------- 2. today's sampler bit for bit
def test_uniform_is_todays_sampler_and_the_switch_is_two_way(L):
    from qldpc_amd.simulation.noise_model import NoiseModel as M
    plan = setup(L)[6]
    p = plan(batch=128)
    today = p.sample(SEED, 0, COUNT)
    today_er = p.sample_erasures(SEED, 0, COUNT)
    p.use_noise_model(M.uniform(P))
    assert same(p.sample(SEED, 0, COUNT), today) and p.noise_model is not None
    p.use_noise_model(NoiseModel("classes"))
    other = p.sample(SEED, 0, COUNT)
    assert not np.array_equal(other[0], today[0]) and not np.array_equal(other[2], today[2])
    p.use_noise_model(M.uniform(0.004))                                     # another p is another sampler
    assert not np.array_equal(p.sample(SEED, 0, COUNT)[0], today[0])
    p.use_noise_model(None)
    assert p.noise_model is None
    assert same(p.sample(SEED, 0, COUNT), today) and same(p.sample_erasures(SEED, 0, COUNT), today_er)
    p.use_noise_model(NoiseModel("classes"))                                # on again: the same samples as before
    assert same(p.sample(SEED, 0, COUNT), other)
    p.close()


# ---------------------------------------------------------------------------------------- 3. position and batch
def test_position_and_batch_independence(L):
    plan = setup(L)[6]
    outs = {}
    for batch in (128, 37):
        p = plan(batch=batch)
        p.use_noise_model(NoiseModel("cnot weights"))
        outs[batch] = p.sample(SEED, 0, COUNT)
        if batch == 128:
            part = p.sample(SEED, 100, 50)
        p.close()
    assert same(outs[37], outs[128])
    assert same(part, [x[100:150] for x in outs[128]])


# ---------------------------------------------------------------------------------------- 4. refusals
def raw_model(L, rates, idle_w=None, cnot_w=None):
    """a qldpc_noise_model filled by hand: what NoiseModel itself would refuse still has to be refused by the library"""
    s = L.NoiseModelStruct()
    keep = [None if w is None else np.ascontiguousarray(w, np.float64) for w in (idle_w, cnot_w)]
    for i, r in enumerate(rates):
        s.rate[i] = r
    s.idle_w = keep[0].ctypes.data_as(C.POINTER(C.c_double)) if keep[0] is not None else None
    s.cnot_w = keep[1].ctypes.data_as(C.POINTER(C.c_double)) if keep[1] is not None else None
    return s, keep


def test_refusals_leave_the_plan_as_it_was(L):
    from qldpc_amd.simulation.noise_model import NoiseModel as M
    plan = setup(L)[6]
    ok = [0.0] + [0.01] * 6
    bad_cnot = np.ones(15)
    bad_cnot[11] = -0.5
    cases = ((ok[:4] + [1.0] + ok[5:], None, None, b"rate[4] (MeasX)"), (ok[:6] + [float("nan")], None, None, b"rate[6] (IDLE)"),
             (ok[:2] + [-0.25] + ok[3:], None, None, b"rate[2] (PrepX)"), (ok, None, bad_cnot, b"cnot_w[11]"), (ok, (1.0, float("inf"), 1.0), None, b"idle_w[1]"),
             (ok, np.zeros(3), None, b"idle_w[0..2] sums to 0"), (ok, None, np.zeros(15), b"cnot_w[0..14] sums to 0"))
    for state in ("fresh", "switched"):
        p = plan(batch=128)
        if state == "switched":
            p.use_noise_model(NoiseModel("biased idle"))
        before = p.sample(SEED, 0, 128)
        for rates, iw, cw, text in cases:
            s, keep = raw_model(L, rates, iw, cw)
            assert L.lib().qldpc_circuit_plan_use_noise_model(p._h, C.byref(s)) == -1
            assert text in L.lib().qldpc_last_error(), (text, L.lib().qldpc_last_error())
            assert same(p.sample(SEED, 0, 128), before), (state, text)
        p.close()
    model = NoiseModel("classes")
    p = plan(batch=128)
    today = p.sample(SEED, 0, 128)
    p.use_fixed_weight(5)                                                   # fixed weight first: the model is refused
    fixed = p.sample(SEED, 0, 128)
    with pytest.raises(L.QldpcError, match=r"error -1: .*fixed weight"):
        p.use_noise_model(model)
    assert same(p.sample(SEED, 0, 128), fixed) and p.noise_model is None
    p.use_fixed_weight(None)
    p.use_noise_model(model)                                                # the model first: a fixed weight is refused, switching it off is not
    noisy = p.sample(SEED, 0, 128)
    with pytest.raises(L.QldpcError, match=r"error -1: .*noise model"):
        p.use_fixed_weight(5)
    p.use_fixed_weight(None)
    assert same(p.sample(SEED, 0, 128), noisy) and p.fixed_weight is None
    with pytest.raises(L.QldpcError, match=r"error -1: .*noise model"):     # ... and so is erasure noise, and switching that off is not
        p.use_erasure_noise(0.01)
    p.use_erasure_noise(None)
    assert same(p.sample(SEED, 0, 128), noisy) and p.erasure_rates is None
    p.use_noise_model(None)
    p.use_erasure_noise({"CNOT": 0.02})                                     # erasure noise first: the model is refused
    erased = p.sample_erasures(SEED, 0, 128)
    with pytest.raises(L.QldpcError, match=r"error -1: .*erasure noise"):
        p.use_noise_model(model)
    assert same(p.sample_erasures(SEED, 0, 128), erased) and erased[4].any() and p.noise_model is None
    p.use_erasure_noise(None)
    assert same(p.sample(SEED, 0, 128), today)
    p.close()
    toy = CM.toy_dem()                                                      # a DEM plan has no gate locations
    views = [toy.decoder_view(s) for s in range(2)]
    d = toy.plan([L.Graph(v.indptr, v.indices, v.shape[1]) for v in views], batch=64)
    sampled = d.sample(3, 0, 64)
    with pytest.raises(L.QldpcError, match=r"error -1: .*circuit plan"):
        d.use_noise_model(M.uniform(0.01))
    assert same(d.sample(3, 0, 64), sampled) and d.noise_model is None
    d.use_noise_model(None)                                                 # off is always allowed
    d.close()
    p = plan(batch=64)
    with pytest.raises(ValueError, match="NoiseModel"):
        p.use_noise_model({"CNOT": 0.01})
    p.close()


# ---------------------------------------------------------------------------------------- 5. the plan equals the chain of its parts
@pytest.mark.parametrize("how", ["default", "layered, then the model", "the model, then osd_cs"])
def test_the_plan_equals_the_chain_of_its_parts(L, how):
    plan = setup(L)[6]
    p = plan(batch=128)
    if how.startswith("layered"):
        SWITCHES["layered"][1](p)                                           # a BP-side switch first ...
    p.use_noise_model(NoiseModel("si1000"))
    if how.endswith("osd_cs"):
        SWITCHES["osd_cs"][1](p)                                            # ... an OSD-side one after
    got = p.run_outcomes(SEED, 0, COUNT)
    tally = p.read(clear=True)
    spz, tz, spx, tx = p.sample(SEED, 0, COUNT)
    pred0, pred1, _ = p.decode_events(L.pack_events(np.hstack([spz, spx])))      # the default layout: sector 0's rows, then sector 1's
    k = tz.shape[1]
    truth = [(t.astype(np.uint64) << np.arange(k, dtype=np.uint64)[None, :]).sum(axis=1).astype(np.uint64) for t in (tz, tx)]
    want = (pred0 != truth[0]).astype(np.uint8) | ((pred1 != truth[1]).astype(np.uint8) << 1)
    assert np.array_equal(got, want), how
    T = L.TALLY
    assert tally[T["trials"]] == COUNT and tally[T["total_err"]] == np.count_nonzero(want)
    assert 0 < tally[T["bp_conv_z"]] < COUNT or 0 < tally[T["bp_conv_x"]] < COUNT       # BP and the OSD stage both took part
    q = plan(batch=128)                                                     # not the unswitched plan's trials
    assert not np.array_equal(q.sample(SEED, 0, COUNT)[0], spz)
    q.close()
    p.close()


# ---------------------------------------------------------------------------------------- 6. priors
def column_feeds(L):
    """per sector: for every column the set of op codes whose faults reach it, and the list (op code, projections a location has in a column) --
    enumerated here from the signatures and the dense matrices, not through the package"""
    if "feeds" not in _CACHE:
        c, compiled, M, graphs, priors, masks, plan, sigs, model = setup(L)
        out = []
        for is_x, name in enumerate("ZX"):
            cols = EM.columns_of(M[f"Hdec{name}"].toarray(), masks[is_x])
            ptr, idx, lm = sigs[is_x]
            single = (5, 3, 6) if is_x else (4, 2, 6)                       # MeasZ, PrepZ, IDLE / MeasX, PrepX, IDLE
            classes = [set() for _ in range(graphs[is_x].n)]
            hits, unmatched = [], 0

            def s(e):
                return frozenset(int(v) for v in idx[ptr[e]:ptr[e + 1]]), int(lm[e])
            for i, op in enumerate(model.loc_type.tolist()):
                if op in single:
                    faults = [s(2 * i)]
                elif op == OP_CNOT:
                    a, b = s(2 * i), s(2 * i + 1)
                    faults = [a, b, (a[0] ^ b[0], a[1] ^ b[1])]
                else:
                    continue
                for f in faults:
                    if f not in cols:                                       # (a fault that flips nothing has a column only if the matrix kept one)
                        unmatched += bool(f[0] or f[1])
                        continue
                    classes[cols[f]].add(op)
                    hits.append(op)
            out.append((classes, np.array(hits), unmatched))
        _CACHE["feeds"] = out
    return _CACHE["feeds"]


def test_uniform_priors_are_the_shipped_ones(L):
    from qldpc_amd.simulation.noise_model import NoiseModel as M
    c, compiled, Mx, graphs, priors, masks, plan, sigs, model = setup(L)
    pz, px = M.uniform(P).channel_probs(compiled, c["Lx"], c["Lz"], Mx, signatures=sigs)
    assert pz.dtype == np.float64 and np.array_equal(pz, np.asarray(Mx["channel_probsZ"], np.float64))
    assert np.array_equal(px, np.asarray(Mx["channel_probsX"], np.float64))
    lz, lx = M.uniform(P).prior_llrs(compiled, c["Lx"], c["Lz"], Mx, signatures=sigs)
    assert np.array_equal(lz, priors[0]) and np.array_equal(lx, priors[1])
    pz2, px2 = M.uniform(P).channel_probs(compiled, c["Lx"], c["Lz"], Mx)   # the signatures computed on the device: the same
    assert np.array_equal(pz2, pz) and np.array_equal(px2, px)


def test_a_class_at_rate_zero_empties_exactly_its_own_columns(L):
    from qldpc_amd.simulation.noise_model import NoiseModel as M, PRIOR_FLOOR
    from qldpc_amd.simulation.engine import prior_llrs
    c, compiled, Mx, graphs, priors, masks, plan, sigs, model = setup(L)
    feeds = column_feeds(L)
    floor_llr = float(prior_llrs(np.array([1e-12]))[0])
    assert PRIOR_FLOOR == 1e-12 and 27.0 < floor_llr < 28.0
    emptied = 0
    for gate, op in EM.GATE_OP.items():
        rates = {g: 0.01 for g in EM.GATE_OP}
        rates[gate] = 0.0
        nm = M(rates)
        probs = nm.channel_probs(compiled, c["Lx"], c["Lz"], Mx, signatures=sigs)
        llrs = nm.prior_llrs(compiled, c["Lx"], c["Lz"], Mx, signatures=sigs)
        for s in range(2):
            only = np.array([cl == {op} for cl in feeds[s][0]])
            assert np.array_equal(probs[s] == 0.0, only), (gate, s)
            assert np.all(llrs[s][only] == floor_llr) and np.all(llrs[s][~only] < floor_llr) and np.isfinite(llrs[s]).all()
            emptied += int(only.sum())
    assert emptied > 0                                                      # some class has columns of its own on this circuit
    assert all(cl for s in range(2) for cl in feeds[s][0]) and feeds[0][2] == feeds[1][2] == 0      # every column is fed; every fault has a column


def test_si1000_total_mass(L):
    c, compiled, Mx, graphs, priors, masks, plan, sigs, model = setup(L)
    nm = NoiseModel("si1000")
    rate = nm.rates_by_op()
    probs = nm.channel_probs(compiled, c["Lx"], c["Lz"], Mx, signatures=sigs)
    for s in range(2):
        hits = column_feeds(L)[s][1]                                        # one entry per (location, projection that has a column)
        mass = np.where(hits == OP_IDLE, rate[hits] * 2 / 3, np.where(hits == OP_CNOT, rate[hits] * 4 / 15, rate[hits]))
        want = float(np.sum(mass.astype(np.longdouble)))
        assert abs(float(probs[s].sum()) - want) <= 1e-12 * want and want > 0
        assert not np.array_equal(probs[s], np.asarray(Mx[f"channel_probs{'ZX'[s]}"]))


# ---------------------------------------------------------------------------------------- 7. run_simulation
def test_run_simulation_noise_model(L):
    from qldpc_amd.data import load_code, load_precomputed_matrices
    from qldpc_amd.simulation.engine import run_simulation
    from qldpc_amd.simulation.noise_model import NoiseModel as M
    plan = setup(L)[6]
    c = load_code("bb72")
    kw = dict(num_cycles=6, precomputed_matrices=load_precomputed_matrices("circ72"), base_seed=SEED, batch=512, num_trials=2048, devices=[0], **_bb_params(c))
    args = (c["Hx"], c["Hz"], c["Lx"], c["Lz"], P)
    r0 = run_simulation(*args, **kw)
    r1 = run_simulation(*args, noise_model=M.uniform(P), **kw)
    assert r0["tally"][L.TALLY["trials"]] == 2048 and np.array_equal(r0["tally"], r1["tally"])
    assert "noise_model" not in r0 and r1["matched_priors"] is True and r1["noise_model"].rates_by_op().tolist() == [0] + [P] * 6
    si = M.si1000(P)
    matched = run_simulation(*args, noise_model=si, **kw)
    uniform = run_simulation(*args, noise_model=si, matched_priors=False, **kw)
    assert matched["tally"][L.TALLY["trials"]] == uniform["tally"][L.TALLY["trials"]] == 2048 and uniform["matched_priors"] is False
    assert not np.array_equal(matched["tally"], uniform["tally"]) and not np.array_equal(uniform["tally"], r0["tally"])
    p = plan(batch=512)                                                     # matched_priors=False is the shipped plan with the sampler switched
    p.use_noise_model(si)
    p.run(SEED, 0, 2048)
    assert np.array_equal(p.read(), uniform["tally"])
    p.close()
    two = run_simulation(*args, noise_model=si, **dict(kw, devices=[0, 0], num_workers=2))      # every worker's plan is switched
    assert np.array_equal(two["tally"], matched["tally"]) and two["num_workers"] == 2
