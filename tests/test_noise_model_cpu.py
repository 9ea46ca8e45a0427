"""The per-class, biased Pauli noise model without a GPU: the cuts of a weight table and the choice they make on the edge words, the argument rules of
NoiseModel and its constructors, the matched channel probabilities on the hand-made circuit of tests/test_erasure_cpu.py by enumerating every Pauli,
the argument rules of run_simulation(noise_model=...) and run_weight_strata, and the binding."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import noise_model_model as NM  # noqa: E402
from fixed_weight_model import CNOT_COMP, IDLE_COMP, OP_CNOT, OP_IDLE, OP_MEAS_X, OP_MEAS_Z, OP_PREP_X, OP_PREP_Z  # noqa: E402
from test_erasure_cpu import COLS_X, COLS_Z, OPS, SIG_X, SIG_Z, matrices, sig_table  # noqa: E402

TOP = 2 ** 32


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def N():
    import qldpc_amd  # noqa: F401
    from qldpc_amd.simulation import noise_model
    return noise_model


def drawn(r, cut):
    return int(NM.choose(np.array([r]), cut)[0])


# ---------------------------------------------------------------------------------------- 1. cuts
@pytest.mark.parametrize("K", [3, 15, 2, 7])
def test_equal_weights_cut_the_words_evenly(N, K):
    for w in (np.ones(K), np.full(K, 0.375)):
        want = [TOP * (i + 1) // K for i in range(K - 1)]
        assert NM.cuts(w) == want and N.weight_cuts(w).tolist() == want and N.weight_cuts(w).dtype == np.uint64


def test_cuts_are_monotone_and_scale_free(N):
    rng = np.random.default_rng(7)
    for K in (3, 15):
        for _ in range(50):
            w = rng.random(K) * (rng.random(K) < 0.7)
            w[int(rng.integers(K))] += 0.5                                  # a positive sum
            cut = NM.cuts(w)
            assert cut == N.weight_cuts(w).tolist()
            assert all(0 <= a <= b <= TOP for a, b in zip(cut, cut[1:] + [TOP]))
            for scale in (2.0 ** -40, 8.0, 2.0 ** 60):                      # a power of two changes no quotient S_i / S
                assert NM.cuts(w * scale) == cut
            p = np.diff([0] + cut + [TOP]) / TOP                            # every probability within 2^-32 of w_i / S
            assert np.all(np.abs(p - w / w.sum()) <= 2.0 ** -32 + 1e-15)


def test_zero_weights_give_empty_intervals(N):
    first, middle, last = NM.cuts([0, 1, 1]), NM.cuts([1, 0, 1]), NM.cuts([1, 1, 0])
    assert first == [0, TOP // 2] and middle == [TOP // 2, TOP // 2] and last == [TOP // 2, TOP]
    for w, want in (([0, 1, 1], first), ([1, 0, 1], middle), ([1, 1, 0], last), ([0, 0, 5], [0, 0]), ([5, 0, 0], [TOP, TOP])):      # the package's cuts: the same literals
        assert N.weight_cuts(w).tolist() == want and N.NoiseModel(0.01, idle_weights=w).cuts()[0].tolist() == want
    words = [0, 1, TOP // 2 - 1, TOP // 2, TOP - 2, TOP - 1]
    assert {drawn(r, first) for r in words} == {1, 2} and drawn(0, first) == 1
    assert {drawn(r, middle) for r in words} == {0, 2} and drawn(TOP // 2 - 1, middle) == 0 and drawn(TOP // 2, middle) == 2
    assert {drawn(r, last) for r in words} == {0, 1} and drawn(TOP - 1, last) == 1        # a zero last weight is never drawn, not even by the top word
    assert NM.cuts([0, 0, 5]) == [0, 0] and drawn(0, [0, 0]) == 2
    assert NM.cuts([5, 0, 0]) == [TOP, TOP] and drawn(TOP - 1, [TOP, TOP]) == 0
    w = np.ones(15)
    w[[0, 6, 14]] = 0
    cut = NM.cuts(w)
    got = {drawn(r, cut) for r in np.linspace(0, TOP - 1, 4001).astype(np.int64).tolist() + [c for c in cut if c < TOP] + [c - 1 for c in cut if c > 0]}
    assert got == set(range(15)) - {0, 6, 14}


def test_model_choice_without_weights_is_the_modulus(N):
    assert N.NoiseModel(0.01).cuts() == (None, None) and tuple(N.IDLE_COMP) == tuple(IDLE_COMP.tolist()) and tuple(N.CNOT_COMP) == tuple(CNOT_COMP.tolist())
    r = np.array([0, 1, 2, 3, 14, 15, 16, TOP - 1], np.int64)
    assert NM.pauli_index(np.full(8, OP_IDLE), r, None, None).tolist() == (r % 3).tolist()
    assert NM.pauli_index(np.full(8, OP_CNOT), r, None, None).tolist() == (r % 15).tolist()
    assert NM.pauli_index(np.full(8, OP_MEAS_X), r, None, None).tolist() == [0] * 8
    assert NM.components(np.array([OP_MEAS_X, OP_PREP_X, OP_MEAS_Z, OP_PREP_Z, OP_IDLE, OP_CNOT]), np.array([0, 0, 0, 0, 2, 14])).tolist() == [4, 4, 1, 1, 4, 6]


# ---------------------------------------------------------------------------------------- 2. argument rules
def test_noise_model_argument_rules(N):
    M = N.NoiseModel
    assert M(0.01).rates_by_op().tolist() == [0] + [0.01] * 6 and M(0.01).cuts() == (None, None)
    assert M({"CNOT": 0.02, "IDLE": 0.5}).rates_by_op().tolist() == [0, 0.02, 0, 0, 0, 0, 0.5]
    assert np.array_equal(M({"MeasX": 0.25, "PrepZ": 0.125}).rates_by_op(), NM.rates_by_op({"MeasX": 0.25, "PrepZ": 0.125}))
    with pytest.raises(ValueError, match=r"unknown noise-model location class\(es\): \['CX'\]"):
        M({"CX": 0.1})
    for bad in (1.0, -0.1, {"CNOT": 1.5}, float("nan"), {"IDLE": float("nan")}):
        with pytest.raises(ValueError, match=r"rates must be in \[0, 1\)"):
            M(bad)
    for bad in ("0.1", [0.1], True):
        with pytest.raises(ValueError, match="a number or a dict keyed by gate name"):
            M(bad)
    for bad in ((1, -1, 1), (1, float("nan"), 1), (1, float("inf"), 1)):
        with pytest.raises(ValueError, match="idle_weights must be finite and >= 0"):
            M(0.01, idle_weights=bad)
    with pytest.raises(ValueError, match="cnot_weights must be finite and >= 0"):
        M(0.01, cnot_weights=[1] * 14 + [-2])
    with pytest.raises(ValueError, match="idle_weights sum to 0"):
        M(0.01, idle_weights=(0, 0, 0))
    with pytest.raises(ValueError, match="cnot_weights sum to 0"):
        M(0.01, cnot_weights=np.zeros(15))
    with pytest.raises(ValueError, match="idle_weights needs 3 weights, got 2"):
        M(0.01, idle_weights=(1, 1))
    with pytest.raises(ValueError, match="cnot_weights needs 15 weights, got 16"):
        M(0.01, cnot_weights=np.ones(16))
    m = M(0.01, idle_weights=(1, 2, 5), cnot_weights=np.arange(15))
    ic, cc = m.cuts()
    assert ic.tolist() == NM.cuts([1, 2, 5]) and cc.tolist() == NM.cuts(np.arange(15)) and cc[0] == 0
    s, keep = m.as_struct()
    assert [s.rate[i] for i in range(7)] == [0] + [0.01] * 6 and [s.idle_w[i] for i in range(3)] == [1, 2, 5] and s.cnot_w[14] == 14
    s, keep = M(0.01).as_struct()
    assert not s.idle_w and not s.cnot_w                                    # NULL: the plain sampler's r % K


# ---------------------------------------------------------------------------------------- 3. the constructors
def test_constructors(N):
    M = N.NoiseModel
    p = 0.003
    u = M.uniform(p)
    assert u.rates_by_op().tolist() == [0] + [p] * 6 and u.idle_weights is None and u.cnot_weights is None
    s = M.si1000(p)
    assert s.rates_by_op().tolist() == [0, p, 2 * p, 2 * p, 5 * p, 5 * p, p / 10] and s.idle_weights is None and s.cnot_weights is None
    assert "SI1000" in M.si1000.__doc__
    b = M.biased(p, 10)
    assert b.rates_by_op().tolist() == [0] + [p] * 6 and b.idle_weights.tolist() == [1, 1, 20] and b.cnot_weights is None
    half = M.biased(p, 0.5)
    assert half.idle_weights.tolist() == [1, 1, 1] and half.cuts()[0].tolist() == [TOP // 3, 2 * TOP // 3]
    assert M.biased(p, 0).idle_weights.tolist() == [1, 1, 0]
    for bad in (-1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            M.biased(p, bad)
    with pytest.raises(ValueError):
        M.si1000(0.25)                                                      # measurements at 5p = 1.25


# ---------------------------------------------------------------------------------------- the matched probabilities, by enumerating every Pauli
def by_enumeration(model):
    """f64[n] per sector: every Pauli of every location with its own mass rate * w_i / sum(w), added to the column of its projection; and per sector
    the number of (location, projection) pairs that no column holds"""
    rate = model.rates_by_op()
    out, missing = [], []
    for is_x, (sig, cols) in enumerate(((SIG_Z, COLS_Z), (SIG_X, COLS_X))):
        index = {(frozenset(d), m): j for j, (d, m) in enumerate(cols)}
        probs = np.zeros(len(cols))
        shift = 0 if is_x else 2
        miss = set()
        for l, op in enumerate(OPS):
            a, b = (frozenset(sig[2 * l][0]), sig[2 * l][1]), (frozenset(sig[2 * l + 1][0]), sig[2 * l + 1][1])
            if op in (OP_IDLE, OP_CNOT):
                comps = IDLE_COMP if op == OP_IDLE else CNOT_COMP
                w = model.idle_weights if op == OP_IDLE else model.cnot_weights
                w = np.ones(len(comps)) if w is None else w
                paulis = [(int(c), rate[op] * w[i] / w.sum()) for i, c in enumerate(comps)]
            elif op in ((OP_MEAS_Z, OP_PREP_Z) if is_x else (OP_MEAS_X, OP_PREP_X)):
                paulis = [(1 << shift, rate[op])]
            else:
                continue
            for comp, mass in paulis:
                part = (comp >> shift) & 3
                proj = {0: None, 1: a, 2: b, 3: (a[0] ^ b[0], a[1] ^ b[1])}[part]
                if proj is None or not (proj[0] or proj[1]):
                    continue
                if proj in index:
                    probs[index[proj]] += mass
                else:
                    miss.add((l, part))
        out.append(probs)
        missing.append(len(miss))
    return out, tuple(missing)


def test_channel_probs_on_a_hand_made_circuit(N):
    rng = np.random.default_rng(3)
    cw = rng.random(15)
    cw[[2, 14]] = 0
    sigs = (sig_table(SIG_Z), sig_table(SIG_X))
    compiled, Lg = {"base_ops": np.array(OPS)}, np.zeros((1, 2))
    for model in (N.NoiseModel.uniform(0.01), N.NoiseModel.si1000(0.01), N.NoiseModel.biased(0.01, 10),
                  N.NoiseModel({"CNOT": 0.02, "MeasX": 0.05, "PrepZ": 0.0, "IDLE": 0.004}, idle_weights=(3, 0, 1), cnot_weights=cw)):
        pz, px, unmatched = model._channel_probs(compiled, Lg, Lg, matrices(), signatures=sigs)
        (wz, wx), missing = by_enumeration(model)
        assert unmatched == missing and pz.shape == (5,) and px.shape == (4,)
        assert np.allclose(pz, wz, rtol=1e-13, atol=0) and np.allclose(px, wx, rtol=1e-13, atol=0)
        assert pz[4] == 0.0                                                 # the column no location reaches has no mass ...
        lz, lx = model.prior_llrs(compiled, Lg, Lg, matrices(), signatures=sigs)
        floor_llr = float(np.log((1 - 1e-12) / 1e-12))
        assert lz[4] == floor_llr and np.isfinite(lz).all() and np.isfinite(lx).all()      # ... and keeps a large finite prior
        assert np.array_equal(lz[pz > 1e-12], np.log((1 - pz[pz > 1e-12]) / pz[pz > 1e-12]))
    # one location, by hand: IDLE at location 1 projects onto Z column ((1,), 1) with the weights of Y and Z, onto X column ((0,), 0) with those of X and Y
    m = N.NoiseModel({"IDLE": 0.008}, idle_weights=(1, 1, 6))
    assert m._projection_masses(OP_IDLE, False) == [0.008 * 7.0 / 8.0] and m._projection_masses(OP_IDLE, True) == [0.008 * 2.0 / 8.0]
    u = N.NoiseModel.uniform(0.005)
    assert u._projection_masses(OP_IDLE, False) == [0.005 * 2 / 3] and u._projection_masses(OP_CNOT, True) == [0.005 * 4 / 15] * 3      # the builder's expressions
    assert u._projection_masses(OP_MEAS_X, False) == [0.005] and u._projection_masses(OP_MEAS_X, True) == [] and u._projection_masses(OP_PREP_Z, True) == [0.005]


# ---------------------------------------------------------------------------------------- 4. run_simulation and run_weight_strata
def test_refused_combinations_raise_before_the_library_is_touched(L, N, monkeypatch):
    from qldpc_amd.simulation import engine, strata

    def no_gpu(*a, **k):
        raise AssertionError("GPU work started before the arguments were checked")
    monkeypatch.setattr(L, "Graph", no_gpu)
    monkeypatch.setattr(L, "lib", no_gpu)
    monkeypatch.setattr(engine, "_circuit_problem", no_gpu)
    model = N.NoiseModel.si1000(0.003)
    args = (None, None, None, None, 0.003)
    with pytest.raises(ValueError, match="noise_model=... does not go with correlated"):
        engine.run_simulation(*args, noise_model=model, correlated={})
    for aware in (True, False):
        with pytest.raises(ValueError, match="noise_model=... does not go with erasure"):
            engine.run_simulation(*args, noise_model=model, erasure={"rates": 0.01, "aware": aware})
    with pytest.raises(ValueError, match="noise_model must be a simulation.noise_model.NoiseModel"):
        engine.run_simulation(*args, noise_model={"CNOT": 0.01})
    with pytest.raises(ValueError, match="matched_priors must be True or False"):
        engine.run_simulation(*args, noise_model=model, matched_priors=1)
    with pytest.raises(ValueError, match="noise_model=... does not go with fixed-weight sampling"):
        strata.run_weight_strata(*args, weights=[1], noise_model=model)
    with pytest.raises(ValueError, match="decoder"):                        # the other rules still hold beside a model
        engine.run_simulation(*args, noise_model=model, decoder="bogus")
    r = engine._extension_rules(0, "f64", None, "flooding", None, None, "bp_osd", None, None, None, True, False, 50, None)
    assert r.noise_model is None and r.matched_priors is True              # no model: the rules of today


def test_binding_follows_the_header(L):
    assert "qldpc_circuit_plan_use_noise_model" in L.exports()
    getattr(L.lib(), "qldpc_circuit_plan_use_noise_model")
    assert L.lib().qldpc_version() == 101
    sig = L.signatures()["qldpc_circuit_plan_use_noise_model"][1]
    assert len(sig) == 2 and sig[1] == C.POINTER(L.NoiseModelStruct)
    assert C.sizeof(L.NoiseModelStruct) == 7 * 8 + 2 * C.sizeof(C.c_void_p)
    s = L.NoiseModelStruct()
    assert L.lib().qldpc_circuit_plan_use_noise_model(None, C.byref(s)) == -1 and b"plan is NULL" in L.lib().qldpc_last_error()
    assert hasattr(L.CircuitPlan, "use_noise_model")
    text = open(L.HEADER_PATH).read()
    assert "i = #{ j < K - 1 : r >= cut[j] }" in text and "cut[j] = (uint64) floor(ldexp(S_j / S_{K-1}, 32))" in text
    assert "out of scope" in text
