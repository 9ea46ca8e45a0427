"""The circuits of tests/circuit_shapes.py without a GPU: the table keeps the edges it was built for, the signature model equals the literal walk of
the same faults, and the draws of the sampler models -- on the model's signatures, at the parameters test_circuit_shapes_gpu.py compares the kernels
at -- reach every edge, so that a bit-for-bit comparison on the GPU means something.  The parameters are fixed here and imported there."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import circuit_shapes as CS  # noqa: E402
import erasure_model as EM  # noqa: E402
import fixed_weight_model as FM  # noqa: E402
import noise_model_model as NM  # noqa: E402
import soft_model as SM  # noqa: E402

NAMES = list(CS.SHAPES)

# ---- the parameters of the GPU comparisons.  Conditions on the models' own draws, not tolerances: the tests below assert what each is chosen for.
SEED = 20261021                       # one seed for every comparison
COUNT, BATCH = 96, 40                 # 96 trials in launches of 40 + 40 + 16: more than one launch, a ragged last one
BEGIN = 2 ** 32 - 40                  # the nonzero trial_begin: the 96 trials cross the 32-bit word of the Philox counter
P_LOW = 0.005                         # the rate of the bundled plans: most trials of the small shapes are fault free
# the rate at which most trials have faults and 96 trials turn every detector and logical bit and fire the last location (13 .. 3069 locations;
# a detector of the last round hangs on one preparation alone, so p * COUNT stays near 5 or above)
P_HIGH = {"c422": 0.2, "steane": 0.06, "shor": 0.05, "k64": 0.05, "hgp": 0.05}
W_ODD = {"c422": 6, "steane": 30, "shor": 30, "k64": 30, "hgp": 30}       # w % 4 = 2: the last Philox block of the Floyd draws is partial
W_BIG = {"hgp": 301}                  # above 256: lanes take a second list entry; 301 % 4 = 1
# a class at 0 (PrepX), one at a high rate (MeasX); PrepZ and MeasX, the classes of the last location, erased often enough to set the last herald bit
ERASURE_RATES = {"CNOT": 0.02, "PrepX": 0.0, "PrepZ": 0.25, "MeasX": 0.5, "MeasZ": 0.05, "IDLE": 0.1}
# a class at 0 (PrepX), two at 0.5 and above; the last location's classes (PrepZ, MeasX) fire in most trials
NOISE_RATES = {"CNOT": 0.05, "PrepX": 0.0, "PrepZ": 0.5, "MeasX": 0.6, "MeasZ": 0.1, "IDLE": 0.2}
NOISE_IDLE_W = (0.0, 1.0, 3.0)        # a zero first weight (cut 0 is 0), Z three times as likely as Y
NOISE_CNOT_W = np.random.default_rng(7).random(15)
NOISE_CNOT_W[[0, 1, 7, 14]] = 0.0     # the first two cuts are 0, the last Pauli is never drawn, the rest non-uniform
# the channels of tests/test_soft_gpu.py as (flip masses, keep masses): 8 levels, 3 levels with an empty flipped bin, 1 level
CHANNELS = {"gaussian": SM.gaussian_masses(0.5, 8), "three": ([0.02, 0.0, 0.005], [0.1, 0.3, 0.575]), "hard": ([0.02], [0.98])}
SOFT_COUNT = 192                      # flip rates of 0.02 .. 0.025: 192 trials flip the last measurement under every channel (launches of 40)


def weights(name):
    S = CS.shape(name)
    return [0, 1, W_ODD[name], S.n_locs] + ([W_BIG[name]] if name in W_BIG else [])


def cuts(which):
    return SM.cuts(*CHANNELS[which])


@functools.lru_cache(maxsize=None)
def models(name):
    """the four sampler models of a shape on the MODEL's signatures: (fixed weight, erasure, noise model, soft)"""
    S, (sz, sx) = CS.shape(name), CS.model_signatures(name)
    args = (sz, sx, np.asarray(S.compiled.base_ops), (S.nsx, S.nsz), S.k)
    return FM.CircuitModel(*args), EM.SamplerModel(*args), NM.SamplerModel(*args), SM.SamplerModel(*args)


@functools.lru_cache(maxsize=None)
def expected(name, what, arg=None):
    """what the GPU sampler must return, computed once: "fixed" (arg = w), "erasure", "noise", "soft" (arg = channel), "plain" (arg = p: the plain
    sampler through the soft model with no channel)"""
    fw, er, nm, so = models(name)
    if what == "fixed":
        return fw.sample(arg, SEED, BEGIN, COUNT)
    if what == "erasure":
        return er.sample(P_HIGH[name], ERASURE_RATES, SEED, 0, COUNT)
    if what == "noise":
        return nm.sample_model(NOISE_RATES, NOISE_IDLE_W, NOISE_CNOT_W, SEED, 0, COUNT)
    if what == "soft":
        return so.sample(P_HIGH[name], cuts(arg), SEED, 0, SOFT_COUNT)
    return so.sample(arg, None, SEED, BEGIN, COUNT)[:4]


@functools.lru_cache(maxsize=None)
def literal_samples(name, p, begin):
    """oracle.circuit_sample (the literal walk of the Philox draws) over COUNT trials -> (sparse_z, true_z, sparse_x, true_x) stacked"""
    from oracle import oracle as orc
    S = CS.shape(name)
    circ = orc.make_circuit(S.compiled, S.Lx, S.Lz)
    rows = [orc.circuit_sample(circ, p, SEED, begin + t) for t in range(COUNT)]
    return tuple(np.stack([r[i] for r in rows]) for i in range(4))


@functools.lru_cache(maxsize=None)
def dead_bits(name):
    """the (output, bit) pairs no fault can set: bits that no signature of the sector holds.  They are detectors of the last noiseless round, which
    repeats the round before it (test_the_table_keeps_its_edges pins that, and that each sector's last word keeps live bits)."""
    S, sigs = CS.shape(name), CS.model_signatures(name)
    dead = []
    for s, (ptr, idx, lm) in enumerate(sigs):
        live = np.zeros((S.nsx, S.nsz)[s], bool)
        live[idx.astype(np.int64)] = True
        dead += [(2 * s, int(b)) for b in np.flatnonzero(~live)]
        dead += [(2 * s + 1, r) for r in range(S.k) if not ((lm >> np.uint64(r)) & np.uint64(1)).any()]
    return frozenset(dead)


def uncovered(name, outs):
    """of (sparse_z, true_z, sparse_x, true_x) arrays -- one tuple or several, OR-ed -- the (output, bit) pairs that no trial sets although a fault can"""
    outs = outs if isinstance(outs, list) else [outs]
    never = [(i, int(b)) for i in range(4) for b in np.flatnonzero(~np.any([o[i].any(axis=0) for o in outs], axis=0))]
    return [x for x in never if x not in dead_bits(name)]


# ---------------------------------------------------------------------------------------- the table keeps its edges
def test_the_table_keeps_its_edges():
    S = {name: CS.shape(name) for name in NAMES}
    words = {name: ((s.nsx + 31) // 32, (s.nsz + 31) // 32) for name, s in S.items()}
    ops = {name: np.asarray(s.compiled.base_ops) for name, s in S.items()}
    assert set(NAMES) >= {"c422", "steane", "shor", "k64", "hgp"}
    for name, s in S.items():                                              # what every shape is: a circuit of the six gates the plan accepts
        assert set(np.unique(np.concatenate([ops[name], s.compiled.suffix_ops])).tolist()) <= {1, 2, 3, 4, 5, 6} and 1 <= s.k <= 64
        assert s.Lx.shape == s.Lz.shape == (s.k, s.cb.n) and s.n_locs == s.compiled.num_error_locs == len(s.cb.cycle) * s.cb.num_cycles
        assert not ((s.cb.Hz.astype(int) @ s.Lx.T) & 1).any() and not ((s.cb.Hx.astype(int) @ s.Lz.T) & 1).any()
        assert s.nsx == len(s.cb.Xchecks) * (s.cb.num_cycles + 2) and s.nsz == len(s.cb.Zchecks) * (s.cb.num_cycles + 2)
    c = S["c422"]
    assert c.cb.n == 4 and c.k == 2 and c.cb.num_cycles == 1
    assert c.n_locs < 32 and c.n_locs % 4 != 0
    assert c.nsx == c.nsz == 3                                             # one partial word per sector
    assert ops["c422"][-1] in (CS.OP_MEAS_X, CS.OP_MEAS_Z) and (c.n_locs - 1) // 4 == c.n_locs // 4      # a measurement inside a partial last Philox block
    s = S["steane"]
    assert s.cb.n == 7 and s.cb.num_cycles == 3 and s.k == 1 and s.n_locs % 32 != 0 and s.n_meas % 4 != 0
    s = S["shor"]
    assert s.cb.n == 9 and (len(s.cb.Xchecks), len(s.cb.Zchecks)) == (2, 6) and s.cb.num_cycles == 4 and s.k == 1
    assert s.nsx != s.nsz and words["shor"][0] != words["shor"][1] and sum(words["shor"]) % 2 == 1
    s = S["k64"]
    assert s.cb.n == 128 and s.k == 64 and s.cb.num_cycles == 1
    for sig in CS.model_signatures("k64"):
        assert (sig[2] >> np.uint64(63)).any()                             # some signature has logical bit 63, in each sector
    s = S["hgp"]
    assert s.nsx > 256 and s.nsz > 256 and s.nsx % 32 != 0 and s.nsz % 32 != 0 and s.nsx != s.nsz and sum(words["hgp"]) % 2 == 1
    assert s.n_locs > 1024 and s.n_locs % 4 != 0 and s.n_locs % 32 != 0
    for name, s in S.items():                                              # the bits no fault can set: detectors of the last round only, never a logical bit,
        nx, nz = len(s.cb.Xchecks), len(s.cb.Zchecks)                      # and the last word of each sector keeps bits that faults do set
        dead = dead_bits(name)
        assert all((i == 0 and b >= s.nsx - nx) or (i == 2 and b >= s.nsz - nz) for i, b in dead), name
        for i, nd, nc in ((0, s.nsx, nx), (2, s.nsz, nz)):
            assert nd % 32 == 0 or any((i, b) not in dead for b in range(nd - nd % 32, nd)), name      # (k64 has whole words only)
    # (the decoding-matrix widths n_z != n_x of shor and hgp need the builder, which runs on the GPU: test_circuit_shapes_gpu.py asserts them)
    for name in ("c422", "steane", "k64", "hgp"):                          # nothing here has circ72's arithmetic
        assert S[name].n_locs % 4 != 0 and S[name].n_locs % 32 != 0
    assert all(S[name].nsx % 32 != 0 and S[name].nsz % 32 != 0 for name in ("c422", "steane", "shor", "hgp"))


def test_the_builder_flag_moves_the_preparation():
    Hx = Hz = np.ones((1, 4), np.uint8)
    last, first = CS.CSSCircuit(Hx, Hz, 2, idle=2), CS.CSSCircuit(Hx, Hz, 2, idle=2, prep_z_first=True)
    assert last.cycle[-1][0] == "PrepZ" and first.cycle[0][0] == "PrepZ" and first.cycle[-1][0] == "MeasX"
    assert sorted(map(str, last.cycle)) == sorted(map(str, first.cycle)) and len(last.get_full_circuit()) == 2 * len(last.cycle)
    assert [g[0] for g in last.cycle].count("IDLE") == 2 and {g[0] for g in last.cycle} == {"CNOT", "PrepX", "PrepZ", "MeasX", "MeasZ", "IDLE"}


# ---------------------------------------------------------------------------------------- the signature model is right
@pytest.mark.parametrize("name", NAMES)
def test_the_signature_model_equals_the_literal_walk(name):
    """about 50 sets of 1 .. 8 distinct locations with random Paulis: the XOR of the model's signatures of the chosen components is what the
    literal walk of the circuit with exactly those faults inserted returns, syndromes and logical bits of both sectors (a walk of hgp, the
    largest, takes a millisecond: every shape has all 50 sets)"""
    S, sigs = CS.shape(name), CS.model_signatures(name)
    for ptr, idx, lm in sigs:
        assert ptr.shape == (2 * S.n_locs + 1,) and ptr.dtype == np.int32 and idx.dtype == np.uint16 and lm.shape == (2 * S.n_locs,) and lm.dtype == np.uint64
        assert ptr[0] == 0 and ptr[-1] == idx.size and (np.diff(ptr) >= 0).all()
        assert all((np.diff(idx[ptr[e]:ptr[e + 1]].astype(int)) > 0).all() for e in range(2 * S.n_locs))      # ascending inside an entry
        slot1 = np.arange(S.n_locs)[np.asarray(S.compiled.base_ops) != CS.OP_CNOT] * 2 + 1
        assert not np.diff(ptr)[slot1].any() and not lm[slot1].any()       # only a CNOT has a second slot
    sets = CS.random_fault_sets(S, 50, 11)
    seen = [set(), set()]
    for faults in sets:
        want = CS.literal_trial(S.compiled, S.Lx, S.Lz, faults)
        got = CS.xor_of_signatures(S, sigs, faults)
        for i, (a, b) in enumerate(zip(got, want)):
            assert np.array_equal(a, b), (name, faults, i)
        seen[0] |= {int(np.asarray(S.compiled.base_ops)[l]) for l, _ in faults}
        seen[1] |= {c for l, c in faults}
    assert S.n_locs - 1 in [l for l, _ in sets[0]] and max(len(f) for f in sets) == min(8, S.n_locs) and min(len(f) for f in sets) == 1
    assert seen[0] == set(np.unique(S.compiled.base_ops).tolist()) and seen[1] == set(range(15))      # every gate class, every Pauli choice


# ---------------------------------------------------------------------------------------- the draws reach the edges
def pad_words_fire(n_locs, thr, domain, begin, count):
    """does some word PAST the last location, in the last Philox block, fall below thr in some trial: then `l < n_locs` decides"""
    w = SM._words(4 * ((n_locs + 3) // 4), domain, SEED, begin, count)
    return bool((w[:, n_locs:] < np.uint64(thr)).any())


@pytest.mark.parametrize("name", NAMES)
def test_plain_draws_reach_the_edges(name):
    S = CS.shape(name)
    high, low = literal_samples(name, P_HIGH[name], BEGIN), literal_samples(name, P_LOW, 0)
    assert uncovered(name, high) == []                                           # every detector and logical bit of both sectors (bit 63 on k64)
    fired = EM._fires(np.full(S.n_locs, EM.threshold(P_HIGH[name])), EM.FAULT_DOMAIN, SEED, BEGIN, COUNT)
    assert fired[:, -1].any() and fired.any(axis=1).mean() > 0.5           # the last location fires; most trials have faults
    if S.n_locs % 4:
        assert pad_words_fire(S.n_locs, EM.threshold(P_HIGH[name]), EM.FAULT_DOMAIN, BEGIN, COUNT)
    assert any(x.any() for x in low)                                       # the small rate is not nothing
    for got, p, begin in ((high, P_HIGH[name], BEGIN), (low, P_LOW, 0)):   # the model's plain sampler, on the model's signatures, is the literal walk
        for a, b in zip(expected(name, "plain", p) if begin else models(name)[3].sample(p, None, SEED, 0, COUNT)[:4], got):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("name", NAMES)
def test_fixed_weight_draws_reach_the_edges(name):
    S = CS.shape(name)
    ws = weights(name)
    assert ws[0] == 0 and ws[1] == 1 and ws[2] % 4 != 0 and 1 < ws[2] < S.n_locs and ws[3] == S.n_locs and all(w > 256 for w in ws[4:])
    outs = [expected(name, "fixed", w) for w in ws]
    assert uncovered(name, outs[1:]) == []
    assert not any(x.any() for x in outs[0])
    w = max(w for w in ws if w < S.n_locs)                                 # the last location is a member in some trial below w = N too
    assert (FM.floyd_sets(S.n_locs, w, SEED, BEGIN, COUNT) == S.n_locs - 1).any(), w


@pytest.mark.parametrize("name", NAMES)
def test_erasure_draws_reach_the_edges(name):
    S = CS.shape(name)
    *out, erased = expected(name, "erasure")
    assert uncovered(name, tuple(out)) == []
    assert erased[:, -1].any()                                             # the last herald bit
    by_op, ty = EM.rates_by_op(ERASURE_RATES), np.asarray(S.compiled.base_ops)
    assert by_op.min() >= 0 and (by_op[1:] == 0).sum() == 1 and by_op.max() >= 0.5
    for op in np.unique(ty):
        assert bool(erased[:, ty == op].any()) == (by_op[op] > 0), op
    if S.n_locs % 32:
        assert EM.pack_heralds(erased)[:, -1].max() < (1 << (S.n_locs % 32))      # the partial last word holds nothing above the last location
    if S.n_locs % 4:
        assert pad_words_fire(S.n_locs, EM.threshold(by_op.max()), EM.ERASE_DOMAIN, 0, COUNT)


@pytest.mark.parametrize("name", NAMES)
def test_noise_model_draws_reach_the_edges(name):
    S = CS.shape(name)
    out, (b, l, idx) = expected(name, "noise")
    assert uncovered(name, out) == []
    assert (l == S.n_locs - 1).any()
    by_op, ty = NM.rates_by_op(NOISE_RATES), np.asarray(S.compiled.base_ops)[l]
    assert (by_op[1:] == 0).sum() == 1 and (by_op >= 0.5).sum() >= 1
    for op in np.unique(S.compiled.base_ops):
        assert bool((ty == op).any()) == (by_op[op] > 0), op
    assert 0.0 in NOISE_IDLE_W and (NOISE_CNOT_W == 0).sum() == 4 and len(set(NOISE_CNOT_W.tolist())) == 12
    assert NM.cuts(NOISE_IDLE_W)[0] == 0 and NM.cuts(NOISE_CNOT_W)[:2] == [0, 0]                       # zero cuts in both tables
    if (ty == CS.OP_IDLE).any():
        assert set(idx[ty == CS.OP_IDLE].tolist()) == {1, 2}
    assert set(idx[ty == CS.OP_CNOT].tolist()) <= set(np.flatnonzero(NOISE_CNOT_W).tolist()) and len(set(idx[ty == CS.OP_CNOT].tolist())) >= 8
    if S.n_locs % 4:                                                       # a pad lane draws below the largest class threshold: the zero padding decides
        assert pad_words_fire(S.n_locs, EM.threshold(by_op.max()), EM.FAULT_DOMAIN, 0, COUNT)


@pytest.mark.parametrize("name", NAMES)
def test_soft_draws_reach_the_edges(name):
    S = CS.shape(name)
    so = models(name)[3]
    assert so.meas.size == S.n_meas
    for which in CHANNELS:
        *out, levels, flipped = expected(name, "soft", which)
        cut = cuts(which)
        K = len(cut) // 2
        assert levels.shape == (SOFT_COUNT, S.n_meas) and flipped[:, -1].any(), which      # the last measurement's readout flips
        assert uncovered(name, tuple(out)) == []
        w = np.diff([0] + cut)
        assert set(np.unique(levels).tolist()) == {k for k in range(K) if w[k] + w[K + k] > 0}
    assert [len(cuts(c)) // 2 for c in ("gaussian", "three", "hard")] == [8, 3, 1]


# ---------------------------------------------------------------------------------------- the builder counts each sector's detectors
@pytest.mark.parametrize("name", ["shor", "hgp"])
def test_the_builder_counts_each_sectors_detectors(name, monkeypatch):
    """build_decoding_matrices on circuits whose sectors differ in size, with the device step (the fault signatures) replaced by the model: the
    host code around it gives sector Z the X checks' detectors and sector X the Z checks', and the widths n_z != n_x the aware paths stride by"""
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    from qldpc_amd.noise.builder import build_decoding_matrices
    monkeypatch.setattr(_lib, "circuit_fault_signatures", lambda comp, Lx, Lz, x: CS.signatures_model(comp, Lx, Lz, bool(x)))
    S = CS.shape(name)
    M = build_decoding_matrices(S.cb, S.Lx, S.Lz, P_LOW, verbose=False)
    assert M["HdecZ"].shape[0] == S.nsx == M["first_logical_rowZ"] and M["HdecX"].shape[0] == S.nsz == M["first_logical_rowX"] and S.nsx != S.nsz
    assert M["HZ_full"].shape == (S.nsx + S.k, M["HdecZ"].shape[1]) and M["HX_full"].shape == (S.nsz + S.k, M["HdecX"].shape[1])
    assert M["HdecZ"].shape[1] != M["HdecX"].shape[1] and M["k"] == S.k and M["num_cycles"] == S.cb.num_cycles
    for nm, sig, rows in (("Z", CS.model_signatures(name)[0], S.nsx), ("X", CS.model_signatures(name)[1], S.nsz)):
        H, probs = np.asarray(M[f"H{nm}_full"]), np.asarray(M[f"channel_probs{nm}"])
        assert probs.shape == (H.shape[1],) and (probs > 0).all() and len({c.tobytes() for c in H.T}) == H.shape[1]      # merged: no two equal columns
        dets = np.zeros(rows, bool)
        dets[sig[1].astype(np.int64)] = True
        assert np.array_equal(H[:rows].any(axis=1), dets)                  # a row has a one exactly where some signature holds its detector
        assert H[rows:].any(axis=1).all()                                  # every logical row is reached


def test_the_builder_row_count_of_a_bb_circuit_is_the_old_one():
    """n / 2 checks of each kind and num_cycles + 2 rounds: the per-sector count equals the n2 * (num_cycles + 2) the builder used for both"""
    import qldpc_amd  # noqa: F401
    from qldpc_amd.codes.bb_code import BBCodeCircuit
    from qldpc_amd.data import load_code
    from qldpc_amd.noise.compiled import CompiledCircuit
    c = load_code("bb72")
    cb = BBCodeCircuit(c["Hx"], c["Hz"], num_cycles=6, ell=c["ell"], m=c["m_dim"], a_x_powers=c["a_x_powers"], a_y_powers=c["a_y_powers"],
                       b_y_powers=c["b_y_powers"], b_x_powers=c["b_x_powers"])
    comp = CompiledCircuit(cb.get_full_circuit(), cb.cycle * 2, cb.lin_order, cb.data_qubits, cb.Xchecks, cb.Zchecks)
    assert int(comp.x_syn_ptrs[-1]) == int(comp.z_syn_ptrs[-1]) == cb.n2 * (cb.num_cycles + 2) == 288
