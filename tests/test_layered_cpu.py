"""CPU suite of the layered-schedule decoder: the greedy colouring on the bundled matrices, the numpy model (tests/layered_model.py) against an
independently written scalar serial loop, the property that licenses the kernel's parallelism (the order of the rows inside a layer cannot change
a bit), the degree-1 / non-finite rules, and the Python-side argument checks, which sit before any device call."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layered_model as LM  # noqa: E402

# layer sizes of the greedy colouring (rows without entries count in layer 0)
SIZES = {
    ("circ72", "Z"): [54, 18, 18, 18] + [9] * 20,
    ("circ72", "X"): [57, 27, 24, 24] + [18] * 6 + [12, 12, 9, 9, 3, 3],
    ("circ144", "Z"): [147, 75, 72, 72, 75, 75, 72, 72, 66, 66, 63, 63, 21, 21, 18, 18, 3, 3, 3, 3],
    ("circ144", "X"): [144, 84, 78, 78] + [63] * 4 + [54, 54] + [48] * 4 + [18] * 4,
}


def sector(tag, s):
    import qldpc_amd  # noqa: F401
    from qldpc_amd.data import load_circuit_matrices
    from qldpc_amd.simulation.engine import prior_llrs
    d = load_circuit_matrices(tag)
    return d[f"Hdec{s}_indptr"], d[f"Hdec{s}_indices"], int(d[f"Hdec{s}_shape"][1]), prior_llrs(np.asarray(d[f"channel_probs{s}"], np.float64))


def serial_decode(indptr, indices, n, prior, s, order, max_iter, alphas, clip):
    """The literal serial schedule in plain Python floats: the rows of `order` one after the other, every step of the header's list spelled out."""
    m = len(indptr) - 1
    V = [float(x) for x in prior]
    R = [0.0] * len(indices)
    for k in range(max_iter):
        a = float(alphas[k])
        for i in order:
            lo, hi = int(indptr[i]), int(indptr[i + 1])
            if hi == lo:
                continue
            Q, sign_prod = [], -1.0 if s[i] else 1.0
            for e in range(lo, hi):
                q = V[indices[e]] - R[e]
                if q != q:
                    q = 0.0
                if q > clip:
                    q = clip
                if q < -clip:
                    q = -clip
                Q.append(q)
                sign_prod = sign_prod * (1.0 if q >= 0 else -1.0)
            min1 = min2 = math.inf
            pos = -1
            for t, q in enumerate(Q):
                if abs(q) < min1:
                    min2, min1, pos = min1, abs(q), t
                elif abs(q) < min2:
                    min2 = abs(q)
            for t, q in enumerate(Q):
                r = a * (sign_prod * (1.0 if q >= 0 else -1.0)) * (min2 if t == pos else min1)
                R[lo + t] = r
                V[indices[lo + t]] = q + r
        e = [1 if v < 0 else 0 for v in V]
        if all((sum(e[indices[x]] for x in range(indptr[i], indptr[i + 1])) & 1) == (s[i] & 1) for i in range(m)):
            return np.array(e, np.int8), 1, np.array(V), k
    return np.array([1 if v < 0 else 0 for v in V], np.int8), 0, np.array(V), max_iter - 1


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


@pytest.mark.parametrize("tag,s", sorted(SIZES))
def test_check_layers_on_the_bundled_matrices(tag, s):
    from qldpc_amd.decoding.layered import check_layers, layer_count
    ip, ix, n, _ = sector(tag, s)
    lay = check_layers((ip, ix, n))
    assert lay.dtype == np.int32 and lay.shape == (len(ip) - 1,) and lay.min() == 0
    assert LM.layers_valid(ip, ix, n, lay)                                     # no shared column inside a layer
    assert np.bincount(lay).tolist() == SIZES[(tag, s)]
    assert np.array_equal(lay, check_layers((ip, ix, n)))                      # deterministic
    assert np.array_equal(lay, LM.greedy_layers(ip, ix, n))                    # the model's own statement of the rule
    assert layer_count((ip, ix, n), lay) == len(SIZES[(tag, s)]) == len(LM.LayeredModel(ip, ix, n, np.ones(n)).stages)
    assert np.all(lay[np.diff(ip) == 0] == 0)                                  # rows without entries: layer 0


def _golden_syndromes(golden, tag, s, count):
    return golden(f"{tag}_decode")[f"{s}_syndromes"][:count].astype(np.int8)


@pytest.mark.parametrize("s", ["Z", "X"])
def test_one_row_per_layer_is_the_serial_loop(golden, s):
    ip, ix, n, prior = sector("circ72", s)
    m = len(ip) - 1
    synd = _golden_syndromes(golden, "circ72", s, 2)
    priors = [prior]
    if s == "X":                                                               # non-finite priors are allowed, as in the plain decoder
        odd = prior.copy()
        odd[3], odd[40], odd[77], odd[200] = np.inf, -np.inf, np.nan, -0.0
        priors.append(odd)
    for pr in priors:
        model = LM.LayeredModel(ip, ix, n, pr, row_layer=np.arange(m))
        assert model.layer_sizes() == [1] * int((np.diff(ip) > 0).sum())
        got = model.decode(synd, max_iter=6)
        for b in range(len(synd)):
            want = serial_decode(ip, ix, n, pr, synd[b], range(m), 6, LM.alpha_table(6, "dynamical", 1.0), 20.0)
            assert same([g[b] for g in got], want), (s, b)


@pytest.mark.parametrize("s", ["Z", "X"])
def test_order_inside_a_layer_cannot_change_a_bit(golden, s):
    ip, ix, n, prior = sector("circ72", s)
    synd = _golden_syndromes(golden, "circ72", s, 2)
    model = LM.LayeredModel(ip, ix, n, prior)
    got = model.decode(synd, max_iter=5, alpha_mode="const", alpha=0.8)
    rng = np.random.default_rng(5)
    for trial in range(2):
        order = []
        for lay in np.unique(model.row_layer):
            rows = np.flatnonzero(model.row_layer == lay)
            order += rng.permutation(rows).tolist() if trial else rows.tolist()
        for b in range(len(synd)):
            want = serial_decode(ip, ix, n, prior, synd[b], order, 5, np.full(5, 0.8), 20.0)
            assert same([g[b] for g in got], want), (s, trial, b)


@pytest.mark.parametrize("tag", ["circ72", "circ144"])
def test_converged_results_satisfy_the_syndrome(golden, tag):
    for s in "ZX":
        ip, ix, n, prior = sector(tag, s)
        model = LM.LayeredModel(ip, ix, n, prior)
        light = np.zeros((4, n), np.int8)                                      # two faults each: these converge
        for b, cols in enumerate(np.random.default_rng(3).choice(np.flatnonzero(np.bincount(ix, minlength=n)), (4, 2), replace=False)):
            light[b, cols] = 1
        synd = np.concatenate([_golden_syndromes(golden, tag, s, 8), model.syndrome_of(light)])
        err, conv, llr, it = model.decode(synd, max_iter=50)
        print(tag, s, "converged", int(conv.sum()), "of", len(synd), "iterations", (it + 1).tolist())
        assert conv.any()
        assert np.array_equal(model.syndrome_of(err)[conv == 1], synd[conv == 1] & 1)
        assert np.all(it[conv == 0] == 49) and np.array_equal(err, (llr < 0).astype(np.int8))


@pytest.mark.parametrize("tag", ["circ72", "circ144"])
def test_degree_one_checks_follow_the_rules(golden, tag):
    """A degree-1 check has min2 = +inf, so its message is +-inf by the syndrome sign and it leaves its column's posterior at +-inf.  The column's
    other check then reads Q = +-inf clipped to +-clip_llr, and the next pass of the degree-1 check reads Q = finite - (+-inf), clipped, so no NaN
    arises.  With the degree-1 checks moved to a last layer of their own (a caller's valid layering) every iteration ends with those posteriors at
    +-inf; a NaN prior there becomes Q = 0.0 in the first pass."""
    ip, ix, n, prior = sector(tag, "X")
    deg = np.diff(ip)
    rows1 = np.flatnonzero(deg == 1)
    assert rows1.size > 0
    cols1 = ix[ip[rows1]]
    assert len(set(cols1.tolist())) == rows1.size                              # on distinct columns
    synd = _golden_syndromes(golden, tag, "X", 3)
    lay = LM.greedy_layers(ip, ix, n)
    lay[rows1] = lay.max() + 1
    assert LM.layers_valid(ip, ix, n, lay)
    model = LM.LayeredModel(ip, ix, n, prior, row_layer=lay)
    other = np.setdiff1d(np.arange(n), cols1)
    want = np.where(synd[:, rows1] & 1, -np.inf, np.inf)
    for max_iter in (1, 2, 7):
        err, conv, llr, it = model.decode(synd, max_iter=max_iter)
        assert not np.isnan(llr).any()
        assert np.array_equal(llr[:, cols1], want)
        assert np.array_equal(err[:, cols1], synd[:, rows1] & 1)
        assert np.isfinite(llr[:, other]).all()
    odd = prior.copy()
    odd[cols1[0]] = np.nan
    llr2 = LM.LayeredModel(ip, ix, n, odd, row_layer=lay).decode(synd, max_iter=2)[2]
    assert np.array_equal(llr2[:, cols1], want) and not np.isnan(llr2).any()
    # with the greedy layers the column's other check runs after the degree-1 check: the posterior it leaves is finite, within 2 clip_llr
    llr3 = LM.LayeredModel(ip, ix, n, prior).decode(synd, max_iter=3)[2]
    assert not np.isnan(llr3).any() and np.abs(llr3[np.isfinite(llr3)]).max() <= 40.0


def test_a_column_with_only_a_degree_one_check():
    """Q = inf - inf = NaN becomes 0.0 (sign +), the message is +-inf by the syndrome sign again: the posterior stays +-inf, never NaN."""
    ip, ix, n = np.array([0, 1, 3, 6]), np.array([0, 1, 2, 1, 2, 3]), 4
    prior = np.array([2.0, 1.5, 1.25, 3.0])
    synd = np.array([[1, 0, 0], [0, 1, 0], [1, 1, 1]], np.int8)
    model = LM.LayeredModel(ip, ix, n, prior)
    assert model.row_layer.tolist() == [0, 0, 1]
    for max_iter in (1, 2, 5):
        got = model.decode(synd, max_iter=max_iter)
        assert np.array_equal(got[2][:, 0], np.where(synd[:, 0] & 1, -np.inf, np.inf)) and not np.isnan(got[2]).any()
        for b in range(len(synd)):
            want = serial_decode(ip, ix, n, prior, synd[b], range(3), max_iter, LM.alpha_table(max_iter, "dynamical", 1.0), 20.0)
            assert same([g[b] for g in got], want)


def test_alpha_modes_max_iter_one_and_the_zero_syndrome(golden):
    ip, ix, n, prior = sector("circ72", "Z")
    prior = np.maximum(prior, 1.0)                                             # (the packaged prior has one entry <= 0)
    m = len(ip) - 1
    synd = np.concatenate([_golden_syndromes(golden, "circ72", "Z", 2), np.zeros((1, m), np.int8)])
    model = LM.LayeredModel(ip, ix, n, prior)
    assert (prior > 0).all()
    for mode, alpha in (("dynamical", 1.0), ("const", 0.75), ("seq", [0.5, 0.625, 0.9])):
        for max_iter in (1, 4):
            err, conv, llr, it = model.decode(synd, max_iter=max_iter, alpha_mode=mode, alpha=alpha)
            assert conv[-1] == 1 and it[-1] == 0 and not err[-1].any()         # zero syndrome: converged at iteration 0 with e = 0
            assert np.all(it[conv == 0] == max_iter - 1)
            b = 0
            want = serial_decode(ip, ix, n, prior, synd[b], np.argsort(model.row_layer, kind="stable"), max_iter, LM.alpha_table(max_iter, mode, alpha), 20.0)
            assert same([g[b] for g in (err, conv, llr, it)], want), (mode, max_iter)
    a = model.decode(synd[:1], max_iter=3, clip_llr=20.0)
    c = model.decode(synd[:1], max_iter=3, clip_llr=2.5)
    assert not np.array_equal(a[2], c[2]) and np.abs(c[2]).max() <= 2.5 + 2.5   # the clip enters: |V| <= |Q| + |R| <= 2 clip


def test_python_argument_checks():
    from qldpc_amd.decoding.layered import LayeredMinSumDecoder, validate_layers
    ip, ix, n, prior = sector("circ72", "Z")
    m = len(ip) - 1
    H = (ip, ix, n)
    with pytest.raises(ValueError, match="max_iter >= 1, got 0"):
        LayeredMinSumDecoder(H, prior, maxIter=0)
    with pytest.raises(ValueError, match="clip_llr must be > 0, got -1.0"):
        LayeredMinSumDecoder(H, prior, clip_llr=-1.0)
    with pytest.raises(ValueError, match="clip_llr must be > 0, got nan"):
        LayeredMinSumDecoder(H, prior, clip_llr=float("nan"))
    with pytest.raises(ValueError, match=f"prior has {n - 1} entries"):
        LayeredMinSumDecoder(H, prior[:-1])
    with pytest.raises(ValueError, match="Unsupported alpha_mode"):
        LayeredMinSumDecoder(H, prior, alpha_mode="bogus")
    with pytest.raises(ValueError, match=f"H has {m} rows"):
        LayeredMinSumDecoder(H, prior, layers=np.zeros(m - 1, np.int32))
    neg = np.arange(m)
    neg[5] = -2
    with pytest.raises(ValueError, match=r"layers\[5\] = -2"):
        LayeredMinSumDecoder(H, prior, layers=neg)
    with pytest.raises(ValueError, match="integers"):
        LayeredMinSumDecoder(H, prior, layers=np.arange(m) + 0.5)
    # rows a < b that share a column, put into one layer: both are named
    shares = np.flatnonzero(np.bincount(ix, minlength=n) >= 2)[0]
    a, b = [i for i in range(m) if shares in ix[ip[i]:ip[i + 1]]][:2]
    lay = np.arange(m)
    lay[b] = lay[a]
    with pytest.raises(ValueError, match=f"rows {a} and {b} are both in layer {a}"):
        LayeredMinSumDecoder(H, prior, layers=lay)
    assert np.array_equal(validate_layers(H, np.arange(m)), np.arange(m))


def test_run_simulation_argument_rules():
    import qldpc_amd  # noqa: F401
    from qldpc_amd.data import load_code
    from qldpc_amd.simulation.engine import run_simulation
    c = load_code("bb72")
    args = (c["Hx"], c["Hz"], c["Lx"], c["Lz"], 0.005)
    for kw, match in ((dict(schedule="serial"), "Unsupported schedule"),
                      (dict(schedule="layered", decoder="relay_bp"), "relay_bp"),
                      (dict(schedule="layered", window=(4, 2)), "window"),
                      (dict(schedule="layered", alpha_mode="alvarado"), "alpha estimator"),
                      (dict(schedule="layered", use_dynamic_alpha=False), "alpha estimator"),
                      (dict(schedule="layered", alpha_mode="alvarado-autoregressive"), "alpha estimator"),
                      (dict(schedule="layered", scopt=True), "SCOPT"),
                      (dict(schedule="layered", osd_order=2), "OSD-w"),
                      (dict(schedule="layered", maxIter=0), "max_iter >= 1"),
                      (dict(schedule="layered", layers=np.zeros(4)), "pair"),
                      (dict(layers=(None, None)), "schedule='layered'")):
        with pytest.raises(ValueError, match=match):
            run_simulation(*args, num_trials=10, **kw)
