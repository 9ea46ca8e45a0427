"""CPU suite of the single-precision min-sum decoder: the numpy model (tests/minsum32_model.py) against an independently written scalar loop over
np.float32 scalars, the anchor to the reference-pinned f64 decoder on inputs where no f32 operation rounds, the run_simulation argument rules (which
sit before any device call) and the header signatures of the new entry points."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import minsum32_model as MM  # noqa: E402

F = np.float32
MODES = (("dynamical", 1.0), ("const", 0.8125), ("seq", [0.5, 0.625, 0.75, 0.9]))


def sector(tag, s):
    import qldpc_amd  # noqa: F401
    from qldpc_amd.data import load_circuit_matrices
    from qldpc_amd.simulation.engine import prior_llrs
    d = load_circuit_matrices(tag)
    return d[f"Hdec{s}_indptr"], d[f"Hdec{s}_indices"], int(d[f"Hdec{s}_shape"][1]), prior_llrs(np.asarray(d[f"channel_probs{s}"], np.float64))


def scalar_decode(indptr, indices, n, prior, s, max_iter, alphas32, clip):
    """The header's list, one np.float32 scalar operation at a time: the reference's loop (rows ascending, scatter-add in row order) in f32."""
    m = len(indptr) - 1
    indptr, indices = [int(x) for x in indptr], [int(x) for x in indices]
    with np.errstate(over="ignore"):
        prior32 = [F(np.float64(x)) for x in prior]
    clip = F(clip)
    Q = [prior32[j] for j in indices]
    R = [F(0.0)] * len(indices)
    V = list(prior32)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(max_iter):
            a = alphas32[k]
            assert type(a) is F
            rsum = [F(0.0)] * n
            for i in range(m):
                lo, hi = indptr[i], indptr[i + 1]
                if lo == hi:
                    continue
                neg_total = bool(s[i] & 1)
                min1 = min2 = F(np.inf)
                pos = -1
                for e in range(lo, hi):
                    if not Q[e] >= 0:
                        neg_total = not neg_total
                    ab = abs(Q[e])
                    if ab < min1:
                        min2, min1, pos = min1, ab, e
                    elif ab < min2:
                        min2 = ab
                for e in range(lo, hi):
                    am = a * (min2 if e == pos else min1)
                    assert type(am) is F
                    r = -am if neg_total != (not Q[e] >= 0) else am
                    R[e] = r
                    rsum[indices[e]] = rsum[indices[e]] + r
            V = [rsum[j] + prior32[j] for j in range(n)]
            for e in range(len(indices)):
                q = V[indices[e]] - R[e]
                assert type(q) is F
                if q != q:
                    q = F(0.0)
                elif q > clip:
                    q = clip
                elif q < -clip:
                    q = -clip
                Q[e] = q
            e_hat = [1 if v < 0 else 0 for v in V]
            if all((sum(e_hat[indices[x]] for x in range(indptr[i], indptr[i + 1])) & 1) == (s[i] & 1) for i in range(m)):
                return np.array(e_hat, np.int8), 1, np.array(V, np.float64), k
    return np.array([1 if v < 0 else 0 for v in V], np.int8), 0, np.array(V, np.float64), max_iter - 1


def same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def check_against_scalar(ip, ix, n, prior, synd, max_iter, mode, alpha, clip=20.0, what=""):
    model = MM.Minsum32Model(ip, ix, n, prior)
    got = model.decode(synd, max_iter=max_iter, alpha_mode=mode, alpha=alpha, clip_llr=clip)
    assert got[2].dtype == np.float64 and got[0].dtype == np.int8
    al = MM.alpha_table32(max_iter, mode, alpha)
    for b in range(len(synd)):
        want = scalar_decode(ip, ix, n, prior, synd[b], max_iter, al, clip)
        assert same([g[b] for g in got], want), (what, mode, max_iter, b)
    return got


def test_model_is_the_scalar_loop_on_steane_and_bb72(golden):
    f = golden("steane_minsum")
    for mode, alpha in MODES:
        for max_iter in (1, 50):
            for prior in (f["prior"], f["prior2"]):
                check_against_scalar(f["indptr"], f["indices"], int(f["n"]), prior, f["syndromes"], max_iter, mode, alpha, what="steane")
    f = golden("bb72_minsum")
    ip, ix, n = f["Hx_indptr"], f["Hx_indices"], int(f["Hx_shape"][1])
    conv = 0
    for mode, alpha in MODES:
        for max_iter in (1, 50):
            got = check_against_scalar(ip, ix, n, f["Hx_p030_prior"], f["Hx_p030_syndromes"][:16], max_iter, mode, alpha, what="bb72")
            conv += int(got[1].sum())
    assert conv > 0


@pytest.mark.parametrize("s", ["Z", "X"])
def test_model_is_the_scalar_loop_on_circ72(golden, s):
    ip, ix, n, prior = sector("circ72", s)
    synd = golden("circ72_decode")[f"{s}_syndromes"].astype(np.int8)
    for mode, alpha in MODES:
        check_against_scalar(ip, ix, n, prior, synd[:2], 1, mode, alpha, what=f"circ72 {s}")
        got = check_against_scalar(ip, ix, n, prior, synd[:1], 50, mode, alpha, what=f"circ72 {s}")
        if s == "X":                                                           # degree-1 checks: min2 = +inf, the posterior of their column is +-inf
            assert np.isinf(got[2]).any() and np.diff(ip).min() <= 1
    got = check_against_scalar(ip, ix, n, prior, synd[1:3], 50, "dynamical", 1.0, what=f"circ72 {s}")
    assert np.all(got[3][got[1] == 0] == 49)


def test_nan_and_subnormal_priors(golden):
    ip, ix, n, prior = sector("circ72", "X")
    synd = golden("circ72_decode")["X_syndromes"][:1].astype(np.int8)
    odd = prior.copy()
    odd[3], odd[40], odd[77], odd[200] = np.inf, -np.inf, np.nan, -0.0
    got = check_against_scalar(ip, ix, n, odd, synd, 6, "dynamical", 1.0, what="non-finite prior")
    assert np.isnan(got[2][:, 77]).all() and np.isinf(got[2][:, 3]).all()     # V = s + NaN stays NaN; the messages into the column's checks do not
    tiny = prior.copy()
    tiny[5], tiny[6] = 1e-40, -1e-40                                           # f32 subnormals: kept, not flushed
    assert 0 < float(F(1e-40)) < float(np.finfo(F).tiny)
    got = check_against_scalar(ip, ix, n, tiny, synd, 6, "const", 0.5, what="subnormal prior")
    # a tiny model whose second iteration multiplies a subnormal: alpha * min1 stays subnormal
    ip2, ix2 = np.array([0, 2, 4]), np.array([0, 1, 1, 2])
    got = check_against_scalar(ip2, ix2, 3, np.array([1e-40, 3e-40, -2e-39]), np.array([[1, 0], [0, 1]], np.int8), 3, "const", 0.5, what="all subnormal")
    assert np.all(got[2] != 0) and np.all(np.abs(got[2]) < float(np.finfo(F).tiny))        # every posterior is a non-zero f32 subnormal


@pytest.mark.parametrize("s", ["Z", "X"])
def test_anchor_to_the_f64_oracle_where_no_f32_operation_rounds(oracle, golden, s):
    """priors +-(1..32)/4, alpha 0.5, clip 20, 12 iterations: every value is a multiple of 2^-14 below 2^7, so every f32 operation is exact and the f32
    model must equal the reference-pinned f64 min-sum bit for bit (err, conv, final_iter, llr after widening)."""
    ip, ix, n, _ = sector("circ72", s)
    synd = golden("circ72_decode")[f"{s}_syndromes"].astype(np.int8)
    rng = np.random.default_rng(72)
    prior = rng.integers(1, 33, n) * 0.25 * rng.choice([-1.0, 1.0], n)
    got = MM.Minsum32Model(ip, ix, n, prior).decode(synd, max_iter=12, alpha_mode="const", alpha=0.5, clip_llr=20.0)
    want = oracle.minsum_decode_batch(ip, ix, n, synd, prior, max_iter=12, alpha=0.5, alpha_mode="alvarado", clip_llr=20.0)
    for name, a, b in zip(("err", "conv", "llr", "final_iter"), got, want):
        assert np.array_equal(a, b, equal_nan=True), (s, name)


def test_run_simulation_precision_rules():
    import qldpc_amd  # noqa: F401
    from qldpc_amd.data import load_code
    from qldpc_amd.simulation.engine import run_simulation
    c = load_code("bb72")
    args = (c["Hx"], c["Hz"], c["Lx"], c["Lz"], 0.005)
    for kw, match in ((dict(precision="f16"), "Unsupported precision"),
                      (dict(precision="f32", decoder="relay_bp"), "relay_bp"),
                      (dict(precision="f32", window=(4, 2)), "window"),
                      (dict(precision="f32", schedule="layered"), "layered"),
                      (dict(precision="f32", decimation={}), "decimation"),
                      (dict(precision="f32", osd_order=2), "OSD-w"),
                      (dict(precision="f32", maxIter=0), "max_iter >= 1")):
        with pytest.raises(ValueError, match=match):
            run_simulation(*args, num_trials=10, **kw)


def test_python_argument_checks_and_header_signatures():
    import ctypes as C
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    with pytest.raises(ValueError, match="max_iter >= 1, got 0"):
        _lib.check_minsum32_args(0, 20.0)
    for clip in (0.0, -1.0, float("nan"), float("inf"), 1e39, 1e-50):           # 1e39 rounds to inf and 1e-50 to 0 in f32
        with pytest.raises(ValueError, match="clip_llr"):
            _lib.check_minsum32_args(5, clip)
    assert _lib.check_minsum32_args(5, 6.5) == (5, 6.5)
    sig = _lib.signatures()
    names = ("qldpc_minsum32_decoder_create", "qldpc_minsum32_decoder_destroy", "qldpc_minsum32_decoder_info", "qldpc_minsum32_decode_batch",
             "qldpc_minsum32_decode_batch_dev", "qldpc_circuit_plan_use_f32")
    for name in names:
        assert name in sig, name
    assert [len(sig[k][1]) for k in names] == [10, 1, 5, 7, 8, 1]
    assert sig["qldpc_minsum32_decoder_create"][1][1] == C.POINTER(C.c_double) and sig["qldpc_minsum32_decoder_create"][1][7] is C.c_double
    assert sig["qldpc_minsum32_decoder_destroy"][0] is None and sig["qldpc_minsum32_decode_batch"][0] is C.c_int
    assert sig["qldpc_minsum32_decode_batch"][1][4] == C.POINTER(C.c_double)          # llr is f64: the f32 posteriors widened
    assert sig["qldpc_minsum32_decode_batch_dev"][1][2] is C.c_void_p and sig["qldpc_minsum32_decode_batch_dev"][1][7] is C.c_void_p
    assert _lib.F32_FORM_CLEAN == 1
