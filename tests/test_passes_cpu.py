"""The models of tests/passes_model.py are the reference: they equal the CPU oracle on every case of the table and reproduce what the
reference itself recorded (tests/golden/core_passes.npz), the table keeps its unstable cases under 10 %, and the comparison the GPU
tests make rejects every deliberately wrong variant.  No GPU.

Measured on this table (largest |f64 - mp| / pass_tolerance over every edge and column sum of every single-pass case):
    numpy (bp_pass_f64)        0.369
    oracle (libm tanh/atanh)   0.447
and for the recorded reference messages bp_R_dense (numba, fastmath) 0.321.  The bound asserted is 0.5; the GPU gets 1.0.
Driver: 196 cases, 8 unstable (the discrete priors, exact zeros among the posteriors); over the stable ones the largest d_ref is 5.8e-9
(a saturated n30 case) and the smallest margin is 1.8e4 tol, against the 1e4 tol the definition asks for.
"""
import numpy as np
import pytest

import passes_model as M


def dense_of(indptr, indices, n):
    m = len(indptr) - 1
    H = np.zeros((m, n))
    for i in range(m):
        H[i, indices[indptr[i]:indptr[i + 1]]] = 1.0
    return H


def scatter(indptr, indices, n, x):
    out = np.zeros((len(indptr) - 1, n))
    for i in range(len(indptr) - 1):
        out[i, indices[indptr[i]:indptr[i + 1]]] = x[indptr[i]:indptr[i + 1]]
    return out


@pytest.fixture(scope="module")
def f64_pass():
    """bp_pass_f64 on every distinct shot of every single-pass case, once"""
    return {c["name"]: np.array([M.bp_pass_f64(c["indptr"], c["indices"], c["Q"][d], c["ssign"][d]) for d in range(M.PASS_DISTINCT)]).reshape(
        M.PASS_DISTINCT, c["nnz"]) for c in M.pass_cases()}


@pytest.fixture(scope="module")
def oracle_pass(oracle):
    out = {}
    for c in M.pass_cases():
        mask = dense_of(c["indptr"], c["indices"], c["n"]) != 0
        rows = []
        for d in range(M.PASS_DISTINCT):
            Rd = oracle.bp_core_dense(scatter(c["indptr"], c["indices"], c["n"], c["Q"][d]), c["ssign"][d], mask, M.CLIP) if c["m"] else np.zeros((0, c["n"]))
            rows.append(Rd[mask])                       # row-major order of the mask is CSR order
        out[c["name"]] = np.array(rows).reshape(M.PASS_DISTINCT, c["nnz"])
    return out


def rows_all():
    return np.arange(M.PASS_DISTINCT)


def test_pass_model_equals_oracle_and_stays_within_half_the_tolerance(f64_pass, oracle_pass):
    """numpy f64 and the oracle against the 50-digit model: both within 0.5 pass_tolerance on every case (hence within 1.0 of each
    other), column sums included"""
    worst = {"numpy": 0.0, "oracle": 0.0}
    for c in M.pass_cases():
        for who, R in (("numpy", f64_pass[c["name"]]), ("oracle", oracle_pass[c["name"]])):
            r = M.pass_ratio(c, rows_all(), R, M.column_sums(c["indptr"], c["indices"], c["n"], R))
            assert r <= 0.5, (c["name"], who, r)
            worst[who] = max(worst[who], r)
        if c["nnz"]:
            assert np.all(np.abs(f64_pass[c["name"]] - oracle_pass[c["name"]]) <= c["tol"]), c["name"]
    print("largest |f64 - mp| / pass_tolerance:", worst)
    assert min(worst.values()) > 0.01                                 # the bound is within two orders of what the arithmetic does


def test_pass_cases_reach_the_edges():
    """the table holds what the issue asks for: clamped factors of both signs and zeros, the clip, infinities, rows of degree 1, 23 and
    56, an empty row, a column without edges, a graph without rows, underflowing products"""
    cases = {c["name"]: c for c in M.pass_cases()}
    assert set(c["graph"] for c in cases.values()) == {"core", "random4", "irregular", "wide", "norows", "bb72"}
    assert cases["norows-n3"]["nnz"] == 0 and cases["norows-n3"]["n"] == 4
    assert sorted(np.diff(cases["wide-n3"]["indptr"]))[-2:] == [23, 56]
    assert sorted(np.diff(cases["irregular-n3"]["indptr"]))[:2] == [0, 1] and 5 not in cases["irregular-n3"]["indices"]
    assert np.max(np.abs(cases["core-n30"]["pc"])) == M.CLIP and np.max(np.abs(cases["core-n1e-3"]["pc"])) < 1e-9
    d = cases["random4-discrete"]
    for v in M.DISCRETE:
        assert np.any((d["Q"] == v) & (np.signbit(d["Q"]) == np.signbit(v))), v
    w = cases["wide-discrete"]
    assert np.all(np.abs(w["R"][:, :56]) < 1e-300) and np.all(np.isin(w["Q"][:, :79], M.CLAMPED))


def test_models_reproduce_the_recorded_reference(golden):
    """bp_R_dense and bpdrv_* of core_passes.npz are what the reference's numba code returned: the f64 models reproduce them, decisions,
    flag and iteration exactly, values within the bounds derived from the 50-digit model"""
    g = golden("core_passes")
    ip, ix, n = g["indptr"], g["indices"], int(g["shape"][1])
    mask = dense_of(ip, ix, n) != 0
    deg = M.edge_degrees(ip)
    worst = 0.0
    for t in range(g["bp_Q"].shape[0]):
        r, pc = M.bp_pass_mp(ip, ix, g["bp_Q"][t], g["syndrome_sign"][t])
        r, pc = np.array([float(x) for x in r]), np.array([float(x) for x in pc])
        tol = M.pass_tolerance(deg, pc, r)
        rec = g["bp_R_dense"][t]
        assert not rec[~mask].any()
        worst = max(worst, float(np.max(np.abs(rec[mask] - r) / tol)))
        assert np.all(np.abs(M.bp_pass_f64(ip, ix, g["bp_Q"][t], g["syndrome_sign"][t]) - rec[mask]) <= tol)
    print("recorded bp_R_dense against the mp model, largest ratio:", worst)
    assert worst <= 0.5
    for t, s in enumerate(g["bpdrv_syndromes"]):
        f = M.bp_decode_f64(ip, ix, n, s, g["bpdrv_prior"], 12)
        assert np.array_equal(f["err"], g["bpdrv_err"][t]) and f["conv"] == bool(g["bpdrv_conv"][t]) and f["iter"] == g["bpdrv_iter"][t], t
        mp_ = M.bp_decode_mp(ip, ix, n, s, g["bpdrv_prior"], 12)
        assert mp_["conv"] == f["conv"] and mp_["iter"] == f["iter"] and np.array_equal(mp_["err"], f["err"])
        V = np.array([[float(x) for x in v] for v in mp_["values"]])
        tol = 100.0 * max(float(np.max(np.abs(f["values"] - V))), 16 * M.U * float(np.max(np.abs(V))))
        assert np.max(np.abs(g["bpdrv_llr"][t] - V[-1])) <= tol and np.max(np.abs(f["values"][-1] - g["bpdrv_llr"][t])) <= tol, t


@pytest.mark.parametrize("max_iter", (1, 2, 3, 10))
def test_driver_model_equals_oracle(oracle, max_iter):
    """bp_decode_f64 against the oracle's dense driver on every case: decisions, flag and iteration exactly, values within the case's
    tol; the prefix rule of passes_model.expected holds for the f64 model too"""
    for c in M.driver_cases():
        H = dense_of(c["indptr"], c["indices"], c["n"])
        f = M.bp_decode_f64(c["indptr"], c["indices"], c["n"], c["syndrome"], c["prior"], max_iter)
        assert np.array_equal(f["values"], c["f64"]["values"][:len(f["values"])]), c["name"]
        if c["m"] == 0:
            continue                                                   # the dense oracle needs a row to read
        e, conv, v, it = oracle.bp_dense_driver(H, c["syndrome"], c["prior"], max_iter=max_iter)
        assert np.array_equal(e, f["err"]) and conv == f["conv"] and it == f["iter"], c["name"]
        assert np.all(np.abs(v - f["values"][-1]) <= c["tol"]), c["name"]
        assert not M.driver_failures(c, max_iter, e, conv, it, v), c["name"]


def test_driver_table_is_stable_enough():
    """at most 10 % of the driver cases are unstable; the batch case holds shots that converge at iteration 0, later and never; the
    ladder has a stable non-converged shot on every graph with rows"""
    cases = M.driver_cases()
    unstable = [c["name"] for c in cases if not c["stable"]]
    print(f"{len(cases)} driver cases, {len(unstable)} unstable:", unstable)
    print("largest d_ref", max(c["d_ref"] for c in cases if c["stable"]), "smallest margin / tol", min(c["margin"] / c["tol"] for c in cases if c["stable"] and c["tol"]))
    assert len(unstable) <= 0.10 * len(cases)
    batch = [c for c in cases if c["group"] == M.BATCH_CASE]
    assert len(batch) == M.BATCH_DISTINCT and all(c["stable"] for c in batch)
    kinds = {("never" if not c["conv"] else "first" if c["iter"] == 0 else "later") for c in batch}
    assert kinds == {"never", "first", "later"}
    for g in ("core", "random4", "irregular", "wide", "bb72"):
        assert any(c["graph"] == g and c["stable"] and not c["conv"] for c in cases), g
    assert any(c["graph"] == "norows" and c["conv"] and c["iter"] == 0 for c in cases)


@pytest.mark.parametrize("flaw", M.PASS_FLAWS)
def test_comparison_rejects_a_wrong_pass(flaw, f64_pass):
    """each wrong variant of the check pass exceeds 1.0 pass_tolerance on at least one case; the right one stays below on all"""
    rejected = []
    for c in M.pass_cases():
        R = np.array([M.bp_pass_f64(c["indptr"], c["indices"], c["Q"][d], c["ssign"][d], flaw=flaw) for d in range(M.PASS_DISTINCT)]).reshape(M.PASS_DISTINCT, c["nnz"])
        if M.pass_ratio(c, rows_all(), R, M.column_sums(c["indptr"], c["indices"], c["n"], R)) > 1.0:
            rejected.append(c["name"])
        assert M.pass_ratio(c, rows_all(), f64_pass[c["name"]]) <= 1.0
    assert rejected, flaw
    print(flaw, "rejected by", rejected)


@pytest.mark.parametrize("flaw", M.PASS_FLAWS[2:] + M.DRIVER_FLAWS)
def test_comparison_rejects_a_wrong_driver(flaw):
    """(the two clamp variants are the single pass's to reject: a posterior that reaches the clamp is an exact zero, which makes its
    case unstable, and the driver runs the single pass's kernel)  each other wrong variant of the driver is refused by at least one of the comparisons test_passes_gpu.py makes: stable cases at
    max_iter 10, the max_iter = 1, 2, 3 ladder on non-converged shots, and iteration 0 against the ordered column sum of the check
    pass's own messages (bit for bit: the only comparison a changed rounding can fail)"""
    rejected = []
    for c in M.driver_cases():
        a = (c["indptr"], c["indices"], c["n"], c["syndrome"], c["prior"])
        for k in (10,) + ((1, 2, 3) if c["stable"] and not c["conv"] else ()):
            f = M.bp_decode_f64(*a, k, flaw=flaw)
            if M.driver_failures(c, k, f["err"], f["conv"], f["iter"], f["values"][-1]):
                rejected.append((c["name"], k))
        first = M.bp_decode_f64(*a, 1, flaw=flaw)["values"][0]
        R = M.bp_pass_f64(c["indptr"], c["indices"], c["prior"][c["indices"]] if len(c["indices"]) else np.zeros(0), 1.0 - 2.0 * c["syndrome"], flaw=flaw if flaw in M.PASS_FLAWS else None)
        if not np.array_equal(first, M.column_sums(c["indptr"], c["indices"], c["n"], R, c["prior"])[0]):
            rejected.append((c["name"], "column sum"))
        if len(rejected) >= 3:
            break                                                      # enough: one case has to reject, the rest of the table adds time only
    assert rejected, flaw
    print(flaw, "rejected by", len(rejected), "comparisons, e.g.", rejected[:4])
