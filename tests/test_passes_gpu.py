"""csrc/passes.hip on the MI355X against the models of tests/passes_model.py (what they are worth is test_passes_cpu.py's business):
qldpc_bp_check_pass within 1.0 pass_tolerance of the 50-digit model, qldpc_minsum_check_pass bit for bit with the oracle,
qldpc_bp_decode_batch on the stable cases, in batches across a 256-thread block, along the max_iter ladder and on degenerate graphs, and
the estimator statistics (qldpc_msgstats_create / _histogram) with samples on bin edges and at every admitted bin count.

Measured on the MI355X over this table: largest |R - mp| / pass_tolerance of qldpc_bp_check_pass 0.288 (the bound asserted is 1.0; numpy's
libm needs 0.369), largest |llr - mp| of qldpc_bp_decode_batch on a stable case 0.017 tol.

Out of reach at test sizes, do not try: the 6 GB trial chunking of qldpc_msgstats_create (a chunk is 6 GB / (16 nnz + 8 n + 9 m) trials;
bb72 would need 1.4 million trials) and the 2^31 samples-per-block guard of qldpc_msgstats_histogram (4096 blocks: 8.8e12 samples).
"""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

import passes_model as M

pytestmark = pytest.mark.gpu

PASS_CASES = [c["name"] for c in M.pass_cases()]
DRIVER_GROUPS = list(dict.fromkeys(c["group"] for c in M.driver_cases()))
MEASURED = {}                                                     # printed by the last test of a group: the figures DESIGN.md quotes


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


@pytest.fixture(scope="module")
def dev_graph(L):
    made = {}

    def get(name):
        if name not in made:
            made[name] = L.Graph(*(M.degree1_graph() if name == "degree1" else M.graphs()[name]))
        return made[name]
    return get


def pd(L, a):
    return L.ptr(a, C.c_double)


def check_pass(L, fn, g, Q, ss, param):
    B = Q.shape[0]
    Q, ss = np.ascontiguousarray(Q, np.float64), np.ascontiguousarray(ss, np.float64)
    R, Rs = np.full((B, g.nnz), 7.0), np.full((B, g.n), 7.0)
    L.check(fn(g.handle, C.c_int64(B), pd(L, Q), pd(L, ss), C.c_double(param), pd(L, R), pd(L, Rs)))
    return R, Rs


def bp_decode(L, g, synd, prior, max_iter):
    synd = np.ascontiguousarray(np.atleast_2d(np.asarray(synd, np.int8)))
    B = synd.shape[0]
    assert synd.shape == (B, g.m)
    prior = np.ascontiguousarray(prior, np.float64)
    err, llr, conv, it = np.full((B, g.n), 9, np.int8), np.full((B, g.n), 7.0), np.full(B, 9, np.uint8), np.full(B, -1, np.int32)
    L.check(L.lib().qldpc_bp_decode_batch(g.handle, C.c_int64(B), L.ptr(synd, C.c_int8), pd(L, prior), C.c_int(max_iter), L.ptr(err, C.c_int8), pd(L, llr),
                                          L.ptr(conv, C.c_uint8), L.ptr(it, C.c_int32)))
    return err, llr, conv, it


def same_bits(a, b):
    """equal bit for bit, the sign of a zero included; a NaN equals a NaN (the sign of inf - inf is the hardware's choice)"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64))


# ---- the single passes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PASS_CASES)
def test_bp_check_pass_within_the_derived_bound(L, dev_graph, name):
    """every message within 1.0 pass_tolerance of the 50-digit model and every R_sum within the sum of its edges' tolerances, at
    B = 1, 3, 257, 1000; R_sum is, bit for bit, the ordered sum of the messages the same call returned"""
    c = next(c for c in M.pass_cases() if c["name"] == name)
    g = dev_graph(c["graph"])
    for B in M.BATCHES:
        rows = M.batch_rows(B, M.PASS_DISTINCT)
        R, Rs = check_pass(L, L.lib().qldpc_bp_check_pass, g, c["Q"][rows], c["ssign"][rows], M.CLIP)
        ratio = M.pass_ratio(c, rows, R, Rs)
        print(f"{name} B={B}: largest |R - mp| / pass_tolerance = {ratio:.3f}")
        MEASURED["pass"] = max(MEASURED.get("pass", 0.0), ratio)
        assert ratio <= 1.0, (name, B, ratio)
        assert same_bits(Rs, M.column_sums(c["indptr"], c["indices"], c["n"], R)), (name, B)
    print("largest single-pass ratio so far:", MEASURED["pass"])


@pytest.mark.parametrize("name", PASS_CASES)
def test_minsum_check_pass_bit_identical_to_the_oracle(L, oracle, dev_graph, name):
    """the same inputs through qldpc_minsum_check_pass: -0.0, +-1e-17, +-inf and the degree-1 row (whose message is +-inf) included"""
    c = next(c for c in M.pass_cases() if c["name"] == name)
    g = dev_graph(c["graph"])
    ref = [oracle.minsum_core_sparse(c["indptr"], c["indices"], c["n"], c["Q"][d], c["ssign"][d], 0.75) for d in range(M.PASS_DISTINCT)]
    refR, refS = np.array([r[0] for r in ref]).reshape(M.PASS_DISTINCT, c["nnz"]), np.array([r[1] for r in ref]).reshape(M.PASS_DISTINCT, c["n"])
    if c["graph"] == "irregular":
        assert np.isinf(refR[:, 0]).all()                             # row 0 has degree 1
    for B in M.BATCHES:
        rows = M.batch_rows(B, M.PASS_DISTINCT)
        R, Rs = check_pass(L, L.lib().qldpc_minsum_check_pass, g, c["Q"][rows], c["ssign"][rows], 0.75)
        assert same_bits(R, refR[rows]) and same_bits(Rs, refS[rows]), (name, B)


# ---- the sum-product driver -------------------------------------------------------------------------------------------------
def group_cases(group):
    return [c for c in M.driver_cases() if c["group"] == group]


@pytest.mark.parametrize("group", DRIVER_GROUPS)
def test_bp_decode_against_the_model(L, dev_graph, group):
    """every case at max_iter 1, 2, 3 and 10 (the ladder: iteration k's values show the Q update between passes): finite values of the
    model's shape; on stable cases the model's decisions, flag and iteration exactly and its values within tol.  Iteration 0 equals, bit
    for bit, the ordered column sum of the check pass's own messages plus the prior."""
    cases = group_cases(group)
    c0 = cases[0]
    g = dev_graph(c0["graph"])
    synd = np.array([c["syndrome"] for c in cases], np.int8).reshape(len(cases), c0["m"])
    for k in (1, 2, 3, 10):
        err, llr, conv, it = bp_decode(L, g, synd, c0["prior"], k)
        for b, c in enumerate(cases):
            assert not M.driver_failures(c, k, err[b], conv[b], it[b], llr[b]), (c["name"], k)
            if c["stable"]:
                MEASURED["driver"] = max(MEASURED.get("driver", 0.0), M.driver_deviation(c, k, llr[b]))
        if k == 1:
            Q = np.tile(c0["prior"][c0["indices"]] if g.nnz else np.zeros(0), (len(cases), 1))
            R, _ = check_pass(L, L.lib().qldpc_bp_check_pass, g, Q, 1.0 - 2.0 * synd, M.CLIP)
            assert same_bits(llr, M.column_sums(c0["indptr"], c0["indices"], c0["n"], R, c0["prior"])), group
    print(f"{group}: largest |llr - mp| so far, in units of tol: {MEASURED.get('driver', 0.0):.3g}")


def test_bp_decode_ladder_has_something_to_show(L, dev_graph):
    """the ladder's shots: on every graph with rows a stable shot that does not converge, whose model values move by more than 1e3 tol
    from one iteration to the next, so that a stale Q cannot pass max_iter = 2 and 3"""
    for gname in ("core", "random4", "irregular", "wide", "bb72"):
        c = next(c for c in M.driver_cases() if c["graph"] == gname and c["stable"] and not c["conv"])
        g = dev_graph(gname)
        prev = None
        for k in (1, 2, 3):
            err, llr, conv, it = bp_decode(L, g, c["syndrome"], c["prior"], k)
            assert conv[0] == 0 and it[0] == k - 1 and np.max(np.abs(llr[0] - c["values"][k - 1])) <= c["tol"], (c["name"], k)
            if prev is not None:
                assert np.max(np.abs(llr[0] - prev)) > 1e3 * c["tol"], (c["name"], k)
            prev = llr[0]


@pytest.fixture(scope="module")
def one_shot_calls(L, dev_graph):
    """the batch case's 32 distinct shots, each decoded in a call of its own (B = 1, max_iter 10), read-only"""
    cases = group_cases(M.BATCH_CASE)
    g = dev_graph(cases[0]["graph"])
    outs = [bp_decode(L, g, c["syndrome"], c["prior"], 10) for c in cases]
    return tuple(np.concatenate([o[i] for o in outs]) for i in range(4))


@pytest.mark.parametrize("B", (257, 1000))
def test_bp_decode_batch_freezes_shots_across_a_block(L, dev_graph, one_shot_calls, B):
    """a batch wider than one 256-thread block whose shots converge at iteration 0, later and never, side by side and on both sides of
    row 256: every row equals its one-shot call bit for bit (a converged shot is frozen, not overwritten) and its model row within tol"""
    cases = group_cases(M.BATCH_CASE)
    g = dev_graph(cases[0]["graph"])
    kind = np.array([2 if not c["conv"] else 0 if c["iter"] == 0 else 1 for c in cases])
    rows = M.batch_rows(B, M.BATCH_DISTINCT)
    side_by_side = [np.flatnonzero(kind == k)[0] for k in (0, 2, 1, 0, 1, 2)][:min(B, 259) - 253]
    rows[253:253 + len(side_by_side)] = side_by_side                                         # rows 253..: first, never, later | first, later, never
    assert set(kind[rows[:256]]) == {0, 1, 2} and kind[rows[255]] != kind[rows[256]]
    synd = np.array([cases[r]["syndrome"] for r in rows], np.int8)
    err, llr, conv, it = bp_decode(L, g, synd, cases[0]["prior"], 10)
    e1, l1, c1, i1 = one_shot_calls
    assert np.array_equal(err, e1[rows]) and same_bits(llr, l1[rows]) and np.array_equal(conv, c1[rows]) and np.array_equal(it, i1[rows])
    for b, r in enumerate(rows):
        assert not M.driver_failures(cases[r], 10, err[b], conv[b], it[b], llr[b]), (B, b, cases[r]["name"])
    assert np.array_equal(conv, (kind[rows] != 2).astype(np.uint8)) and (it[kind[rows] == 0] == 0).all() and (it[kind[rows] == 2] == 9).all()


def test_bp_decode_degenerate_graphs(L, dev_graph):
    """no rows: the sign of the prior, converged at iteration 0; a column without edges keeps its prior (0.0 + prior) whatever the
    other columns do, in the unstable discrete cases too"""
    for c in group_cases("norows-n3") + group_cases("norows-n30"):
        err, llr, conv, it = bp_decode(L, dev_graph("norows"), np.zeros((3, 0), np.int8), c["prior"], 10)
        assert np.array_equal(err, np.tile((c["prior"] < 0).astype(np.int8), (3, 1))) and same_bits(llr, np.tile(0.0 + c["prior"], (3, 1)))
        assert conv.all() and not it.any()
    for fam in M.DRIVER_FAMILIES + ("discrete",):
        cases = group_cases(f"irregular-{fam}")
        synd = np.array([c["syndrome"] for c in cases], np.int8)
        for k in (1, 10):
            err, llr, conv, it = bp_decode(L, dev_graph("irregular"), synd, cases[0]["prior"], k)
            assert same_bits(llr[:, 5], np.full(len(cases), 0.0 + cases[0]["prior"][5])) and np.array_equal(err[:, 5], np.full(len(cases), cases[0]["prior"][5] < 0))


# ---- estimator statistics -----------------------------------------------------------------------------------------------------
def binned_like_numpy(stats, samples, bits):
    """range, finite counts and the histograms of a MessageStats equal the oracle's samples binned by numpy: over 7 uniform bins of the
    finite range, and over edges laid through every distinct sample value where there are at most 4096 (which pins the samples
    themselves, not only their counts per coarse bin)"""
    fin = np.isfinite(samples)
    assert stats.finite == (int(np.count_nonzero(fin & (bits == 0))), int(np.count_nonzero(fin & (bits == 1))))
    if not fin.any():
        assert stats.range == (0.0, 0.0)
        return
    assert stats.range == (samples[fin].min(), samples[fin].max())
    x0, x1 = samples[fin & (bits == 0)], samples[fin & (bits == 1)]
    grids = []
    if stats.range[0] < stats.range[1]:
        grids.append((True, np.histogram_bin_edges(np.zeros(0), bins=7, range=stats.range)))
    distinct = np.unique(samples[fin])
    if 2 <= distinct.size <= 4097:
        grids.append((False, distinct))
    for uniform, edges in grids:
        h0, h1 = stats.histogram(edges)
        assert np.array_equal(h0, np.histogram(x0, edges)[0]) and np.array_equal(h1, np.histogram(x1, edges)[0])
        if uniform:
            assert np.array_equal(h0, np.histogram(x0, bins=7, range=stats.range)[0]) and np.array_equal(h1, np.histogram(x1, bins=7, range=stats.range)[0])


def stats_inputs(gname, inf_column=None):
    indptr, indices, n = M.degree1_graph() if gname == "degree1" else M.graphs()[gname]
    rng = np.random.default_rng([20261022, len(gname)])
    q = rng.uniform(0.02, 0.2, n)
    prior = np.log((1 - q) / q)
    if inf_column is not None:
        prior[inf_column] = np.inf
    return indptr, indices, n, prior, (rng.random((300, n)) < 0.1).astype(np.int8)


@pytest.mark.parametrize("gname,inf_column", [("irregular", None), ("wide", None), ("random4", None), ("degree1", None), ("irregular", 2), ("wide", 41)])
def test_message_stats_check_messages(L, oracle, dev_graph, gname, inf_column):
    """check messages after 0, 1 and 3 iterations (damped and clipped from the second on) against oracle.alpha_messages: the degree-1
    row's infinite samples are dropped; with every row of degree 1 no sample is finite, the range is (0, 0) and class_densities raises
    the reference's ValueError; a prior of +inf goes through the Q update of alpha.py:226-244 as in the oracle"""
    from qldpc_amd.decoding._fit import class_densities
    indptr, indices, n, prior, E = stats_inputs(gname, inf_column)
    g = dev_graph(gname)
    for prev, damping, clip in (((), 1.0, 20.0), ((0.7,), 1.0, 20.0), ((0.6, 0.75, 0.85), 0.8, 7.5)):
        R = oracle.alpha_messages(indptr, indices, n, E, prior, alpha_prev=prev, damping=damping, clip_llr=clip)
        mode, alpha = ("alvarado-autoregressive", np.array(prev)) if prev else ("dynamical", 1.0)
        st = L.MessageStats(g, E, prior, L.STATS_CHECK_MESSAGES, len(prev), alpha_mode=mode, alpha=alpha, damping=damping, clip_llr=clip)
        binned_like_numpy(st, R.ravel(), E[:, indices].ravel())
        if gname == "degree1":
            assert st.finite == (0, 0) and st.range == (0.0, 0.0) and np.isinf(R).all()
            with pytest.raises(ValueError, match="No finite samples"):
                class_densities(st, 10, "alpha")
        elif gname == "irregular":
            assert np.isinf(R[:, 0]).all() and sum(st.finite) == R.size - len(E)
        st.close()


@pytest.mark.parametrize("gname", ("irregular", "wide", "random4"))
def test_message_stats_posteriors(L, oracle, dev_graph, gname):
    """the posterior kind after at most 1 and 10 iterations against oracle.scopt_values"""
    indptr, indices, n, prior, E = stats_inputs(gname)
    for iters in (1, 10):
        V = oracle.scopt_values(indptr, indices, n, E, prior, max_iter=iters)
        st = L.MessageStats(dev_graph(gname), E, prior, L.STATS_POSTERIOR, iters)
        binned_like_numpy(st, V.ravel(), E.ravel())
        st.close()


@pytest.fixture(scope="module")
def edge_samples(L, oracle, dev_graph):
    """iteration-0 messages under a prior of 2.0 and 1.0 by turns: every sample is one of -2, -1, 1, 2 -> (MessageStats, x of class 0, x of class 1)"""
    indptr, indices, n = M.graphs()["random4"]
    prior = np.where(np.arange(n) % 2 == 0, 2.0, 1.0)
    E = (np.random.default_rng(20261023).random((200, n)) < 0.15).astype(np.int8)
    R = oracle.alpha_messages(indptr, indices, n, E, prior).ravel()
    bits = E[:, indices].ravel()
    assert set(np.unique(R)) == {-2.0, -1.0, 1.0, 2.0}
    st = L.MessageStats(dev_graph("random4"), E, prior, L.STATS_CHECK_MESSAGES, 0)
    assert st.range == (-2.0, 2.0) and st.finite == (int((bits == 0).sum()), int((bits == 1).sum()))
    yield st, R[bits == 0], R[bits == 1]
    st.close()


@pytest.mark.parametrize("edges", [np.linspace(-2.0, 2.0, 5), [-2.0, -1.0, 0.5, 1.0, 2.0], [-1.0, 0.0, 1.0], [-3.0, -2.0, 2.0], [-2.0, 2.0], [-1.0, 1.0],
                                   [2.0, 3.0], [-4.0, -3.0], [1.0, np.nextafter(1.0, 2.0), 2.0], [-2.0, np.nextafter(-1.0, -2.0), -1.0, 1.5]],
                         ids=lambda e: "e" + "_".join(f"{x:g}" for x in e))
def test_histogram_edges_through_sample_values(edge_samples, edges):
    """samples sit on the first, on interior and on the last edge: bin i holds edges[i] <= x < edges[i + 1], the last bin its upper
    edge too, samples outside are dropped; uniform edges equal np.histogram(x, bins, range), all equal np.histogram(x, edges)"""
    st, x0, x1 = edge_samples
    edges = np.asarray(edges, np.float64)
    h0, h1 = st.histogram(edges)
    assert np.array_equal(h0, np.histogram(x0, edges)[0]) and np.array_equal(h1, np.histogram(x1, edges)[0])
    if np.array_equal(edges, np.linspace(-2.0, 2.0, 5)):
        for x, h in ((x0, h0), (x1, h1)):
            assert np.array_equal(h, np.histogram(x, bins=4, range=(-2.0, 2.0))[0])
            assert list(h) == [np.sum(x == -2), np.sum(x == -1), 0, np.sum(x == 1) + np.sum(x == 2)] and h[0] > 0 and h[1] > 0 and np.sum(x == 2) > 0
    if list(edges) == [-1.0, 0.0, 1.0]:
        assert list(h0) == [np.sum(x0 == -1), np.sum(x0 == 1)]        # +-2 dropped, the last edge inclusive
    if list(edges) == [-4.0, -3.0]:
        assert not h0.any() and not h1.any()


@pytest.mark.parametrize("bins", (1, 2, 4095, 4096))
def test_histogram_bin_counts(edge_samples, bins):
    """every admitted bin count up to kStatsMaxBins = 4096 (65 544 bytes of dynamic LDS: the launch needs the raised limit), uniform
    edges over the range and over a wider interval"""
    st, x0, x1 = edge_samples
    for lo, hi in ((-2.0, 2.0), (-2.5, 3.0)):
        edges = np.linspace(lo, hi, bins + 1)
        h0, h1 = st.histogram(edges)
        assert h0.shape == (bins,) and np.array_equal(h0, np.histogram(x0, edges)[0]) and np.array_equal(h1, np.histogram(x1, edges)[0])
        assert h0.sum() == x0.size and h1.sum() == x1.size


def test_histogram_refusals(L, edge_samples):
    """4097 bins, no bin, and edges that do not increase strictly are refused; the object still works afterwards"""
    st, x0, x1 = edge_samples
    for edges in (np.linspace(-2.0, 2.0, 4098), [1.0], [0.0, 0.0, 1.0], [1.0, 0.0], [0.0, 1.0, 1.0], [0.0, np.nan, 1.0]):
        with pytest.raises(L.QldpcError):
            st.histogram(np.asarray(edges))
    assert st.histogram(np.array([-2.0, 2.0]))[0][0] == x0.size
