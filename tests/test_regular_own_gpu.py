"""The regular min-sum kernel with two edges of each check kept inside its thread (csrc/regular_own.h, qldpc_set_option "regular_own_edges", default 1),
bit for bit against the C oracle: the decode API (posterior words, hard decisions, verdicts, iteration counts) on the BB graphs and on the S = 14 and
the S = 1 (63 lanes without a team) shapes of regular_shapes, for one shot and for one shot more than a workgroup holds, early exit and fixed work,
max_iter 1, 2 and 50; the fused Monte-Carlo tally around a workgroup's S shots and into a partly filled second trip of the persistent grid; and the
option itself: 0 gives what 1 gives, and a (4,2) graph, which has no ownership form, decodes the same under either value."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_minima_model as CM  # noqa: E402
import regular_shapes as RS  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = ("bb72", "bb144", "r63_m36", "r63_m257")
BB_RATE = 0.03
MC_P, MC_SEED = 0.02, 20261019
_CACHE = {}


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


@pytest.fixture
def options(L):
    """qldpc_set_option switches are process-wide: put the defaults back after a test that turns one"""
    yield L.set_option
    L.set_option("regular_own_edges", 1)
    L.set_option("mc_first_iteration", 1)


def shape(L, name):
    """-> (graph handle, indptr, indices, m, n, S, prior, syndromes of S + 1 shots, logicals): once per module"""
    if name not in _CACHE:
        if name.startswith("bb"):
            from qldpc_amd.data import load_code
            c = load_code(name)
            ip, ix, m, n = c["Hx_indptr"], c["Hx_indices"], int(c["m"]), int(c["n"])
            S = RS.plan(6, m, n)[1]
            prior = np.full(n, np.log((1 - BB_RATE) / BB_RATE))
            errs = (np.random.default_rng([MC_SEED, m]).random((S + 1, n)) < BB_RATE * 2.0).astype(np.int64)
            synd = (errs[:, ix.reshape(m, 6)].sum(axis=-1) & 1).astype(np.int8)
            logicals = c["Lx"]
        else:
            g = RS.graph(name)
            ip, ix, m, n, S = g.indptr, g.indices, g.m, g.n, g.S
            prior = RS.priors(g)["normal"]
            synd = RS.syndromes(g, S + 3, prior, salt=3)[:S + 1]          # shot 0 is unrealisable: BP fails on it
            logicals = RS.logicals(g)
        _CACHE[name] = (L.Graph(ip, ix, n), ip, ix, m, n, S, prior, synd, logicals)
    return _CACHE[name]


def same(got, want, ctx):
    for what, a, b in zip(("err", "conv", "llr", "iter"), got, want):
        if what == "llr":
            a, b = CM.words(a), CM.words(b)
        assert np.array_equal(np.asarray(a), np.asarray(b)), f"{ctx}: {what} differs from the oracle"


@pytest.mark.parametrize("max_iter", [1, 2, 50])
@pytest.mark.parametrize("name", SHAPES)
def test_decode_equals_the_oracle(L, oracle, name, max_iter):
    graph, ip, ix, m, n, S, prior, synd, _ = shape(L, name)
    assert (S, L.minsum_decode_path(graph, prior, max_iter, "dynamical", 1.0)[0]) == (RS.LB_T // m, L.PATH_REGULAR)
    want = oracle.minsum_decode_batch(ip, ix, n, synd, prior, max_iter=max_iter, threads=0)
    if max_iter == 50:
        assert 0 < int(np.asarray(want[1]).sum()) < S + 1, name            # converging and failing shots in one workgroup
    for B in (1, S + 1):
        for flags, form in ((0, "early exit"), (L.FLAG_FIXED_ITERS, "fixed work")):
            got = L.minsum_decode_batch(graph, synd[:B], prior, max_iter, "dynamical", 1.0, flags=flags)
            same(got, [np.asarray(w)[:B] for w in want], f"{name} max_iter {max_iter} B {B} {form}")


def mc_counts(S):
    return (1, S - 1, S, S + 1, RS.GRID_CAP * S + S + 5)          # the last: every workgroup once, then one full and one partly filled workgroup


@pytest.fixture(scope="module")
def mc_reference(L, oracle):
    """the oracle's tallies on bb72, one per shot count, shared by the forms below"""
    graph, ip, ix, m, n, S, _, _, Lmat = shape(L, "bb72")
    return {count: oracle.cc_sample_decode_tally(ip, ix, n, Lmat, MC_P, MC_SEED, 0, count, max_iter=50, threads=0) for count in mc_counts(S)}


@pytest.mark.parametrize("form", ["early exit", "early exit, every shot in the full decoder", "fixed work"])
def test_monte_carlo_tally_equals_the_oracle(L, options, mc_reference, form):
    graph, ip, ix, m, n, S, _, _, Lmat = shape(L, "bb72")
    options("mc_first_iteration", 0 if "every shot" in form else 1)
    flags = L.FLAG_FIXED_ITERS if form == "fixed work" else 0
    for count, want in mc_reference.items():
        assert want[L.TALLY["trials"]] == count
        got = L.cc_sample_decode_tally(graph, Lmat, MC_P, MC_SEED, 0, count, max_iter=50, flags=flags)
        assert np.array_equal(got, want), (form, count, got.tolist(), want.tolist())
    big = mc_reference[max(mc_reference)]
    assert 0 < big[L.TALLY["bp_conv_z"]] < max(mc_reference)                        # BP failures are exported from the run that takes a second trip


def test_option_off_equals_option_on(L, options, oracle, mc_reference):
    graph, ip, ix, m, n, S, prior, synd, Lmat = shape(L, "bb72")
    runs = {}
    for value in (1, 0):
        options("regular_own_edges", value)
        runs[value] = [L.minsum_decode_batch(graph, synd, prior, 50, "dynamical", 1.0, flags=flags) for flags in (0, L.FLAG_FIXED_ITERS)]
        runs[value].append(L.cc_sample_decode_tally(graph, Lmat, MC_P, MC_SEED, 0, S + 1, max_iter=50, flags=L.FLAG_FIXED_ITERS))
    for a, b in zip(runs[0][:2], runs[1][:2]):
        same(a, b, "regular_own_edges 0 against 1")
    assert np.array_equal(runs[0][2], runs[1][2]) and np.array_equal(runs[0][2], mc_reference[S + 1])
    with pytest.raises(L.QldpcError):
        L.set_option("regular_own_edges", 2)


def test_a_42_graph_decodes_the_same_under_either_value(L, options, oracle):
    g = RS.graph("r42_m30")
    graph = L.Graph(g.indptr, g.indices, g.n)
    prior = RS.priors(g)["normal"]
    synd = RS.syndromes(g, g.S + 1, prior, salt=3)
    assert L.minsum_decode_path(graph, prior, 50, "dynamical", 1.0)[0] == L.PATH_REGULAR
    want = oracle.minsum_decode_batch(g.indptr, g.indices, g.n, synd, prior, max_iter=50, threads=0)
    for value in (1, 0):
        options("regular_own_edges", value)
        for flags in (0, L.FLAG_FIXED_ITERS):
            same(L.minsum_decode_batch(graph, synd, prior, 50, "dynamical", 1.0, flags=flags), want, f"r42_m30 regular_own_edges {value} flags {flags}")
