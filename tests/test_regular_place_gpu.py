"""The fixed-work ownership form of the regular min-sum kernel on LDS addresses taken from a per-thread place table (csrc/regular_place.h,
qldpc_set_option "regular_place", default 1; 0 = the linear layout through the same kernel): bit for bit against the C oracle and against each other.  The
early-exit form keeps the slot-relative addresses and runs beside it under both values.  The decode API
(posterior words, hard decisions, verdicts, iteration counts) on bb72 Hx (S = 14, teams that straddle waves), bb144 Hx, the m = 257 graph (S = 1, 63 lanes
of no team) and the m = 36 graph without torus structure; early exit and fixed work; max_iter 0, 1, 2 and 50; one converging shot, one failing shot and
S + 1 shots (a second trip with a partly filled workgroup).  The fused Monte-Carlo tally at p = 0.005 and 0.08 over 1, S + 1 and 1501 shots; a
shot-list launch under "mc_list_shots", whose S differs from the full launch's; and a fixed-work decode with an iteration table long enough to cut S: a
second table on the same handle."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_minima_model as CM  # noqa: E402
import regular_shapes as RS  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = ("bb72", "bb144", "r63_m257", "r63_m36")
MC_SHAPES = ("bb72", "r63_m257")
BB_RATE = 0.03
MC_PS, MC_SEED, MC_MANY = (0.005, 0.08), 20261020, 1501
LIST_SHOTS = 3
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
    L.set_option("regular_place", 1)
    L.set_option("mc_first_iteration", 1)
    L.set_option("mc_list_shots", 0)


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
            synd[0] = np.random.default_rng([MC_SEED, m, 1]).random(m) < 0.5          # unrealisable: BP fails on it
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
        assert np.array_equal(np.asarray(a), np.asarray(b)), f"{ctx}: {what} differs"


@pytest.mark.parametrize("max_iter", [0, 1, 2, 50])
@pytest.mark.parametrize("name", SHAPES)
def test_decode_equals_the_oracle_under_either_value(L, options, oracle, name, max_iter):
    graph, ip, ix, m, n, S, prior, synd, _ = shape(L, name)
    assert (S, L.minsum_decode_path(graph, prior, max_iter, "dynamical", 1.0)[0]) == (RS.LB_T // m, L.PATH_REGULAR)
    want = [np.asarray(w) for w in oracle.minsum_decode_batch(ip, ix, n, synd, prior, max_iter=max_iter, threads=0)]
    batches = {"S + 1 shots": np.arange(S + 1), "one failing shot": np.array([0])}
    if max_iter == 50:
        conv = want[1].astype(bool)
        assert not conv[0] and conv[1:].any(), name                                  # converging and failing shots in one workgroup
        batches["one converging shot"] = np.array([int(np.flatnonzero(conv)[0])])
    for value in (1, 0):
        options("regular_place", value)
        for what, pick in batches.items():
            for flags, form in ((0, "early exit"), (L.FLAG_FIXED_ITERS, "fixed work")):
                got = L.minsum_decode_batch(graph, synd[pick], prior, max_iter, "dynamical", 1.0, flags=flags)
                same(got, [w[pick] for w in want], f"{name} max_iter {max_iter} {what} {form} regular_place {value}")


@pytest.fixture(scope="module")
def mc_reference(L, oracle):
    """the oracle's tallies, shared by the forms below: {(graph, p, count): tally}"""
    out = {}
    for name in MC_SHAPES:
        graph, ip, ix, m, n, S, _, _, Lmat = shape(L, name)
        for p in MC_PS:
            for count in (1, S + 1, MC_MANY):
                out[name, p, count] = oracle.cc_sample_decode_tally(ip, ix, n, Lmat, p, MC_SEED, 0, count, max_iter=50, threads=0)
    return out


@pytest.mark.parametrize("form", ["early exit", "early exit, every shot in the full decoder", "fixed work"])
def test_monte_carlo_tally_equals_the_oracle_under_either_value(L, options, mc_reference, form):
    options("mc_first_iteration", 0 if "every shot" in form else 1)
    flags = L.FLAG_FIXED_ITERS if form == "fixed work" else 0
    for (name, p, count), want in mc_reference.items():
        graph, *_, Lmat = shape(L, name)
        assert want[L.TALLY["trials"]] == count
        for value in (1, 0):
            options("regular_place", value)
            got = L.cc_sample_decode_tally(graph, Lmat, p, MC_SEED, 0, count, max_iter=50, flags=flags)
            assert np.array_equal(got, want), (form, name, p, count, value, got.tolist(), want.tolist())
    for name in MC_SHAPES:
        assert mc_reference[name, 0.08, MC_MANY][L.TALLY["bp_conv_z"]] < mc_reference[name, 0.005, MC_MANY][L.TALLY["bp_conv_z"]] <= MC_MANY      # BP failures to export at 0.08


def test_a_shot_list_launch_with_another_s(L, options, mc_reference):
    """early exit with the bit-sliced first iteration: the shots it does not finish go to the full decoder as a list, LIST_SHOTS per workgroup instead of
    bb72's 14 -- another (S, block) on the handle the full launches above have used"""
    graph, ip, ix, m, n, S, _, _, Lmat = shape(L, "bb72")
    assert S != LIST_SHOTS
    options("mc_first_iteration", 1)
    for list_shots in (LIST_SHOTS, 0, LIST_SHOTS):
        options("mc_list_shots", list_shots)
        for value in (1, 0):
            options("regular_place", value)
            for p in MC_PS:
                got = L.cc_sample_decode_tally(graph, Lmat, p, MC_SEED, 0, MC_MANY, max_iter=50)
                assert np.array_equal(got, mc_reference["bb72", p, MC_MANY]), (list_shots, value, p, got.tolist())


@pytest.mark.parametrize("name", ["bb72", "bb144"])
def test_a_long_iteration_table_cuts_s_and_takes_a_second_table(L, options, oracle, name):
    """the alpha table lives in LDS behind the posteriors: at max_iter 1024 the carve holds fewer shots, so the same handle launches with another (S, block)
    and builds another place table; then the first shape again"""
    graph, ip, ix, m, n, S, prior, synd, _ = shape(L, name)
    long_iter = 1024
    assert RS.plan(6, m, n, long_iter)[1] < S == RS.plan(6, m, n, 50)[1]
    for max_iter in (50, long_iter, 50):
        want = oracle.minsum_decode_batch(ip, ix, n, synd, prior, max_iter=max_iter, threads=0)
        for value in (1, 0):
            options("regular_place", value)
            got = L.minsum_decode_batch(graph, synd, prior, max_iter, "dynamical", 1.0, flags=L.FLAG_FIXED_ITERS)
            same(got, want, f"{name} max_iter {max_iter} fixed work regular_place {value}")


def test_the_option_takes_0_and_1_only(L, options):
    for bad in (2, -1):
        with pytest.raises(L.QldpcError):
            L.set_option("regular_place", bad)
    L.set_option("regular_place", 0)
    L.set_option("regular_place", 1)
