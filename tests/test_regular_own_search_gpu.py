"""The regular min-sum kernel on the edge-ownership table that regular_own_assign CHOOSES (csrc/regular_own.h; qldpc_set_option "regular_own_search",
read when a graph handle is created), bit for bit against the C oracle and against the other tables: a handle created under regular_own_search 0 (the
first matching found) and a launch under regular_own_edges 0 (no ownership at all).  Which valid assignment a handle holds moves LDS bank conflicts
and nothing else, so posterior words, hard decisions, verdicts, iteration counts and the Monte-Carlo tally are the same words under all three.
Shapes: bb72 (S = 14, a translation-invariant table), r63_m36 (S = 14, a searched table), r63_m257 (S = 1, 63 lanes without a team), bb144 (S = 7,
the benchmark's graph); batches of about two thousand shots that leave teams of the last workgroup without a shot; early exit and fixed work at
max_iter 1, 2 and 50."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regular_shapes as RS  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = ("bb72", "r63_m36", "r63_m257", "bb144")
SHOTS = 2053                    # 2053 = 146 * 14 + 9 = 293 * 7 + 2: the last workgroup has five teams without a shot at S = 14 and at S = 7
MC_SHOTS, MC_P, MC_SEED = 3005, 0.02, 20261020
BB_RATE = 0.03
TABLES = ("search 1", "search 0", "edges 0")
_CACHE = {}


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


@pytest.fixture
def options(L):
    """qldpc_set_option switches are process-wide: the defaults come back after every test, passed or not"""
    yield L.set_option
    L.set_option("regular_own_search", 1)
    L.set_option("regular_own_edges", 1)


def shape(L, name):
    """-> (handles {"search 1", "search 0"}, indptr, indices, m, n, S, prior, syndromes [SHOTS, m], logicals, error rate of the tally): once per module"""
    if name not in _CACHE:
        if name.startswith("bb"):
            from qldpc_amd.data import load_code
            c = load_code(name)
            ip, ix, m, n = c["Hx_indptr"], c["Hx_indices"], int(c["m"]), int(c["n"])
            S = RS.plan(6, m, n)[1]
            prior = np.full(n, np.log((1 - BB_RATE) / BB_RATE))
            errs = (np.random.default_rng([MC_SEED, m]).random((SHOTS, n)) < BB_RATE * 2.0).astype(np.int64)
            synd = (errs[:, ix.reshape(m, 6)].sum(axis=-1) & 1).astype(np.int8)
            logicals, p = c["Lx"], MC_P
        else:
            g = RS.graph(name)
            ip, ix, m, n, S = g.indptr, g.indices, g.m, g.n, g.S
            prior = RS.priors(g)["normal"]
            synd = RS.syndromes(g, SHOTS, prior, salt=5)                   # shot 0 is unrealisable: BP fails on it
            logicals, p = RS.logicals(g), g.rate
        handles = {}
        try:
            for value in (1, 0):
                L.set_option("regular_own_search", value)
                handles[f"search {value}"] = L.Graph(ip, ix, n)
        finally:
            L.set_option("regular_own_search", 1)
        _CACHE[name] = (handles, ip, ix, m, n, S, prior, synd, logicals, p)
    return _CACHE[name]


def under(L, handles, table):
    """the handle and the regular_own_edges value of one of TABLES"""
    L.set_option("regular_own_edges", 0 if table == "edges 0" else 1)
    return handles["search 0" if table == "search 0" else "search 1"]


def same(got, want, ctx):
    for what, a, b in zip(("err", "conv", "llr", "iter"), got, want):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        if what == "llr":
            a, b = a.view(np.uint64), b.view(np.uint64)                    # words, not values: -0.0 and NaN payloads count
        assert a.shape == b.shape and np.array_equal(a, b), f"{ctx}: {what} differs"


@pytest.mark.parametrize("max_iter", [1, 2, 50])
@pytest.mark.parametrize("name", SHAPES)
def test_decode_equals_the_oracle_on_every_table(L, options, oracle, name, max_iter):
    handles, ip, ix, m, n, S, prior, synd, _, _ = shape(L, name)
    assert S == RS.LB_T // m and (S == 1 or SHOTS % S != 0)                # a team without a shot wherever a workgroup has more than one team
    assert L.minsum_decode_path(handles["search 1"], prior, max_iter, "dynamical", 1.0)[0] == L.PATH_REGULAR
    want = oracle.minsum_decode_batch(ip, ix, n, synd, prior, max_iter=max_iter, threads=0)
    if max_iter == 50:
        assert 0 < int(np.asarray(want[1]).sum()) < SHOTS, name            # converging and failing shots
    for flags, form in ((0, "early exit"), (L.FLAG_FIXED_ITERS, "fixed work")):
        first = None
        for table in TABLES:
            got = L.minsum_decode_batch(under(L, handles, table), synd, prior, max_iter, "dynamical", 1.0, flags=flags)
            same(got, want, f"{name} max_iter {max_iter} {form} {table} against the oracle")
            if first is None:
                first = got
            same(got, first, f"{name} max_iter {max_iter} {form} {table} against {TABLES[0]}")


@pytest.mark.parametrize("name", SHAPES)
def test_monte_carlo_tally_equals_the_oracle_on_every_table(L, options, oracle, name):
    handles, ip, ix, m, n, S, _, _, Lmat, p = shape(L, name)
    assert S == 1 or MC_SHOTS % S != 0
    want = oracle.cc_sample_decode_tally(ip, ix, n, Lmat, p, MC_SEED, 0, MC_SHOTS, max_iter=50, threads=0)
    assert want[L.TALLY["trials"]] == MC_SHOTS and 0 < want[L.TALLY["bp_conv_z"]] <= MC_SHOTS
    for flags, form in ((0, "early exit"), (L.FLAG_FIXED_ITERS, "fixed work")):
        for table in TABLES:
            got = L.cc_sample_decode_tally(under(L, handles, table), Lmat, p, MC_SEED, 0, MC_SHOTS, max_iter=50, flags=flags)
            assert np.array_equal(got, want), (name, form, table, got.tolist(), want.tolist())


def test_the_option_takes_0_and_1_only_and_ends_at_its_default(L, options):
    with pytest.raises(L.QldpcError):
        L.set_option("regular_own_search", 2)
    with pytest.raises(L.QldpcError):
        L.set_option("regular_own_search", -1)
    L.set_option("regular_own_search", 0)
    L.set_option("regular_own_search", 1)
