"""The clean forms of the regular min-sum kernel after two changes to their loops (csrc/minsum_regular.hip): the variable sum starts at its first message
instead of at 0.0 + that message (header comment, "zero"; both loops, with and without edge ownership), and the bare loop of the fixed-work form takes
alpha_it from a scalar load issued one pass ahead, its index clamped to max_iter - 1, instead of from the staged LDS table.  Every output word --
posterior words, hard decisions, verdicts, iteration counts, the Monte-Carlo tally -- is compared with the C oracle, whose sum is the reference's
((0.0 + a) + b) + c + prior, under regular_own_edges 1 and 0.

What a case can and cannot see: the bare loop runs once every shot of a workgroup is frozen, so nothing it computes is an output; a wrong alpha there
cannot change a word, and what these cases pin of it is that outputs stay frozen through it and that it ends (max_iter 1 and 2 leave it nothing or one
pass to run, 50 many; a batch of one converging shot sends its workgroup there at once, with every other team idle).  The first loop's sum is
observable in every posterior word.  Alpha is non-constant in both modes ("dynamical" and a sequence with max_iter distinct entries).
Shapes: bb72 Hx (m = 36, 14 teams per workgroup), bb144 Hx (72-lane teams that straddle the 32-lane groups), r63_m257 (one team, 63 idle lanes).
Batches: one converging shot, one failing shot, S + 1 shots of both kinds (teams without a shot); low and high error rates."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regular_shapes as RS  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = ("bb72", "bb144", "r63_m257")
SEED = 20261021
LOW, HIGH = 0.01, 0.12           # error rates of the two kinds of shot: BP converges on the first kind and fails on most of the second
MC_RATES = (0.005, 0.08)
MC_COUNT = 1501                  # odd and no multiple of 7 or 14: the last workgroup has teams without a shot
TABLES = ("edges 1", "edges 0")
_CACHE = {}


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


@pytest.fixture
def options(L):
    """qldpc_set_option switches are process-wide: the default comes back after every test, passed or not"""
    yield L.set_option
    L.set_option("regular_own_edges", 1)


def alpha_sequence(max_iter):
    """max(max_iter, 1) distinct finite positive factors, neither monotone nor ending on a repeated value"""
    k = np.arange(max(max_iter, 1))
    return 0.625 + 0.3125 * ((7 * k + 3) % 53) / 53.0


def shape(L, oracle, name):
    """-> (handle, indptr, indices, m, n, S, prior, syndromes [S + 1, m], logicals): shot 0 converges, shot 1 fails, the rest alternate; once per module"""
    if name not in _CACHE:
        if name.startswith("bb"):
            from qldpc_amd.data import load_code
            c = load_code(name)
            ip, ix, m, n = c["Hx_indptr"], c["Hx_indices"], int(c["m"]), int(c["n"])
            S = RS.plan(6, m, n)[1]
            logicals = c["Lx"]
        else:
            g = RS.graph(name)
            ip, ix, m, n, S = g.indptr, g.indices, g.m, g.n, g.S
            logicals = RS.logicals(g)
        cols = np.asarray(ix, np.int64).reshape(m, 6)
        prior = np.full(n, np.log((1 - 0.03) / 0.03))
        rng = np.random.default_rng([SEED, m])
        pool = {}
        for rate in (LOW, HIGH):
            errs = rng.random((64, n)) < rate
            synd = (errs[:, cols].sum(axis=-1) & 1).astype(np.int8)
            conv = np.asarray(oracle.minsum_decode_batch(ip, ix, n, synd, prior, max_iter=50, threads=0)[1]).astype(bool)
            keep = conv & synd.any(axis=1) if rate == LOW else ~conv
            assert keep.sum() >= (S + 2) // 2, (name, rate, int(keep.sum()))
            pool[rate] = synd[keep]
        synd = np.empty((S + 1, m), np.int8)
        synd[0::2] = pool[LOW][:len(synd[0::2])]
        synd[1::2] = pool[HIGH][:len(synd[1::2])]
        _CACHE[name] = (L.Graph(ip, ix, n), ip, ix, m, n, S, prior, synd, logicals)
    return _CACHE[name]


def same(got, want, ctx):
    for what, a, b in zip(("err", "conv", "llr", "iter"), got, want):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        if what == "llr":
            a, b = a.view(np.uint64), b.view(np.uint64)                    # words, not values: -0.0 counts
        assert a.shape == b.shape and np.array_equal(a, b), f"{ctx}: {what} differs"


@pytest.mark.parametrize("max_iter", [0, 1, 2, 50])
@pytest.mark.parametrize("name", SHAPES)
def test_decode_equals_the_oracle_word_for_word(L, options, oracle, name, max_iter):
    handle, ip, ix, m, n, S, prior, synd, _ = shape(L, oracle, name)
    assert len(synd) == S + 1 and S == RS.LB_T // m
    for mode, alpha in (("dynamical", 1.0), ("alvarado-autoregressive", alpha_sequence(max_iter))):
        assert L.minsum_decode_path(handle, prior, max_iter, mode, alpha)[0] == L.PATH_REGULAR
        want = oracle.minsum_decode_batch(ip, ix, n, synd, prior, max_iter=max_iter, alpha=alpha, alpha_mode=mode, threads=0)
        if max_iter == 50:
            conv = np.asarray(want[1]).astype(bool)
            assert conv[0] and not conv[1] and 0 < conv.sum() < len(conv), (name, mode)      # frozen and failing shots, whatever the alpha schedule
        for flags, form in ((0, "early exit"), (L.FLAG_FIXED_ITERS, "fixed work")):
            for table in TABLES:
                options("regular_own_edges", 1 if table == "edges 1" else 0)
                for lo, hi, batch in ((0, 1, "one converging shot"), (1, 2, "one failing shot"), (0, S + 1, "S + 1 shots")):
                    got = L.minsum_decode_batch(handle, synd[lo:hi], prior, max_iter, mode, alpha, flags=flags)
                    same(got, [np.asarray(w)[lo:hi] for w in want], f"{name} max_iter {max_iter} {mode} {form} {table} {batch}")


@pytest.mark.parametrize("name", SHAPES)
def test_monte_carlo_tally_equals_the_oracle(L, options, oracle, name):
    handle, ip, ix, m, n, S, _, _, Lmat = shape(L, oracle, name)
    alpha = alpha_sequence(50)
    for p in MC_RATES:
        for count in (1, S + 1, MC_COUNT):
            want = oracle.cc_sample_decode_tally(ip, ix, n, Lmat, p, SEED, 0, count, max_iter=50, alpha=alpha, alpha_mode="alvarado-autoregressive", threads=0)
            assert want[L.TALLY["trials"]] == count
            if count == MC_COUNT:
                conv = want[L.TALLY["bp_conv_z"]]
                assert (conv > 0) if p == MC_RATES[0] else (conv < count), (name, p, want.tolist())       # frozen workgroups at the low rate, failing ones at the high rate
            for flags, form in ((0, "early exit"), (L.FLAG_FIXED_ITERS, "fixed work")):
                for table in TABLES:
                    options("regular_own_edges", 1 if table == "edges 1" else 0)
                    got = L.cc_sample_decode_tally(handle, Lmat, p, SEED, 0, count, max_iter=50, alpha=alpha, alpha_mode="alvarado-autoregressive", flags=flags)
                    assert np.array_equal(got, want), (name, p, count, form, table, got.tolist(), want.tolist())


def test_a_negative_iteration_count_is_refused(L, oracle):
    handle, _, _, _, _, _, prior, synd, _ = shape(L, oracle, "bb72")
    with pytest.raises(L.QldpcError):
        L.minsum_decode_batch(handle, synd[:1], prior, -1, "dynamical", 1.0)
