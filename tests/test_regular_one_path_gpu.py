"""The bare passes of the fixed-work ownership form once a wave of class "none" runs them in one straight path and every other wave takes its sums out
of line behind one taken branch (csrc/minsum_regular.hip, PLACE): the Monte-Carlo tally and the decode API's outputs bit for bit against the C oracle,
with qldpc_set_option "regular_wave_classes" 1 and 0 (0: no wave is labelled "none", every wave takes the out-of-line arm).

The smallest inputs at which the two paths can go wrong.  bb72 Hx (S = 14: six "none" waves, a pure "one" wave and a mixed wave) and bb144 Hx (S = 7:
seven "none" waves and a wave of "one", "both" and the 8 lanes of no team).  max_iter 2, 3 and 50: the switch into the bare loop at its earliest pass
and at a normal one (the loop now fetches its first alpha itself).  S - 1, S + 1 and 3 S + 2 shots: a team without a shot and the lanes of no team run
the arms.  p = 0.005, where every workgroup enters the bare loop, and p = 0.05, where by the oracle 27 of 280 shots on bb72 and 15 of 140 on bb144 are
BP failures at max_iter 50, so some workgroups of 20 never enter it and others do (FAILURES pins the oracle's counts).  max_iter 0 is not compared:
the oracle's own tally differs between processes there (tests/test_regular_waves_gpu.py)."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_minima_model as CM  # noqa: E402
import regular_shapes as RS  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = {"bb72": 14, "bb144": 7}                                   # graph -> S
ITERS = (2, 3, 50)
MC_SEED, LOW, HIGH = 20261021, 0.005, 0.05
FAILURES = {"bb72": 27, "bb144": 15}                                # osd_z of 20 S shots at HIGH, max_iter 50, by the oracle
BB_RATE, ERR_RATE = 0.03, 0.01                                      # the prior's rate; the errors of the decode test: by the oracle every one converges within two iterations
_CACHE = {}


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


@pytest.fixture
def options(L):
    """qldpc_set_option switches are process-wide: put the default back after a test that turns one"""
    yield L.set_option
    L.set_option("regular_wave_classes", 1)


def shape(L, name):
    """-> (graph handle, indptr, indices, m, n, S, prior, syndromes of 3 S + 3 shots with an unrealisable one first, logicals): once per module"""
    if name not in _CACHE:
        from qldpc_amd.data import load_code
        c = load_code(name)
        ip, ix, m, n = c["Hx_indptr"], c["Hx_indices"], int(c["m"]), int(c["n"])
        S = RS.plan(6, m, n)[1]
        assert S == SHAPES[name], (name, S)
        prior = np.full(n, np.log((1 - BB_RATE) / BB_RATE))
        errs = (np.random.default_rng([MC_SEED, m]).random((3 * S + 3, n)) < ERR_RATE).astype(np.int64)
        synd = (errs[:, ix.reshape(m, 6)].sum(axis=-1) & 1).astype(np.int8)
        synd[0] = np.random.default_rng([MC_SEED, m, 1]).random(m) < 0.5              # unrealisable: BP fails on it
        _CACHE[name] = (L.Graph(ip, ix, n), ip, ix, m, n, S, prior, synd, c["Lx"])
    return _CACHE[name]


@pytest.mark.parametrize("max_iter", ITERS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_monte_carlo_tally_equals_the_oracle(L, options, oracle, name, max_iter):
    graph, ip, ix, m, n, S, _, _, Lmat = shape(L, name)
    for p, counts in ((LOW, (S - 1, S + 1, 3 * S + 2)), (HIGH, (S - 1, S + 1, 3 * S + 2, 20 * S))):
        for count in counts:
            want = oracle.cc_sample_decode_tally(ip, ix, n, Lmat, p, MC_SEED, 0, count, max_iter=max_iter, threads=0)
            assert want[L.TALLY["trials"]] == count
            if p == LOW:
                assert want[L.TALLY["bp_conv_z"]] == count, (name, max_iter, count)  # every workgroup enters the bare loop
            if p == HIGH and count == 20 * S and max_iter == 50:
                assert want[L.TALLY["osd_z"]] == FAILURES[name], (name, want.tolist())  # fewer failures than workgroups: some enter it, some never do
            for value in (1, 0):
                options("regular_wave_classes", value)
                got = L.cc_sample_decode_tally(graph, Lmat, p, MC_SEED, 0, count, max_iter=max_iter, flags=L.FLAG_FIXED_ITERS)
                assert np.array_equal(got, want), (name, max_iter, p, count, value, got.tolist(), want.tolist())


@pytest.mark.parametrize("max_iter", ITERS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_decode_equals_the_oracle(L, options, oracle, name, max_iter):
    graph, ip, ix, m, n, S, prior, synd, _ = shape(L, name)
    assert L.minsum_decode_path(graph, prior, max_iter, "dynamical", 1.0)[0] == L.PATH_REGULAR
    want = [np.asarray(w) for w in oracle.minsum_decode_batch(ip, ix, n, synd, prior, max_iter=max_iter, threads=0)]
    assert not want[1][0] and want[1][1:].all(), name                                # shot 0 fails, the others converge: their workgroups enter the bare loop at its first pass
    # S - 1 realisable shots (one team without a shot), S + 1 with the failing one (the first workgroup never enters the bare loop, the second holds one
    # shot), 3 S + 2 realisable ones (the last workgroup holds 2 shots)
    batches = {"S - 1 shots": np.arange(1, S), "S + 1 shots": np.arange(S + 1), "3 S + 2 shots": np.arange(1, 3 * S + 3)}
    for value in (1, 0):
        options("regular_wave_classes", value)
        for what, pick in batches.items():
            got = L.minsum_decode_batch(graph, synd[pick], prior, max_iter, "dynamical", 1.0, flags=L.FLAG_FIXED_ITERS)
            for part, a, b in zip(("err", "conv", "llr", "iter"), got, [w[pick] for w in want]):
                if part == "llr":
                    a, b = CM.words(a), CM.words(b)
                assert np.array_equal(np.asarray(a), np.asarray(b)), f"{name} max_iter {max_iter} {what} regular_wave_classes {value}: {part} differs"
