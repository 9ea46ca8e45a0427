"""What a shot of the fixed-work ownership form runs before its workgroup reaches the bare loop (csrc/minsum_regular.hip, PLACE): the Monte-Carlo form
reads the columns of a thread's check in front of the sampler, takes the syndrome from them and keeps the two owned ones, packed, for the logical
comparison at the freeze.  The Monte-Carlo tally (its logical-error and zero-syndrome counts come through those columns) and the decode API's four
outputs, bit for bit against the C oracle.

The smallest inputs at which this can go wrong (tests/regular_early_columns_cases.py; tests/test_regular_early_columns_cpu.py proves their properties
with the oracle alone).  bb72 Hx (S = 14) and bb144 Hx (S = 7).  max_iter 1: a shot freezes at pass 1 = max_iter; 2: no bare pass, the final syndrome
test; 3: one bare pass or one more pass of the first loop; 4 and 50.  S - 1, S + 1, 3 S + 2 and 20 S shots: a team without a shot (its lanes load no
columns), a workgroup that holds one shot, the lanes of no team.  Monte-Carlo at p = 0.005, where every shot freezes at pass 1 and every workgroup leaves
through the bare loop, at p = 0.05, where shots freeze at later passes of the first loop and workgroups with a BP failure never leave it, and there
without the OSD export, so that a failing shot takes the logical comparison at it == max_iter.  The decode API with a non-uniform prior and, in the
first workgroup of every batch, a shot that never converges next to shots that converge at iteration 0, at iteration 1 and later.  max_iter 0 is not
compared: the oracle's own tally differs between processes there (tests/test_regular_waves_gpu.py)."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_minima_model as CM  # noqa: E402
import regular_early_columns_cases as OC  # noqa: E402

pytestmark = pytest.mark.gpu
_GRAPHS = {}


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


def graph(L, name):
    if name not in _GRAPHS:
        ip, ix, m, n, S, _ = OC.code(name)
        _GRAPHS[name] = L.Graph(ip, ix, n)
    return _GRAPHS[name]


@pytest.mark.parametrize("max_iter", OC.ITERS)
@pytest.mark.parametrize("name", list(OC.SHAPES))
def test_monte_carlo_tally_equals_the_oracle(L, oracle, name, max_iter):
    ip, ix, m, n, S, Lmat = OC.code(name)
    g = graph(L, name)
    for p, use_osd in ((OC.LOW, True), (OC.HIGH, True), (OC.HIGH, False)):
        for count in OC.counts(S):
            want = oracle.cc_sample_decode_tally(ip, ix, n, Lmat, p, OC.SEED, 0, count, max_iter=max_iter, use_osd=use_osd, threads=0)
            assert want[L.TALLY["trials"]] == count
            if p == OC.LOW and max_iter >= 2:
                assert want[L.TALLY["bp_conv_z"]] == count, (name, max_iter, count)      # every shot freezes at pass 1: every workgroup leaves through the bare loop
            if p == OC.HIGH and count == 20 * S:
                assert 0 < want[L.TALLY["bp_conv_z"]] < count, (name, max_iter)          # BP failures: their workgroups stay in the first loop
            got = L.cc_sample_decode_tally(g, Lmat, p, OC.SEED, 0, count, max_iter=max_iter, use_osd=use_osd, flags=L.FLAG_FIXED_ITERS)
            print(name, max_iter, p, use_osd, count, got.tolist())
            assert np.array_equal(got, want), (name, max_iter, p, use_osd, count, got.tolist(), want.tolist())


@pytest.mark.parametrize("max_iter", OC.ITERS)
@pytest.mark.parametrize("name", list(OC.SHAPES))
def test_decode_equals_the_oracle(L, oracle, name, max_iter):
    ip, ix, m, n, S, _ = OC.code(name)
    g = graph(L, name)
    prior, synd = OC.decode_inputs(name, oracle)
    assert L.minsum_decode_path(g, prior, max_iter, "dynamical", 1.0)[0] == L.PATH_REGULAR
    want = [np.asarray(w) for w in oracle.minsum_decode_batch(ip, ix, n, synd, prior, max_iter=max_iter, threads=0)]
    for count in OC.counts(S):
        head = min(count, S)
        assert OC.classes(want[1][:head], want[3][:head]) == OC.expected_classes(max_iter), (name, max_iter, count)   # all in the first workgroup
        got = L.minsum_decode_batch(g, synd[:count], prior, max_iter, "dynamical", 1.0, flags=L.FLAG_FIXED_ITERS)
        for part, a, b in zip(("err", "conv", "llr", "iter"), got, [w[:count] for w in want]):
            if part == "llr":
                a, b = CM.words(a), CM.words(b)
            assert np.array_equal(np.asarray(a), np.asarray(b)), f"{name} max_iter {max_iter}, {count} shots: {part} differs"
