"""The inputs of tests/test_regular_early_columns_gpu.py, proven with the oracle alone (no GPU).

For every max_iter under test the first workgroup of every decode batch holds a shot that never converges and one each that converges at iteration 0,
at iteration 1 and later, as far as that max_iter can reach them (regular_early_columns_cases.expected_classes); the Monte-Carlo calls at the low rate
converge on every shot, so every workgroup freezes all its shots at pass 1 and leaves through the bare loop, and at the high rate the twenty workgroups
hold BP failures, with and without the OSD export."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regular_early_columns_cases as OC  # noqa: E402

TALLY_TRIALS, TALLY_BP_CONV_Z = 0, 4        # include/qldpc_hip.h: QLDPC_TALLY_TRIALS, QLDPC_TALLY_BP_CONV_Z


@pytest.mark.parametrize("name", list(OC.SHAPES))
def test_the_first_workgroup_of_every_decode_batch_holds_every_class(oracle, name):
    ip, ix, m, n, S, _ = OC.code(name)
    prior, synd = OC.decode_inputs(name, oracle)
    assert np.unique(prior).size > 1 and np.isfinite(prior).all() and (prior > 0).all()          # non-uniform and clean
    assert synd.shape == (20 * S, m)
    for max_iter in OC.ITERS:
        _, conv, _, iters = oracle.minsum_decode_batch(ip, ix, n, synd, prior, max_iter=max_iter, threads=0)
        for count in OC.counts(S):
            head = min(count, S)                                                                 # the first workgroup's shots
            assert OC.classes(conv[:head], iters[:head]) == OC.expected_classes(max_iter), (name, max_iter, count)
        assert not conv[0] and iters[0] == max_iter - 1                                          # kernels.py:267


@pytest.mark.parametrize("name", list(OC.SHAPES))
def test_the_monte_carlo_rates_reach_both_exits(oracle, name):
    ip, ix, m, n, S, Lmat = OC.code(name)
    for max_iter in (2, 50):
        for count in OC.counts(S):
            low = oracle.cc_sample_decode_tally(ip, ix, n, Lmat, OC.LOW, OC.SEED, 0, count, max_iter=max_iter, threads=0)
            assert low[TALLY_TRIALS] == count and low[TALLY_BP_CONV_Z] == count, (name, max_iter, count, low.tolist())
        for use_osd in (True, False):
            high = oracle.cc_sample_decode_tally(ip, ix, n, Lmat, OC.HIGH, OC.SEED, 0, 20 * S, max_iter=max_iter, use_osd=use_osd, threads=0)
            assert 0 < high[TALLY_BP_CONV_Z] < 20 * S, (name, max_iter, use_osd, high.tolist())
