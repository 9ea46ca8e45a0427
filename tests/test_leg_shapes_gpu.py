"""BP with guided decimation (csrc/decimation.hip) and the leg and launch it shares with Relay-BP (csrc/bp_leg.h) on the cases of tests/leg_shapes.py:
every decode is bit-identical to the numpy model (tests/decimation_model.py, tests/relay_model.py), the accept / refuse lines of both LDS counts are
where the restated rules put them, the atomic queue hands a workgroup a second shot (B above any grid), the device entry takes a NULL rounds / fixed
pair, and max_rounds = 0 is Relay-BP without memory on a graph whose posteriors hold NaN.

What is observed and what is not: the lines between "posteriors in global memory" and "refused" (decim_vg_last / decim_refused, relay_vg_last /
relay_refused) are observed directly, by the return code.  The ABI does not report whether the posteriors live in LDS or in global memory, so on
the other two lines (decim_lds_last / _first, relay_lds_last / _first) this module asserts bit-equality with the model on both sides and nothing
else: a limit that moved by a few columns would go unnoticed there as long as both forms stay correct."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import leg_shapes as LS  # noqa: E402
import relay_model as RM  # noqa: E402
from test_decimation_gpu import assert_same  # noqa: E402
from test_relay_gpu import PARAM_SETS  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = LS.all_cases()
BY_NAME = {c.name: c for c in CASES}
DECIM_CASES = [c.name for c in CASES if LS.modes(c)[0]]
RELAY_CASES = [c.name for c in CASES if c.relay_here and LS.modes(c)[1]]
_GRAPHS = {}


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


def graph_of(L, c):
    """one handle per family for the whole module"""
    if c.name not in _GRAPHS:
        _GRAPHS[c.name] = L.Graph(c.indptr, c.indices, c.n)
    return _GRAPHS[c.name]


def test_the_parameter_sets_and_the_case_lists_are_the_stated_ones():
    assert LS.RELAY_SCALED == PARAM_SETS["scaled"]
    assert sorted(tuple(p[k] for k in ("alpha", "clip_llr", "t_round", "max_rounds", "per_round", "fix_llr")) for p in LS.DECIM_SETS.values()) == \
        [(0.625, 6.5, 6, 3, 7, 1000.0), (0.875, 20.0, 3, 4, 64, 25.0), (1.0, 20.0, 1, 40, 1, 5.0)]
    refused = {"decim_refused", "relay_vg_last", "relay_refused"}
    assert set(DECIM_CASES) == set(BY_NAME) - refused
    # Relay-BP here: what tests/test_wg_shapes_gpu.py does not decode (the families of the table kernel and of the small-graph forms) and the new ones
    import graph_shapes as GS
    there = {c.name for c in GS.families() if c.relay}
    assert set(RELAY_CASES) == set(BY_NAME) - there - {"relay_refused"} and not (set(RELAY_CASES) & there)
    assert {"rowdeg48", "rowdeg56", "hub_col", "hub_row", "block_513_4096", "vglobal_beyond_plain", "lds_wg", "regular63", "reg63_m512", "reg63_m513",
            "small_irregular", "relay_vg_last", "decim_refused", "n1", "ties_1024"} <= set(RELAY_CASES)


@pytest.mark.parametrize("name", DECIM_CASES)
def test_decimation_equals_the_model(L, name):
    """all six outputs, every prior of the family, the three parameter sets, B = 4 (an unrealisable syndrome, two of random errors, an all-zero one)"""
    c = BY_NAME[name]
    g, synd = graph_of(L, c), LS.syndromes(c)
    for pn, prior in c.priors.items():
        for sn, p in LS.DECIM_SETS.items():
            ref, _ = LS.decim_reference(c, pn, sn)
            assert_same(L.decim_decode_batch(g, synd, prior, **p), ref, f"{name} / {pn} / {sn}")


@pytest.mark.parametrize("name", RELAY_CASES)
def test_relay_bp_equals_the_model(L, name):
    c = BY_NAME[name]
    g, synd = graph_of(L, c), LS.syndromes(c)
    for pn, prior in c.priors.items():
        got = L.relay_decode_batch(g, synd, prior, *LS.RELAY_CALL, **LS.RELAY_SCALED)
        with np.errstate(invalid="ignore"):
            ref = RM.relay_decode(c.indptr, c.indices, c.n, synd, prior, *LS.RELAY_CALL, **LS.RELAY_SCALED)
        for a, b, what in zip(got, ref, ("err", "conv", "legs", "iters", "solutions")):
            assert np.array_equal(a, b), (name, pn, what)


def test_refusals_are_where_the_two_counts_put_them(L):
    p = LS.DECIM_SETS["3x4x64"]
    for name in ("decim_refused", "relay_vg_last", "relay_refused"):
        c = BY_NAME[name]
        assert LS.modes(c)[0] == 0
        with pytest.raises(L.QldpcError, match=r"error -4: .*row degree"):       # QLDPC_ERR_UNSUPPORTED
            L.decim_decode_batch(graph_of(L, c), LS.syndromes(c), c.priors["three values"], **p)
    c = BY_NAME["relay_refused"]
    assert LS.modes(c)[1] == 0
    with pytest.raises(L.QldpcError, match=r"error -4: .*row degree"):
        L.relay_decode_batch(graph_of(L, c), LS.syndromes(c), c.priors["three values"], *LS.RELAY_CALL, **LS.RELAY_SCALED)
    # the last sizes on the accepted side decode (and equal their models: test_decimation_equals_the_model, test_relay_bp_equals_the_model)
    assert "decim_vg_last" in DECIM_CASES and "relay_vg_last" in RELAY_CASES and "decim_refused" in RELAY_CASES
    c = BY_NAME["decim_vg_last"]
    assert L.decim_decode_batch(graph_of(L, c), LS.syndromes(c), c.priors["three values"], **p)[4].min() >= 1
    c = BY_NAME["relay_vg_last"]
    assert L.relay_decode_batch(graph_of(L, c), LS.syndromes(c), c.priors["three values"], *LS.RELAY_CALL, **LS.RELAY_SCALED)[2].min() >= 1


@pytest.mark.parametrize("name", ["n63", "ties_512"])
def test_the_queue_hands_out_a_second_shot(L, name):
    """B = 1500 is above the largest grid (256 compute units x at most 4 workgroups of 512 threads would be 1024; these two run 512 threads): some
    workgroup takes a second shot from the atomic queue and must start it from clean planes, flags and candidates.  The 1500 syndromes are the four
    of the case in 375 different orders, so every row has a model row and a B = 4 row to equal."""
    c = BY_NAME[name]
    assert LS.block_threads(c.m, c.n) == 512
    g, synd = graph_of(L, c), LS.syndromes(c)
    order = np.concatenate([np.random.default_rng([c.seed, k]).permutation(LS.B) for k in range(375)])
    assert order.size == 1500 and len({tuple(order[i:i + 4]) for i in range(0, 1500, 4)}) > 12
    for pn, prior in c.priors.items():
        for sn, p in LS.DECIM_SETS.items():
            ref, _ = LS.decim_reference(c, pn, sn)
            small = L.decim_decode_batch(g, synd, prior, **p)
            big = L.decim_decode_batch(g, synd[order], prior, **p)
            assert_same(big, [a[order] for a in ref], f"{name} / {pn} / {sn}: B = 1500 against the model")
            assert_same(big, [a[order] for a in small], f"{name} / {pn} / {sn}: B = 1500 against B = 4")


@pytest.mark.parametrize("name", ["decim_lds_first", "m1025"])
def test_device_entry_with_null_rounds_and_fixed(L, name):
    c = BY_NAME[name]
    g, synd = graph_of(L, c), LS.syndromes(c)
    dev = torch.device("cuda:0")
    pn, prior = next(iter(c.priors.items()))
    ds, dp = torch.from_numpy(np.ascontiguousarray(synd)).to(dev), torch.from_numpy(np.ascontiguousarray(prior)).to(dev)
    for sn, p in LS.DECIM_SETS.items():
        ref, _ = LS.decim_reference(c, pn, sn)
        for with_counts in (False, True):
            err, llr, conv, iters, rounds, fixed = (torch.zeros((LS.B, c.n), dtype=torch.int8, device=dev), torch.zeros((LS.B, c.n), dtype=torch.float64, device=dev),
                                                    torch.zeros(LS.B, dtype=torch.uint8, device=dev), torch.zeros(LS.B, dtype=torch.int32, device=dev),
                                                    torch.full((LS.B,), -7, dtype=torch.int32, device=dev), torch.full((LS.B,), -7, dtype=torch.int32, device=dev))
            L.check(L.lib().qldpc_decim_decode_batch_dev(g.handle, LS.B, ds.data_ptr(), dp.data_ptr(), p["alpha"], p["clip_llr"], p["t_round"], p["max_rounds"],
                                                         p["per_round"], p["fix_llr"], err.data_ptr(), llr.data_ptr(), conv.data_ptr(), iters.data_ptr(),
                                                         rounds.data_ptr() if with_counts else None, fixed.data_ptr() if with_counts else None,
                                                         C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
            torch.cuda.synchronize(dev)
            got = [t.cpu().numpy() for t in (err, llr, conv, iters, rounds, fixed)]
            if with_counts:
                assert_same(got, ref, f"{name} / {sn}: device entry")
            else:
                assert_same(got[:4], ref[:4], f"{name} / {sn}: device entry, rounds = fixed = NULL")
                assert (got[4] == -7).all() and (got[5] == -7).all()           # ... and nothing was written in their place


def test_no_rounds_is_relay_without_memory_with_nan_marginals(L):
    """step 7 of the header without a circuit: on deg1_shared two degree-1 checks disagree on a column, its marginal is inf - inf, and the NaN rides
    through the shared leg of both kernels"""
    c = BY_NAME["deg1_shared"]
    g, synd = graph_of(L, c), LS.syndromes(c)
    nan = 0
    for pn, prior in c.priors.items():
        err, llr, conv, iters, rounds, fixed = L.decim_decode_batch(g, synd, prior, alpha=0.875, clip_llr=20.0, t_round=30, max_rounds=0, per_round=8, fix_llr=50.0)
        rerr, rconv, rlegs, riters, _ = L.relay_decode_batch(g, synd, prior, 5, 0, 2, alpha=0.875, gamma0=0.0, t0=30, max_legs=0, stop_after=1)
        assert err.tobytes() == rerr.tobytes() and conv.tobytes() == rconv.tobytes() and iters.tobytes() == riters.tobytes(), pn
        assert (rounds == 1).all() and (rlegs == 1).all() and (fixed == 0).all() and np.array_equal(err, (llr < 0.0).astype(np.int8))
        nan += int(np.isnan(llr).any(axis=1).sum())
    assert nan >= 1
