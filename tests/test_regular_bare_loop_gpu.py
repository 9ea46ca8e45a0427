"""The fixed-work form of the clean regular min-sum kernel (csrc/minsum_regular.hip) runs its iteration body with every lane enabled -- the lanes of a
block that belong to no team work on a dummy region of LDS, a team without a shot on its own slot -- and, once every shot of a workgroup is frozen, the
remaining passes in a loop without freeze bookkeeping.  Neither may change a result: the fused Monte-Carlo tally under FLAG_FIXED_ITERS against the same
plan without the flag and against the C oracle, at shot counts around the S shots of a workgroup and with a partly filled last group of a second trip
of the persistent grid; a sample whose workgroups hold converged and failing shots side by side, so that some never change loops; and the decode API
under FLAG_FIXED_ITERS, bit for bit, on bb72, bb144, a (4,2)- and an (8,4)-regular graph with B = 1 and B = S + 1."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_minima_model as CM  # noqa: E402
import regular_shapes as RS  # noqa: E402

pytestmark = pytest.mark.gpu

SEED = 20261019
TALLY_P = 0.02                  # bb72 / bb144: BP failures, late convergence and convergence at iteration 1 all occur within a few thousand shots
MIXED_P, MIXED_SHOTS, MIXED_SEED, MIXED_CLIP, MIXED_BATCH = 0.02, 20000, 20261018, 6.0, 4096


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


def bb(tag):
    """-> (code, graph-like namespace for regular_shapes.syndromes, S of plan_regular)"""
    from qldpc_amd.data import load_code
    c = load_code(tag)
    ip, ix, n = c["Hx_indptr"], c["Hx_indices"], int(c["n"])
    m = len(ip) - 1
    g = SimpleNamespace(name=tag, cdeg=6, vdeg=3, m=m, n=n, indptr=ip, indices=ix, cols=np.asarray(ix).reshape(m, 6).astype(np.int64), rate=0.03)
    g.TS, g.S, g.block, g.lds = RS.plan(6, m, n)
    return c, g


def shot_counts(S):
    """around the S shots of a workgroup, and a second trip of the persistent grid whose last group holds 3 of its S shots"""
    return (1, S - 1, S, S + 1, 3 * S + 2, RS.GRID_CAP * S + S + 3)


@pytest.mark.parametrize("max_iter", [1, 2, 50])
@pytest.mark.parametrize("tag", ["bb72", "bb144"])
def test_fixed_work_tally_equals_early_exit_and_the_oracle(L, oracle, tag, max_iter):
    c, g = bb(tag)
    assert g.S == {"bb72": 14, "bb144": 7}[tag] and g.block - g.S * g.TS == 8          # 8 lanes of the block belong to no team
    graph = L.Graph(g.indptr, g.indices, g.n)
    counts = shot_counts(g.S)
    batch = 1 << 16
    assert counts[-1] <= batch and counts[-1] % g.S not in (0, 1)                      # one launch; the last group is partly filled
    plans = [(name, L.CodeCapacityPlan(graph, c["Lx"], TALLY_P, max_iter=max_iter, flags=flags, batch=batch))
             for flags, name in ((L.FLAG_FIXED_ITERS, "fixed work"), (0, "early exit"))]
    try:
        for count in counts:
            want = oracle.cc_sample_decode_tally(g.indptr, g.indices, g.n, c["Lx"], TALLY_P, SEED, 0, count, max_iter=max_iter, threads=0)
            for name, plan in plans:
                plan.run(SEED, 0, count)
                got = plan.read(clear=True)
                assert np.array_equal(got, want), f"{tag} max_iter {max_iter} {count} shots, {name}: tally {got.tolist()} != oracle {want.tolist()}"
        if max_iter == 50:
            T = L.TALLY
            assert 0 < want[T["bp_conv_z"]] < counts[-1] and want[T["iters_z"]] > want[T["trials"]]      # the largest count holds failures and late convergence
    finally:
        for _, plan in plans:
            plan.close()


def test_workgroups_that_hold_a_failure_never_change_loops(L, oracle):
    """bb72, p = 0.02, clip 6, seed 20261018, 20 000 shots (the sample of tests/test_loo_messages_gpu.py).  Counted with the oracle alone: 155 BP
    failures, 3516 shots that converge after iteration 1, 16 329 that converge at iteration 1; of the 1429 groups of S = 14 consecutive shots 148 hold
    a failure, every one of them next to converged shots.  Those workgroups stay in the loop with the freeze bookkeeping for all 50 iterations, the
    others leave it at different iterations."""
    c, g = bb("bb72")
    errors = np.array([oracle.cc_sample_errors(MIXED_SEED, b, g.n, MIXED_P) for b in range(MIXED_SHOTS)]).astype(np.int64).reshape(MIXED_SHOTS, g.n)
    prior = np.full(g.n, np.log((1 - MIXED_P) / MIXED_P))
    ref = oracle.minsum_decode_batch(g.indptr, g.indices, g.n, RS.syndromes_of(g, errors), prior, max_iter=50, clip_llr=MIXED_CLIP, threads=0)
    conv, iters = np.asarray(ref[1]).astype(bool), np.asarray(ref[3])
    failures, late = int((~conv).sum()), int((conv & (iters >= 1)).sum())
    print(f"bb72 p {MIXED_P} clip {MIXED_CLIP}: {failures} BP failures, {late} shots converge after iteration 1, of {MIXED_SHOTS}")
    assert failures >= 100 and late >= 100
    want = oracle.cc_sample_decode_tally(g.indptr, g.indices, g.n, c["Lx"], MIXED_P, MIXED_SEED, 0, MIXED_SHOTS, max_iter=50, clip_llr=MIXED_CLIP, threads=0)
    assert int(want[L.TALLY["trials"]] - want[L.TALLY["bp_conv_z"]]) == failures
    graph = L.Graph(g.indptr, g.indices, g.n)
    for flags, name in ((L.FLAG_FIXED_ITERS, "fixed work"), (0, "early exit")):
        plan = L.CodeCapacityPlan(graph, c["Lx"], MIXED_P, max_iter=50, clip_llr=MIXED_CLIP, flags=flags, batch=MIXED_BATCH)
        try:
            plan.run(MIXED_SEED, 0, MIXED_SHOTS)
            got = plan.read()
        finally:
            plan.close()
        assert np.array_equal(got, want), f"{name}: tally {got.tolist()} != oracle {want.tolist()}"


def decode_graph(tag):
    return bb(tag)[1] if tag.startswith("bb") else RS.graph(tag)


@pytest.mark.parametrize("tag", ["bb72", "bb144", "r42_m30", "r84_m24"])
def test_fixed_work_decode_equals_the_oracle(L, oracle, tag):
    """LLR words, hard decisions, verdicts and iteration counts of minsum_decode_batch under FLAG_FIXED_ITERS with one shot and with S + 1 shots (a
    second workgroup with one team that holds a shot)"""
    g = decode_graph(tag)
    assert g.S > 1 and g.block > g.S * g.TS                  # teams without a shot, and lanes without a team
    prior = np.full(g.n, np.log((1 - g.rate) / g.rate))
    graph = L.Graph(g.indptr, g.indices, g.n)
    assert L.minsum_decode_path(graph, prior, RS.MAX_ITER, "dynamical", 1.0, flags=L.FLAG_FIXED_ITERS)[0] == L.PATH_REGULAR
    for B in (1, g.S + 1):
        synd = RS.syndromes(g, B, salt=3)
        want = oracle.minsum_decode_batch(g.indptr, g.indices, g.n, synd, prior, max_iter=RS.MAX_ITER, threads=0)
        got = L.minsum_decode_batch(graph, synd, prior, RS.MAX_ITER, "dynamical", 1.0, flags=L.FLAG_FIXED_ITERS)
        for what, a, b in zip(("err", "conv", "llr", "iter"), got, want):
            if what == "llr":
                a, b = CM.words(a), CM.words(b)
            bad = np.flatnonzero((np.asarray(a) != np.asarray(b)).reshape(B, -1).any(axis=1))
            assert bad.size == 0, f"{tag} B {B}: {what} differs from the oracle on shots {bad[:8].tolist()} ({bad.size} of {B})"
