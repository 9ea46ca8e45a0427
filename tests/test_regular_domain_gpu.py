"""The regular min-sum kernel (csrc/minsum_regular.hip) over the whole domain its entry points accept, bit for bit against the C oracle: clean priors
of every kind (unique minima, negative and zero classes -- the -0.0 messages of the header comment --, values above the clip, subnormals, sums that
overflow), every team size plan_regular takes (S = 14 .. 1, a block that ends in the middle of a wave, the 512-thread team and the hand-over to the
resident kernel at 513), max_iter on both sides of the 1024 alpha values kept in LDS, batches that send a workgroup of the persistent grid on a
second `base`, and the fused Monte-Carlo plan at error rates >= 0.5 (prior +0.0 or negative), on both sides of the first-iteration pipeline's size
bound and with failures exported from a second trip.  tests/test_regular_domain_cpu.py shows with the oracle alone that every case holds converging
and failing shots.  Every decode is preceded by an assertion of the decoder form the library reports for the same arguments."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_minima_model as CM  # noqa: E402
import graph_shapes as GS  # noqa: E402
import regular_shapes as RS  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = RS.decode_cases()
_HANDLES = {}


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
    L.set_option("mc_first_iteration", 1)


def handle(L, g):
    """one graph handle per graph for the whole module"""
    if g.name not in _HANDLES:
        _HANDLES[g.name] = L.Graph(g.indptr, g.indices, g.n)
    return _HANDLES[g.name]


def forms(L):
    return ((0, "early exit"), (L.FLAG_FIXED_ITERS, "fixed work"))


def same(got, want, ctx):
    """err, conv, posterior words and iter, bit for bit; the message names the case and the first differing shots"""
    B = len(want[1])
    for what, a, b in zip(("err", "conv", "llr", "iter"), got, want):
        if what == "llr":
            a, b = CM.words(a), CM.words(b)
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape, (ctx, what, a.shape, b.shape)
        bad = np.flatnonzero((a != b).reshape(B, -1).any(axis=1))
        assert bad.size == 0, f"{ctx}: {what} differs from the oracle on shots {bad[:8].tolist()} ({bad.size} of {B})"


def decode_both_forms(L, oracle, g, synd, prior, expected, ctx, max_iter=RS.MAX_ITER, alpha_mode="dynamical", alpha=1.0, damping=1.0, clip=20.0):
    """path assertion, then the decode with flags 0 and FLAG_FIXED_ITERS against the oracle -> the oracle's outputs"""
    graph = handle(L, g)
    path = L.minsum_decode_path(graph, prior, max_iter, alpha_mode, alpha, damping=damping, clip_llr=clip)[0]
    assert path == getattr(L, "PATH_" + expected), (ctx, path, expected)
    assert GS.rule_path(g.indptr, g.indices, g.n, prior, damping=damping, max_iter=max_iter, clip=clip) == expected, ctx
    want = oracle.minsum_decode_batch(g.indptr, g.indices, g.n, synd, prior, max_iter=max_iter, alpha=alpha, alpha_mode=alpha_mode, damping=damping,
                                      clip_llr=clip, threads=0)
    for flags, name in forms(L):
        assert L.minsum_decode_path(graph, prior, max_iter, alpha_mode, alpha, damping=damping, clip_llr=clip, flags=flags)[0] == path, (ctx, name)
        got = L.minsum_decode_batch(graph, synd, prior, max_iter, alpha_mode, alpha, damping=damping, clip_llr=clip, flags=flags)
        same(got, want, f"{ctx} {name}")
    return want


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_decode_case_equals_the_oracle(L, oracle, case):
    """Prior classes x clips on the S = 14 and the S = 1 team, the uniform and the tie-free prior on every team size (the 512 / 513 pair included: both
    sides equal the oracle), a constant and a short sequence alpha, and the damped (per-edge) form on a non-uniform prior."""
    g = RS.graph(case.graph)
    prior = RS.priors(g)[case.prior]
    synd = RS.syndromes(g, case.B, prior, case.salt)
    want = decode_both_forms(L, oracle, g, synd, prior, g.expected, case.id, max_iter=case.max_iter, alpha_mode=case.alpha_mode, alpha=case.alpha,
                             damping=case.damping, clip=case.clip)
    assert 0 < int(want[1].sum()) < case.B


def test_team_limit_and_clip_sign_in_the_path_query(L):
    """the library on both sides of the 512-thread team and of clip = 0, against the restated rules (no decode)"""
    for name in ("r63_m512", "r42_m512", "r84_m512", "r63_m513", "r63_m36"):
        g = RS.graph(name)
        prior = RS.priors(g)["uniform"]
        for kw in (dict(), dict(clip=0.0), dict(clip=-1.0), dict(max_iter=1024), dict(max_iter=1025), dict(damping=0.85)):
            got = L.minsum_decode_path(handle(L, g), prior, kw.get("max_iter", RS.MAX_ITER), "dynamical", 1.0, damping=kw.get("damping", 1.0),
                                       clip_llr=kw.get("clip", 20.0))[0]
            assert got == getattr(L, "PATH_" + GS.rule_path(g.indptr, g.indices, g.n, prior, **kw)), (name, kw, got)
    assert L.minsum_decode_path(handle(L, RS.graph("r63_m512")), None, RS.MAX_ITER, "dynamical", 1.0)[0] == L.PATH_REGULAR        # device prior: the NaN-tolerant form


def test_iteration_cap(L, oracle):
    """max_iter = 1024 fills the alpha table the kernel keeps in LDS (kMaxIterLds) and is REGULAR; 1025 is not; both equal the oracle on shots that
    run every iteration"""
    g = RS.graph("r63_m36")
    prior = RS.priors(g)["uniform"]
    synd = RS.never_converging(g, oracle, prior)
    for max_iter, expected in ((1024, "REGULAR"), (1025, "RESIDENT")):
        want = decode_both_forms(L, oracle, g, synd, prior, expected, f"max_iter {max_iter}", max_iter=max_iter)
        assert not want[1].any() and (want[3] == max_iter - 1).all()


def test_second_trip_one_shot_per_workgroup(L, oracle):
    """B = 3072 + 128 on the S = 1 team: workgroups 0 .. 127 decode a second shot.  Against the oracle, and the first 3072 shots alone (no second
    trip) give what the full batch gives for them."""
    g, B, trips = RS.second_trip("r63_m257")
    pc, clip = RS.SECOND_TRIP["r63_m257"]
    prior = RS.priors(g)[pc]
    synd = RS.syndromes(g, B, prior, salt=2)
    assert g.S == 1 and B == RS.GRID_CAP + 128
    want = decode_both_forms(L, oracle, g, synd, prior, "REGULAR", f"second trip r63_m257 B {B}", clip=clip)
    conv = np.asarray(want[1]).astype(bool)
    first, second = np.array(trips).T
    assert (conv[first] != conv[second]).any()
    graph = handle(L, g)
    for flags, name in forms(L):
        full = L.minsum_decode_batch(graph, synd, prior, RS.MAX_ITER, "dynamical", 1.0, clip_llr=clip, flags=flags)
        head = L.minsum_decode_batch(graph, synd[:RS.GRID_CAP], prior, RS.MAX_ITER, "dynamical", 1.0, clip_llr=clip, flags=flags)
        same(head, tuple(np.asarray(x)[:RS.GRID_CAP] for x in full), f"first {RS.GRID_CAP} shots alone against the full batch, {name}")


def test_second_trip_many_shots_per_workgroup(L, oracle):
    """B = 3072 * 14 + 14 + 3 on the S = 14 team, posteriors included: workgroup 0 decodes a full second group, workgroup 1 a ragged one of 3 shots"""
    g, B, trips = RS.second_trip("r63_m36")
    pc, clip = RS.SECOND_TRIP["r63_m36"]
    prior = RS.priors(g)[pc]
    synd = RS.syndromes(g, B, prior, salt=2)
    assert g.S == 14 and B == RS.GRID_CAP * 14 + 14 + 3
    graph = handle(L, g)
    assert L.minsum_decode_path(graph, prior, RS.MAX_ITER, "dynamical", 1.0, clip_llr=clip)[0] == L.PATH_REGULAR
    want = oracle.minsum_decode_batch(g.indptr, g.indices, g.n, synd, prior, max_iter=RS.MAX_ITER, clip_llr=clip, threads=0)
    conv = np.asarray(want[1]).astype(bool)
    first, second = np.array(trips).T
    assert (conv[first] != conv[second]).any()
    for flags, name in forms(L):
        got = L.minsum_decode_batch(graph, synd, prior, RS.MAX_ITER, "dynamical", 1.0, clip_llr=clip, flags=flags, want_llr=True)
        same(got, want, f"second trip r63_m36 B {B} {name}")


def mc_same(L, oracle, g, p, count, ctx, clip=20.0, use_osd=True, want=None):
    """path assertion, then the plan's tally with flags 0 and FLAG_FIXED_ITERS against the oracle's: all 16 slots"""
    graph = handle(L, g)
    prior = np.full(g.n, np.log((1 - p) / p))
    assert L.minsum_decode_path(graph, prior, RS.MAX_ITER, "dynamical", 1.0, clip_llr=clip)[0] == L.PATH_REGULAR, ctx
    Lmat = RS.logicals(g)
    if want is None:
        want = oracle.cc_sample_decode_tally(g.indptr, g.indices, g.n, Lmat, p, RS.MC_SEED, 0, count, max_iter=RS.MAX_ITER, clip_llr=clip, use_osd=use_osd, threads=0)
    assert want.shape == (16,) and want[L.TALLY["trials"]] == count
    for flags, name in forms(L):
        got = L.cc_sample_decode_tally(graph, Lmat, p, RS.MC_SEED, 0, count, max_iter=RS.MAX_ITER, clip_llr=clip, use_osd=use_osd, flags=flags)
        assert np.array_equal(got, want), f"{ctx} clip {clip} osd {use_osd} {name}: tally {got.tolist()} != oracle {want.tolist()}"
    return want


@pytest.mark.parametrize("p", RS.MC_PS)
@pytest.mark.parametrize("name", RS.MC_GRAPHS)
def test_monte_carlo_plan_with_nonpositive_prior(L, oracle, name, p):
    """p >= 0.5: iteration 0 of the fused kernel is a closed form in prior0 with a sign rule for p0 < 0; p0 = +0.0 makes every message +-0.0"""
    g = RS.graph(name)
    assert oracle.bernoulli_threshold(p) == int(np.floor(p * 2.0 ** 32)) and np.log((1 - p) / p) <= 0
    for clip in RS.MC_CLIPS:
        for use_osd in (True, False):
            want = mc_same(L, oracle, g, p, RS.MC_SHOTS, f"{name} p {p}", clip=clip, use_osd=use_osd)
            if p == 0.7:
                assert 0 < want[L.TALLY["bp_conv_z"]] < RS.MC_SHOTS
            if p == 0.5:
                assert want[L.TALLY["bp_conv_z"]] == want[L.TALLY["zero_synd_z"]]


@pytest.mark.parametrize("name", ["r63_m320", "r63_m321"])
def test_monte_carlo_plan_at_the_first_iteration_bound(L, oracle, options, name):
    """(m + n) * 64 <= 60 KiB admits m = 320 to the bit-sliced first iteration and keeps m = 321 out; with the option either way the tally is the oracle's"""
    g = RS.graph(name)
    want = None
    for first in (0, 1):
        options("mc_first_iteration", first)
        want = mc_same(L, oracle, g, RS.MC_BOUND_P, RS.MC_BOUND_SHOTS, f"{name} mc_first_iteration {first}", want=want)


def test_monte_carlo_plan_exports_failures_from_a_second_trip(L, oracle, options):
    """more than 3072 shots on the S = 1 team at an error rate that leaves BP failures among the shots of the second `base`: the export of their
    records for OSD-0 runs while the workgroup is on its second trip (full decoder for every shot), and through the shot list of the first iteration"""
    g = RS.graph("r63_m257")
    assert g.S == 1 and RS.MC_TRIP_SHOTS > RS.GRID_CAP
    for use_osd in (True, False):
        want = None
        for first in (0, 1):
            options("mc_first_iteration", first)
            want = mc_same(L, oracle, g, RS.MC_TRIP_P, RS.MC_TRIP_SHOTS, f"r63_m257 mc_first_iteration {first}", use_osd=use_osd, want=want)
        assert 0 < want[L.TALLY["bp_conv_z"]] < RS.MC_TRIP_SHOTS
