"""The resident min-sum kernel (csrc/minsum_resident.hip) over every form and team shape it takes (tests/resident_shapes.py), bit for bit against the
C oracle: the four instantiations <6,3,1,2>, <6,3,2,4>, <8,4,1,2>, <8,4,2,4>, each plain, with damping and as the fused Monte-Carlo kernel; irregular
graphs in the two-rows-per-thread form (ragged and empty second row slices, empty rows, degree-1 checks, a column that meets two of them with
opposite syndrome bits); prior classes x clips, non-finite and -0.0 priors on columns of either row slice; the limits of the plan (256 / 257 rows, the
1024-thread team, 60 KiB per shot, S uncut and cut); max_iter 0 and 1; batches that end in a ragged group and batches that send a workgroup of the
4096-group grid on a second `base`.  tests/test_resident_domain_cpu.py shows with the oracle alone that the inputs hold both verdicts.

Every decode is preceded by an assertion of the path and the QLDPC_DETAIL_RES_* / QLDPC_DETAIL_DAMPING bits the library reports for the same
arguments against the plan restated in resident_shapes.plan: that is how the module knows which instantiation ran.  A Monte-Carlo call is fused (the
MC form) when damping == 1 and takes the sample / decode / judge launches through the DAMP form otherwise (qldpc_cc_plan_create).  The last test
asserts that all twelve (instantiation, form) combinations were reported."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_minima_model as CM  # noqa: E402
import graph_shapes as GS  # noqa: E402
import resident_shapes as RS  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = RS.decode_cases()
MC_CASES = RS.mc_cases()
_HANDLES = {}
REPORTED = {}                   # (instantiation, form) -> number of launches the path query announced


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


def handle(L, g):
    """one graph handle per graph for the whole module"""
    if g.name not in _HANDLES:
        _HANDLES[g.name] = L.Graph(g.indptr, g.indices, g.n)
    return _HANDLES[g.name]


def forms(L):
    return ((0, "early exit"), (L.FLAG_FIXED_ITERS, "fixed work"))


def same(got, want, ctx):
    """err, conv, posterior words (NaN payloads included) and iter, bit for bit; the message names the case and the first differing shots"""
    B = len(want[1])
    for what, a, b in zip(("err", "conv", "llr", "iter"), got, want):
        if what == "llr":
            a, b = CM.words(a), CM.words(b)
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape, (ctx, what, a.shape, b.shape)
        bad = np.flatnonzero((a != b).reshape(B, -1).any(axis=1))
        assert bad.size == 0, f"{ctx}: {what} differs from the oracle on shots {bad[:8].tolist()} ({bad.size} of {B})"


def announced(L, g, prior, ctx, max_iter=RS.MAX_ITER, alpha_mode="dynamical", alpha=1.0, damping=1.0, clip=20.0, flags=0, monte_carlo=False):
    """the library reports the resident kernel and the instantiation the restated plan gives; counts it"""
    got = L.minsum_decode_path(handle(L, g), prior, max_iter, alpha_mode, alpha, damping=damping, clip_llr=clip, flags=flags)
    inst = g.plan.inst
    assert got == (L.PATH_RESIDENT, RS.detail_of(L, inst, damping != 1.0)), (ctx, got, inst)
    assert GS.rule_path(g.indptr, g.indices, g.n, prior, damping=damping, max_iter=max_iter, clip=clip) == "RESIDENT", ctx
    form = "DAMP" if damping != 1.0 else ("MC" if monte_carlo else "plain")
    REPORTED[(inst, form)] = REPORTED.get((inst, form), 0) + 1


def decode_both_forms(L, oracle, g, synd, prior, ctx, max_iter=RS.MAX_ITER, alpha_mode="dynamical", alpha=1.0, damping=1.0, clip=20.0):
    """path and detail assertion, then the decode with flags 0 and FLAG_FIXED_ITERS against the oracle -> the oracle's outputs"""
    want = oracle.minsum_decode_batch(g.indptr, g.indices, g.n, synd, prior, max_iter=max_iter, alpha=alpha, alpha_mode=alpha_mode, damping=damping,
                                      clip_llr=clip, threads=0)
    for flags, name in forms(L):
        announced(L, g, prior, f"{ctx} {name}", max_iter, alpha_mode, alpha, damping, clip, flags)
        got = L.minsum_decode_batch(handle(L, g), synd, prior, max_iter, alpha_mode, alpha, damping=damping, clip_llr=clip, flags=flags)
        same(got, want, f"{ctx} {name}")
    return want


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_decode_case_equals_the_oracle(L, oracle, case):
    """The uniform and the tie-free prior on every graph the kernel takes; on one graph per instantiation the prior classes x clips, damping, constant
    and sequence alpha, max_iter 0 and 1, and +inf / -inf / NaN / -0.0 priors on columns of either row slice, plain and damped."""
    g = RS.graph(case.graph)
    assert g.plan.inst == g.inst
    prior = RS.prior_of(g, case)
    synd = RS.syndromes(g, case.B, prior, case.salt)
    want = decode_both_forms(L, oracle, g, synd, prior, case.id, max_iter=case.max_iter, alpha_mode=case.alpha_mode, alpha=case.alpha,
                             damping=case.damping, clip=case.clip)
    if case.max_iter > 0 and case.graph != "one_edge":               # the two exceptions: see tests/test_resident_domain_cpu.py
        assert 0 < int(want[1].sum()) < case.B


def test_the_refused_side_of_each_pair_takes_the_path_the_rules_give(L):
    """one column beyond the 1024-thread team, one row beyond the 60 KiB of a shot: not RESIDENT, and asking for it is an error"""
    for taken, refused in RS.PAIRS:
        g = RS.graph(refused)
        assert RS.graph(taken).plan is not None and g.plan is None
        prior = RS.priors(g)["uniform"]
        for kw in (dict(), dict(damping=0.85), dict(max_iter=1025)):
            want = GS.rule_path(g.indptr, g.indices, g.n, prior, **kw)
            got = L.minsum_decode_path(handle(L, g), prior, kw.get("max_iter", RS.MAX_ITER), "dynamical", 1.0, damping=kw.get("damping", 1.0))
            assert want != "RESIDENT" and got[0] == getattr(L, "PATH_" + want), (refused, kw, got, want)
            assert not got[1] & (L.DETAIL_RES_CDEG8 | L.DETAIL_RES_CPT2), (refused, kw, got)
        with pytest.raises(L.QldpcError):
            L.minsum_decode_path(handle(L, g), prior, RS.MAX_ITER, "dynamical", 1.0, flags=L.FLAG_KERNEL_GENERIC)


def test_second_trip_two_shots_per_workgroup(L, oracle):
    """B = 4096 * 2 + 2 + 1 on the S = 2 two-row team, posteriors included: workgroup 0 decodes a full second group, workgroup 1 a ragged one of one
    shot.  Against the oracle, and the first 8192 shots alone (no second trip) give what the full batch gives for them."""
    g, B, first, synd = RS.second_trip("i84_m300")
    assert g.plan.S == 2 and first == 8192 and B == first + 3
    prior = RS.priors(g)["normal"]
    want = decode_both_forms(L, oracle, g, synd, prior, f"second trip i84_m300 B {B}")
    conv = np.asarray(want[1]).astype(bool)
    assert 0 < conv[first:].sum() < B - first
    for flags, name in forms(L):
        full = L.minsum_decode_batch(handle(L, g), synd, prior, RS.MAX_ITER, "dynamical", 1.0, flags=flags)
        head = L.minsum_decode_batch(handle(L, g), synd[:first], prior, RS.MAX_ITER, "dynamical", 1.0, flags=flags)
        same(head, tuple(np.asarray(x)[:first] for x in full), f"first {first} shots alone against the full batch, {name}")


def test_second_trip_one_shot_per_workgroup(L, oracle):
    """B = 4096 + 100 on the S = 1 team of exactly 256 threads: workgroups 0 .. 99 decode a second shot"""
    g, B, first, synd = RS.second_trip("i84_m511")
    assert g.plan.S == 1 and first == RS.GRID_CAP and B == first + 100
    want = decode_both_forms(L, oracle, g, synd, RS.priors(g)["normal"], f"second trip i84_m511 B {B}")
    conv = np.asarray(want[1]).astype(bool)
    assert 0 < conv[first:].sum() < B - first


@pytest.mark.parametrize("case", MC_CASES, ids=[c.id for c in MC_CASES])
def test_monte_carlo_tally_equals_the_oracle(L, oracle, case):
    """cc_sample_decode_tally, all 16 slots: OSD-0 on and off, early exit and fixed work, a shot count that is no multiple of S from a shot_begin > 0,
    one call cut into pieces by the plan's batch, one call with failure records exported from a second trip, and damping (not fused: the DAMP form)."""
    g = RS.graph(case.graph)
    p = RS.MC_P
    prior = np.full(g.n, np.log((1 - p) / p))
    flags = L.FLAG_FIXED_ITERS if case.fixed else 0
    Lmat = RS.logicals(g)
    want = oracle.cc_sample_decode_tally(g.indptr, g.indices, g.n, Lmat, p, RS.MC_SEED, case.begin, case.count, max_iter=RS.MAX_ITER, damping=case.damping,
                                         use_osd=case.use_osd, threads=0)
    assert want.shape == (16,) and want[L.TALLY["trials"]] == case.count and 0 < want[L.TALLY["bp_conv_z"]] < case.count
    announced(L, g, prior, case.id, damping=case.damping, flags=flags, monte_carlo=True)
    if case.batch is None:
        got = L.cc_sample_decode_tally(handle(L, g), Lmat, p, RS.MC_SEED, case.begin, case.count, max_iter=RS.MAX_ITER, damping=case.damping,
                                       use_osd=case.use_osd, flags=flags)
    else:
        plan = L.CodeCapacityPlan(handle(L, g), Lmat, p, max_iter=RS.MAX_ITER, damping=case.damping, use_osd=case.use_osd, flags=flags, batch=case.batch)
        try:
            plan.run(RS.MC_SEED, case.begin, case.count)
            got = plan.read()
        finally:
            plan.close()
    assert np.array_equal(got, want), f"{case.id}: tally {np.asarray(got).tolist()} != oracle {want.tolist()}"


def test_all_twelve_instantiations_were_reported():
    """runs last: over the module, the path query announced every (instantiation, form) of the kernel at least once"""
    print("resident launches announced:", {f"<{','.join(map(str, i))}> {f}": REPORTED.get((i, f), 0) for i in RS.INSTANCES for f in RS.FORMS})
    missing = [(i, f) for i in RS.INSTANCES for f in RS.FORMS if not REPORTED.get((i, f))]
    assert not missing, missing
