"""CPU side of the resident kernel's domain suite (tests/resident_shapes.py).  (a) csrc/resident_plan.h, compiled into tests/resident_plan_main.cpp,
equals the plan restated in resident_shapes.plan over a sweep that holds refusals of every kind and S > 1; (b) the kernel's carve of the dynamic LDS,
restated from its pointer arithmetic, ends inside the planned size at every point; (c) every table graph has the structure and the plan it is named
for, and the two sides of a pair differ only as stated; (d) the C oracle alone finds in the inputs what the GPU module needs to see: converging and
failing shots in every decode case, NaN posteriors where the priors or the graph make them, BP failures for OSD-0 in the Monte-Carlo cases and both
verdicts on the second `base` of the second-trip batches.  Nothing is skipped or filtered.

Two kinds of decode case cannot hold both verdicts, whatever the inputs, and assert the one they have instead:
  * max_iter = 0: no iteration runs, the syndrome test of iteration k belongs to iteration k + 1, so no shot converges (conv = 0, iter = -1,
    posteriors 0) -- the case is about that exit;
  * `one_edge` (one check on one column): the check's message is +-inf with the sign the syndrome bit asks for, so the first hard decision satisfies
    it for either bit and any finite prior: every shot converges at iteration 0."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_shapes as GS  # noqa: E402
import resident_shapes as RS  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "qldpc-branched-off_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CASES = RS.decode_cases()
MC_CASES = RS.mc_cases()
T = {"trials": 0, "z_err": 1, "bp_conv_z": 4, "osd_z": 6, "iters_z": 8, "zero_synd_z": 10, "unsat_z": 12}      # slots of the tally (include/qldpc_hip.h)
DEGREE_CAPS = ((6, 3), (6, 4), (7, 3), (8, 4), (9, 4), (8, 5))


def sweep():
    """(m, n, nnz, max row degree, max column degree): m 1 .. 80 and around every limit of the plan, n in {m, 2m, 2m +- 1, 4m, 8m}, the degree caps on
    both sides of (6,3) / (8,4) / refused, and a few degenerate points"""
    ms = list(range(1, 81))
    for c in (128, 256, 257, 512, 682, 829, 1024, 2047):
        ms += [c - 1, c, c + 1]
    pts = [(m, n, 2 * m, rd, cd) for m in sorted(set(ms)) for n in sorted({m, 2 * m, 2 * m - 1, 2 * m + 1, 4 * m, 8 * m}) for rd, cd in DEGREE_CAPS]
    pts += [(0, 5, 1, 3, 3), (5, 0, 1, 3, 3), (5, 5, 0, 0, 0), (438, 4096, 2520, 6, 3), (438, 4097, 2520, 6, 3), (10, 200, 58, 6, 3), (1, 1, 1, 1, 1)]
    return pts


@pytest.fixture(scope="module")
def compiled_plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("resident_plan") / "resident_plan_main")
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-I", CSRC, os.path.join(HERE, "resident_plan_main.cpp"), "-o", exe], check=True)
    pts = sweep()
    out = subprocess.run([exe], input="".join("%d %d %d %d %d\n" % p for p in pts), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(pts)
    return pts, [tuple(int(x) for x in line.split()) for line in out]


def test_compiled_plan_equals_the_restated_plan(compiled_plan):
    pts, got = compiled_plan
    taken = cut = 0
    refused = {"degree": 0, "bytes": 0, "team": 0, "empty": 0}
    seen = set()
    for pt, g in zip(pts, got):
        m, n, nnz, rd, cd = pt
        p = RS.plan(*pt)
        want = (0,) if p is None else (1,) + p.inst + (p.TS, p.S, p.block, p.lds)
        assert g == want, (pt, g, want)
        # the second restatement of the take / refuse rule (graph_shapes.resident_takes) agrees
        assert GS.resident_takes(m, n, nnz, np.array([rd]), np.array([cd])) == (p is not None), pt
        if p is None:
            if min(m, n, nnz) <= 0:
                refused["empty"] += 1
            elif rd > 8 or cd > 4:
                refused["degree"] += 1
            elif 8 * (m * (7 if rd <= 6 and cd <= 3 else 9) + n) + 32 + (n + 3) // 4 * 4 > RS.SHOT_BYTES:
                refused["bytes"] += 1
            else:
                refused["team"] += 1
        else:
            taken += 1
            cut += 1 < p.S < p.uncut
            seen.add(p.inst)
    print(f"{len(pts)} points: {taken} taken ({cut} with 1 < S < 1024 // TS), refused {refused}")
    assert seen == set(RS.INSTANCES) and cut >= 10 and all(v >= 1 for v in refused.values()), (seen, cut, refused)
    assert any(p is not None and p.S > 1 and p.S == p.uncut for p in (RS.plan(*pt) for pt in pts))


def test_kernel_carve_ends_inside_the_planned_lds(compiled_plan):
    pts, got = compiled_plan
    for pt, g in zip(pts, got):
        if g[0]:
            m, n = pt[:2]
            cdeg, TS, S, block, lds = g[1], g[5], g[6], g[7], g[8]
            assert RS.carve_end(m, n, cdeg, S) <= lds <= RS.LDS_BUDGET, (pt, g)
            assert block <= 1024 and block % 64 == 0 and S * TS <= block < S * TS + 64 and 1 <= S <= block, (pt, g)
            assert g[3] * TS >= m and g[4] * TS >= n, (pt, g)                  # cpt rows and vpt columns per thread cover the graph


def test_table_graphs_have_the_structure_and_plan_they_are_named_for():
    G = {name: RS.graph(name) for name in RS.TABLE}
    for name, g in G.items():
        m, n, cap = RS.TABLE[name][:3]
        rd, cd = GS.degrees(g.indptr, g.indices, g.n)
        assert (g.m, g.n) == (m, n) and g.indptr.dtype == np.int32 and g.indices.dtype == np.int32 and rd.max() <= cap, name
        for i in range(m):
            row = g.indices[g.indptr[i]:g.indptr[i + 1]]
            assert (np.diff(row) > 0).all() and (len(row) == 0 or (0 <= row[0] and row[-1] < n)), (name, i)
        assert (g.plan is not None) == (g.inst is not None) == GS.resident_takes(m, n, g.nnz, rd, cd), name
        pr = np.full(n, 3.0)
        assert (GS.rule_path(g.indptr, g.indices, n, pr) == "RESIDENT") == (g.inst is not None), name
        if g.inst is not None:
            assert g.plan.inst == g.inst and RS.carve_end(m, n, g.inst[0], g.plan.S) <= g.plan.lds, name
        if name not in RS.PLAIN and RS.TABLE[name][3] is not None:
            assert (rd == 0).sum() >= 1 and (rd == 1).sum() >= 1 and (cd == 0).sum() >= 1 and rd.max() == cap, name
            assert rd[1] >= 2 and np.array_equal(g.H[1], g.H[m - 2]), name                   # the duplicated row
            assert rd[0] == 1 and rd[m - 1] == 1 and g.indices[g.indptr[0]] != g.indices[g.indptr[m - 1]], name
    P = {name: g.plan for name, g in G.items()}
    shape = lambda p: (p.inst, p.TS, p.S, p.uncut, p.block, p.idle)      # noqa: E731
    assert shape(P["i63_m256"]) == ((6, 3, 1, 2), 256, 3, 4, 768, 0)
    assert shape(P["i63_m257"]) == ((6, 3, 2, 4), 129, 3, 7, 448, 61)
    g = G["i63_wide"]
    assert shape(g.plan) == ((6, 3, 2, 4), 129, 6, 7, 832, 58) and g.m <= g.plan.TS < (g.n + 1) // 2            # no row in any second slice
    assert shape(P["i63_tall"]) == ((6, 3, 2, 4), 300, 1, 3, 320, 20) and (G["i63_tall"].n + 3) // 4 < 300
    assert shape(P["i63_team1024"]) == ((6, 3, 2, 4), 1024, 1, 1, 1024, 0) and P["i63_team1024"].per_shot == RS.SHOT_BYTES - 16 == 61424
    assert shape(P["i84_m70"]) == ((8, 4, 1, 2), 75, 10, 13, 768, 18)
    assert shape(P["i84_m300"]) == ((8, 4, 2, 4), 150, 2, 6, 320, 20)
    assert shape(P["i84_m511"]) == ((8, 4, 2, 4), 256, 1, 4, 256, 0) and G["i84_m511"].m % 2 == 1 and G["i84_m511"].n % 2 == 1
    assert shape(P["uncut"]) == ((6, 3, 1, 2), 100, 10, 10, 1024, 24)
    assert shape(P["one_edge"]) == ((6, 3, 1, 2), 1, 654, 1024, 704, 50) and G["one_edge"].nnz == 1
    # the (8,4) instance by a column degree alone and by a row degree alone
    assert G["i84_bycol"].row_deg.max() == 6 and G["i84_bycol"].col_deg.max() == 4 and P["i84_bycol"].inst == (8, 4, 1, 2)
    assert G["i84_byrow"].row_deg.max() == 7 and G["i84_byrow"].col_deg.max() == 3 and P["i84_byrow"].inst == (8, 4, 1, 2)
    # the two-row graphs with rows in their second slice have an empty row, a degree-1 check and a longer row in either slice
    for name in ("i63_m257", "i63_tall", "i63_bytes_in", "i84_bytes_in", "i84_m300", "i84_m511"):
        g = G[name]
        sl = np.arange(g.m) // g.plan.TS
        assert set(sl) == {0, 1} and g.plan.inst[2] == 2, name
        for c in (0, 1):
            assert {0, 1} <= set(g.row_deg[sl == c]) and g.row_deg[sl == c].max() >= 3, (name, c)
        assert (sl == 1).sum() < g.plan.TS or g.m == 2 * g.plan.TS, name
    assert (np.arange(G["i63_m257"].m) // 129 == 1).sum() == 128                                # a ragged second slice: 128 rows on 129 threads
    # the pairs: the same edges, plus one column of degree 0 resp. one row of degree 2 on two new columns
    a, b = G["i63_team1024"], G["i63_team1025"]
    assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and b.n == a.n + 1 and b.col_deg[-1] == 0
    assert (b.n + 3) // 4 == RS.TEAM + 1 and 8 * (b.m * 7 + b.n) + 32 + (b.n + 3) // 4 * 4 <= RS.SHOT_BYTES          # refused by the team alone
    for small, big, per_row in (("i63_bytes_in", "i63_bytes_out", 74), ("i84_bytes_in", "i84_bytes_out", 90)):
        a, b = G[small], G[big]
        assert (b.m, b.n) == (a.m + 1, a.n + 2) and np.array_equal(b.H[:a.m, :a.n], a.H) and not b.H[:a.m, a.n:].any(), small
        assert b.H[a.m].nonzero()[0].tolist() == [a.n, a.n + 1], small
        # per_row * m + 32 bytes per shot with n = 2 m, the error bytes rounded up to whole words
        per_shot = lambda g: per_row * g.m + 32 + (-g.n) % 4      # noqa: E731
        assert a.plan.per_shot == per_shot(a) <= RS.SHOT_BYTES < per_shot(b) and a.n == 2 * a.m and b.n == 2 * b.m, small
        assert max(-(-b.m // 2), -(-b.n // 4)) <= RS.TEAM, small                                  # refused by the bytes alone
    # one column meets two degree-1 checks, pinned to opposite syndrome bits
    g = G[RS.NAN_GRAPH]
    (r0, b0), (r1, b1) = sorted(g.pinned.items())
    assert g.row_deg[r0] == g.row_deg[r1] == 1 and g.indices[g.indptr[r0]] == g.indices[g.indptr[r1]] and b0 != b1
    assert RS.slice_of(g, r0) != RS.slice_of(g, r1)
    for name in RS.FULL_GRAPHS + RS.MC_GRAPHS + tuple(RS.SECOND_TRIP) + (RS.MC_PIECES[0], RS.MC_TRIP[0]):
        assert G[name].inst is not None
    for g in G.values():
        if g.plan is not None and g.plan.S > 1:
            assert RS.batch(g) % g.plan.S != 0, g.name


@pytest.mark.parametrize("name", RS.FULL_GRAPHS)
def test_prior_classes_have_the_property_they_are_named_for(name):
    g = RS.graph(name)
    P = RS.priors(g)
    assert tuple(P) == RS.PRIOR_CLASSES
    for k, pr in P.items():
        assert pr.shape == (g.n,) and pr.dtype == np.float64 and GS.prior_is_clean(pr), k
        assert np.array_equal(pr.view(np.uint64), RS.priors(g)[k].view(np.uint64)), k       # deterministic
    assert len(np.unique(np.abs(P["normal"]))) == g.n
    assert (P["negative class"] == -1.5).sum() == g.n // 9 and (P["zero class"] == 0).sum() == g.n // 9 and (P["above clip"] == 27.0).sum() == g.n // 7
    assert (P["subnormal"] == 5e-324).sum() == 3 and (P["subnormal"] == 1e-310).sum() == 3
    j = RS.overflow_column(g)
    rows = np.flatnonzero(g.H[:, j])
    assert len(rows) >= 3 and P["huge"][j] == 4.0 and all((P["huge"][np.setdiff1d(np.flatnonzero(g.H[i]), [j])] == 1.5e308).all() for i in rows)
    # the non-clean prior: one of each value on a column of a row of either slice
    cols = RS.not_clean_columns(g)
    pr = RS.not_clean_prior(g)
    slices = 2 if g.m > g.plan.TS else 1
    assert cols.shape == (4, slices) and len(set(cols.ravel().tolist())) == 4 * slices and not GS.prior_is_clean(pr)
    for c in range(slices):
        assert np.isposinf(pr[cols[0, c]]) and np.isneginf(pr[cols[1, c]]) and np.isnan(pr[cols[2, c]]) and pr[cols[3, c]] == 0 and np.signbit(pr[cols[3, c]])
        for j in cols[:, c]:
            assert (np.flatnonzero(g.H[:, j]) // g.plan.TS == c).any(), (name, j, c)
    assert (~np.isfinite(pr)).sum() == 3 * slices
    assert (slices == 2) == (g.plan.inst[2] == 2)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_decode_case_has_both_outcomes(oracle, case):
    g = RS.graph(case.graph)
    prior = RS.prior_of(g, case)
    synd = RS.syndromes(g, case.B, prior, case.salt)
    assert synd.shape == (case.B, g.m) and not synd[-1].any() and (case.B % g.plan.S != 0 or g.plan.S == 1)
    err, conv, llr, iters = oracle.minsum_decode_batch(g.indptr, g.indices, g.n, synd, prior, max_iter=case.max_iter, alpha=case.alpha,
                                                       alpha_mode=case.alpha_mode, damping=case.damping, clip_llr=case.clip, threads=0)
    print(f"{case.id}: {int(conv.sum())} of {case.B} shots converge, iterations up to {int(iters.max()) + 1}, {int(np.isnan(llr).sum())} NaN posteriors, "
          f"{int(np.isinf(llr).sum())} infinite ones")
    if case.max_iter == 0:
        assert not conv.any() and (iters == -1).all() and not llr.any() and not err.any()
        return
    if case.graph == "one_edge":
        assert conv.all() and (iters == 0).all() and np.array_equal(err[:, 0], synd[:, 0])
        return
    assert 0 < int(conv.sum()) < case.B, "the syndromes should hold converging and failing shots"
    if case.prior == "not clean":
        cols = RS.not_clean_columns(g)
        assert np.isnan(llr[:, cols[2]]).all()                                              # a NaN prior: a NaN posterior on every shot
        assert np.isinf(llr[:, cols[0]]).all() or np.isnan(llr[:, cols[0]]).any()           # +-inf priors stay infinite (or meet an opposite infinity)
        assert np.isinf(llr[:, cols[1]]).all() or np.isnan(llr[:, cols[1]]).any()
    elif case.graph == RS.NAN_GRAPH:
        j = g.indices[g.indptr[0]]
        assert np.isnan(llr[0:-1:2, j]).all() and not np.isnan(llr[1::2]).any()             # the pinned shots: +inf and -inf into one posterior
    else:
        assert not np.isnan(llr).any()
    if case.prior == "huge":
        assert np.isinf(llr[:, RS.overflow_column(g)]).any()


@pytest.mark.parametrize("name", sorted(RS.SECOND_TRIP))
def test_second_trip_holds_both_verdicts(oracle, name):
    """A workgroup's second `base` reuses unsat, active, the message registers and `done`: the shots of the second trip converge and fail, and differ
    in verdict from the shots the same (workgroup, slot) decoded first."""
    g, B, first, synd = RS.second_trip(name)
    assert first == RS.GRID_CAP * g.plan.S and first < B <= 2 * first and synd.shape == (B, g.m)
    assert g.plan.S == 1 or (B - first) % g.plan.S != 0                                      # the last group of the second trip is ragged
    conv = np.asarray(oracle.minsum_decode_batch(g.indptr, g.indices, g.n, synd, RS.priors(g)["normal"], max_iter=RS.MAX_ITER, threads=0)[1]).astype(bool)
    print(f"{name}: B {B}, {int(conv.sum())} converge; of the {B - first} shots of the second trip {int(conv[first:].sum())}")
    assert 0 < conv[first:].sum() < B - first and 0 < conv[:first].sum() < first
    assert (conv[first:] != conv[:B - first]).any()


@pytest.mark.parametrize("case", MC_CASES, ids=[c.id for c in MC_CASES])
def test_monte_carlo_case_has_failures_for_osd(oracle, case):
    g = RS.graph(case.graph)
    assert case.count % g.plan.S != 0 or g.plan.S == 1
    assert case.begin > 0 and (case.batch is None or case.batch < case.count)
    t = oracle.cc_sample_decode_tally(g.indptr, g.indices, g.n, RS.logicals(g), RS.MC_P, RS.MC_SEED, case.begin, case.count, max_iter=RS.MAX_ITER,
                                      damping=case.damping, use_osd=case.use_osd, threads=0)
    print(f"{case.id}: {t[T['bp_conv_z']]} of {t[T['trials']]} converge, {t[T['zero_synd_z']]} zero syndromes, {t[T['z_err']]} logical errors, "
          f"{t[T['osd_z']]} through OSD-0, {t[T['unsat_z']]} left unsatisfied")
    assert t[T["trials"]] == case.count and 0 < t[T["bp_conv_z"]] < case.count
    assert t[T["osd_z"]] == (case.count - t[T["bp_conv_z"]] if case.use_osd else 0)
    if case.graph == RS.MC_TRIP[0] and case.count > RS.GRID_CAP:
        # BP failures among the shots of the second `base`, and converging ones
        lo = oracle.cc_sample_decode_tally(g.indptr, g.indices, g.n, RS.logicals(g), RS.MC_P, RS.MC_SEED, case.begin + RS.GRID_CAP, case.count - RS.GRID_CAP,
                                           max_iter=RS.MAX_ITER, threads=0)
        assert g.plan.S == 1 and 0 < lo[T["bp_conv_z"]] < case.count - RS.GRID_CAP and lo[T["osd_z"]] > 0
