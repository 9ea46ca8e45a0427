"""The OSD-w cases of tests/osdw_shapes.py hold what they are named for (no GPU: the independent model of tests/osdw_model.py, the oracle and plain
arithmetic only).  The model equals the 44 solutions the reference returned (tests/golden/osdw.npz) and the oracle on every case of at most
osdw_shapes.MODEL_MAX = 5000 candidates per shot; the three capacity cases above that (65535 and 65536 candidates) stay with the oracle alone, here and in
tests/test_osdw_domain_gpu.py.  Each deliberate mistake of osdw_model.MISTAKES that CAN change an answer changes one of the table's.

Three of the listed mistakes cannot, and the module says why instead of pretending:
  * "le_valid", "valid_needs_metric": no candidate of a sweep is ever valid (the sweep runs only for syndromes outside the column space), so the valid
    branches never fire through performOSD_enhanced -- test_no_candidate_of_a_sweep_is_ever_valid holds that over the table and the reference cases, and
    test_selection_rule_on_made_up_lists checks those branches of the model against the rule as stated;
  * "wmax_is_order": a weight class above K is empty under itertools.combinations and has C(K, w) = 0 members in a rank / unrank enumeration alike."""
import numpy as np
import pytest

import osdw_model as M
import osdw_shapes as S

OBSERVABLE = ("maxc_plus_one", "maxc_minus_one", "colex", "le_invalid", "unstable_second_sort", "nan_first", "all_columns", "stale_eperm", "first_candidate_free")
UNOBSERVABLE = ("wmax_is_order", "le_valid", "valid_needs_metric")
# where each mistake is looked for (a mistake is rejected if ANY of these answers changes)
WHERE = {
    "maxc_plus_one": ("cut_1", "cut_c1m", "cut_c1", "cut_c1p", "cut_256"), "maxc_minus_one": ("cut_1", "cut_c1m", "cut_c1", "cut_c1p", "cut_256", "cut_257"),
    "colex": ("cut_c1p", "cut_256", "cut_257"), "le_invalid": ("sel_tie",), "unstable_second_sort": ("k_cut_tie",), "nan_first": ("in_nonfinite",),
    "all_columns": ("k_exact", "sel_deep", "n64"), "stale_eperm": ("trips_small", "trips_ordering"), "first_candidate_free": ("sel_none",),
}


def test_the_mistakes_are_all_accounted_for():
    assert set(OBSERVABLE) | set(UNOBSERVABLE) == set(M.MISTAKES) and not set(OBSERVABLE) & set(UNOBSERVABLE)
    assert set(WHERE) == set(OBSERVABLE) and len(OBSERVABLE) >= 8


def test_model_equals_the_44_reference_solutions(golden):
    """with the ordering the reference's argsort produced (its tie order is the reference's own)"""
    from conftest import osdw_cases
    cases = osdw_cases(golden("osdw"))
    assert len(cases) == 44
    swept = 0
    for c in cases:
        H = np.asarray(c["H"].todense(), np.uint8)
        sol, rec = M.osdw(H, c["syndrome"], c["llr"], c["hard"], c["order"], c["maxc"], c["ordering"])
        assert np.array_equal(sol, c["solution"]), (c["name"], rec)
        assert not (rec["first_valid"] or rec["better_valid"] or rec["invalid_after_valid_ignored"]), c["name"]
        swept += rec["winner"] >= 0
    assert swept == 18                       # 18 of the 44 end on a swept candidate


@pytest.mark.parametrize("name", [n for n in S.RUN if S.case(n).modelled])
def test_model_equals_oracle(oracle, name):
    sol, _ = S.model_answers(name)
    want = S.oracle_answers(oracle, name)
    assert np.array_equal(sol, want), (name, np.flatnonzero((sol != want).any(axis=1)))


@pytest.mark.parametrize("name", S.RUN)
def test_case_holds_what_it_is_named_for(oracle, name):
    c = S.case(name)
    e = c.expect
    assert S.verdict(c.m, c.n, c.order, c.maxc) is None
    assert e["tested"] == min(M.candidate_count(e["K"], c.order, c.maxc), S.MAX_CAND)                # the table's own two numbers agree
    assert S.worst_candidates(c.n, c.order, c.maxc) >= e["tested"]
    if not c.modelled:
        # above MODEL_MAX: the oracle alone.  Rank 0 (an empty row), so K = min(n, order + 10); the marked flip set is the answer, found or cut off
        assert e["tested"] > S.MODEL_MAX and not c.H.any() and e["K"] == min(c.n, c.order + 10)
        want = S.oracle_answers(oracle, name)
        for b in range(c.B):
            assert np.flatnonzero(c.hard[b]).size <= c.order and not want[b].any(), (name, b)      # hard + (exactly the marked flips) = 0, metric 0
        assert any(c.hard[b].sum() >= 5 for b in range(c.B))                                        # a deep candidate really won
        return
    sol, recs = S.model_answers(name)
    swept = [r for r in recs if r["w0"] > 0]
    if e.get("swept", c.B) is not None:                                              # (None: the trips, counted by test_three_trips_mix_their_shots)
        assert len(swept) == e.get("swept", c.B), (name, len(swept))
    assert {r["K"] for r in swept} == {e["K"]} and {r["tested"] for r in swept} == {e["tested"]}, name
    assert all(r["tested"] == 0 and r["winner"] == -1 for r in recs if r["w0"] == 0)
    if "winner" in e:
        assert [(r["winner"], r["winner_weight"]) for r in recs] == e["winner"], name
    for branch in e.get("fires", ()):
        assert sum(r[branch] for r in recs) > 0, (name, branch)
    H64 = c.H.astype(np.int64)
    for b, r in enumerate(recs):                                                    # w0 is what it says: the answer of a satisfiable shot satisfies
        assert (((H64 @ sol[b]) % 2 != c.synd[b]).sum() == 0) == (r["w0"] == 0), (name, b)


def test_the_table_covers_what_the_suite_is_for():
    """one case per K edge, per max_combinations cut-off, per reachable selection branch; both sides of the refusal lines and of the LDS lines"""
    T = {n: S.case(n) for n in S.TABLE}
    k_of = lambda n: T[n].expect["K"]          # noqa: E731
    assert k_of("k0_tall") == 0 and k_of("k1") == 1 and k_of("k_below_order") == T["k_below_order"].order - 1
    assert k_of("k_exact") == T["k_exact"].order + 10 == T["k_exact"].n - 3 and k_of("k_cut_tie") == T["k_cut_tie"].order + 10 < T["k_cut_tie"].n - 3
    t = T["k_cut_tie"]
    assert (np.abs(t.llr[:, 3 + 10]) == np.abs(t.llr[:, 3 + 11])).all() and (np.abs(t.llr[:, 3 + 9]) < np.abs(t.llr[:, 3 + 10])).all()
    assert (T["n1"].m, T["n1"].n) == (1, 1) and T["n1_k0"].n == 1 and T["m1"].m == 1
    c1, total = 13, S.T3
    assert [T[n].maxc for n in ("cut_1", "cut_c1m", "cut_c1", "cut_c1p", "cut_256", "cut_257", "cut_total", "cut_total1", "cut_none")] == \
        [1, c1 - 1, c1, c1 + 1, 256, 257, total, total + 1, 0]
    assert len({T[n].H.tobytes() for n in T if n.startswith("cut_")}) == 1 and M.candidate_count(13, 3, None) == total
    # capacity: 65535 uncut is the largest accepted, 106761 is refused and accepted once cut to the slab; order 10 accepted, 11 refused
    assert S.worst_candidates(17, 8, None) == 65535 and S.worst_candidates(18, 8, None) == 106761 and S.worst_candidates(18, 8, 65536) == 65536
    assert S.verdict(1, 17, 8, None) is None and S.verdict(1, 18, 8, None) == (S.ERR_UNSUPPORTED, S.CAND_TEXT) and S.verdict(1, 18, 8, 65536) is None
    assert S.verdict(1, 18, 8, 65537) == (S.ERR_UNSUPPORTED, S.CAND_TEXT)
    assert S.verdict(1, 20, 10, 65536) is None and S.verdict(1, 4, 11, 16) == (S.ERR_INVALID, S.ORDER_TEXT)
    assert S.worst_candidates(20, 10, None) == 616665 and T["cap_order10"].order == S.MAX_ORDER
    # the elimination scratch: 5 m + 8 nwords + 40, one row word up to n = 64
    assert [S.elim_lds_bytes(m, 1) for m in (13097, 13098, 30710, 30711)] == [65533, 65538, 153598, 153603]
    assert S.nwords_of(24) == S.nwords_of(64) == 1 and S.nwords_of(65) == 2 and S.nwords_of(129) == 3
    assert S.elim_lds_bytes(13097, 1) <= 64 * 1024 < S.elim_lds_bytes(13098, 1) and S.elim_lds_bytes(30710, 1) <= S.ELIM_MAX < S.elim_lds_bytes(30711, 1)
    assert S.verdict(30710, 24, 1, None) is None and S.verdict(30711, 24, 1, None) == (S.ERR_UNSUPPORTED, S.LDS_TEXT)
    for n in S.REFUSED:
        assert S.verdict(T[n].m, T[n].n, T[n].order, T[n].maxc) == T[n].refused, n
    assert [T[n].m for n in ("lds_13097", "lds_13098", "lds_30710", "lds_30711")] == [13097, 13098, 30710, 30711]
    assert {T[n].n for n in ("n63", "n64", "n65", "n129")} == {63, 64, 65, 129}
    # the grid: 64 workgroups, three trips at B = 133
    assert S.grid_of(1) == 1 and S.grid_of(64) == 64 and S.grid_of(65) == 64 and S.trips_of(64) == 1 and S.trips_of(65) == 2 and S.trips_of(S.TRIP_B) == 3
    assert all(T[n].B == S.TRIP_B == 133 for n in S.TRIPS)
    # selection: a winner of weight >= 2 past index 256, a kept tie, nothing better; every reachable branch fires somewhere
    assert T["sel_deep"].expect["winner"][0][0] > 256 and T["sel_deep"].expect["winner"][0][1] >= 2
    fired = {b: sum(r[b] for n in S.RUN if T[n].modelled for r in S.model_answers(n)[1]) for b in M.BRANCHES}
    assert fired["better_invalid"] > 0 and fired["tie_kept_earlier"] > 0
    assert any(r["winner"] == -1 and r["tested"] > 0 for n in S.RUN if T[n].modelled for r in S.model_answers(n)[1])


def test_inputs_are_what_they_are_named_for():
    c = S.case("in_nonfinite")
    assert np.isnan(c.llr).any() and np.isposinf(c.llr).any() and np.isneginf(c.llr).any() and ((c.llr == 0) & np.signbit(c.llr)).any()
    assert c.hard.any() and (c.H.sum(axis=1) == 0).any() and np.array_equal(c.H[7], c.H[0]) and np.array_equal(c.H[:, -1], c.H[:, 6])
    for name in ("in_nonfinite", "n63", "n64", "n65", "n129"):
        c = S.case(name)
        a = np.abs(c.llr)
        assert all(np.unique(a[b][np.isfinite(a[b])]).size < np.isfinite(a[b]).sum() for b in range(c.B)), name       # runs of equal magnitude
        assert np.array_equal(c.H[6], np.zeros(c.n, np.uint8)) and np.array_equal(c.H[7], c.H[0]) and np.array_equal(c.H[8], c.H[0] ^ c.H[1])
    for name in ("n63", "n64", "n65", "n129"):
        w = [r["winner"] for r in S.model_answers(name)[1]]
        assert max(w) >= 0 and min(w) == -1, (name, w)                                # the sweep changes some answers and leaves others


@pytest.mark.parametrize("name", S.TRIPS)
def test_three_trips_mix_their_shots(name):
    """every workgroup b takes shots b, b + 64 (and b + 128 for b < 5): satisfiable and swept shots follow each other in every order, neighbours in a workgroup differ in
    their order (so in pivots and e_permuted); on the small matrix every pair of kinds follows each other in some workgroup"""
    c = S.case(name)
    _, recs = S.model_answers(name)
    sat = np.array([r["w0"] == 0 for r in recs])
    win = np.array([r["winner"] >= 0 for r in recs])
    differ = 0
    for b in range(S.GRID):
        mine = list(range(b, c.B, S.GRID))
        assert len(mine) == (3 if b < 5 else 2)
        assert not sat[mine].all(), (name, b)
        differ += not np.array_equal(recs[mine[0]]["eperm"], recs[mine[1]]["eperm"])
    assert differ >= 56 or name == "trips_tall", differ                     # what a neighbour leaves behind is not what the next shot needs
    assert 40 <= sat.sum() <= 50
    if name == "trips_tall":
        assert all(r["K"] == 0 for r in recs) and np.linalg.matrix_rank(c.H.astype(float)) == c.n
        return
    seqs = {tuple("s" if sat[i] else "w" if win[i] else "0" for i in range(b, c.B, S.GRID)) for b in range(S.GRID)}
    pairs = {q[i:i + 2] for q in seqs for i in range(len(q) - 1)}                 # s: satisfiable, w: a swept candidate wins, 0: swept, OSD-0 kept
    assert {("w", "s"), ("s", "w"), ("s", "0"), ("0", "s"), ("w", "0"), ("0", "w"), ("w", "w"), ("0", "0")} <= pairs, pairs
    assert any(len(q) == 3 for q in seqs)
    if name == "trips_ordering":
        key = np.abs(c.llr)
        unsorted = [b for b in range(c.B) if (np.diff(key[b][c.ordering[b]]) < 0).any()]
        assert unsorted == list(range(1, c.B, 3)) and len(unsorted) >= c.B // 3
        assert all(sorted(c.ordering[b]) == list(range(c.n)) for b in range(c.B))


@pytest.mark.parametrize("mistake", OBSERVABLE)
def test_mistake_changes_an_answer(mistake):
    """a wrong copy of the model (osdw_model.MISTAKES) gives another answer on at least one case of the table: the table would catch a kernel with the
    same defect.  maxc_plus_one / maxc_minus_one are the two directions of "max_combinations off by one"."""
    right = {n: S.model_answers(n)[0] for n in WHERE[mistake]}
    changed = [n for n in WHERE[mistake] if not np.array_equal(S.model_answers(n, mistake)[0], right[n])]
    assert changed, (mistake, M.MISTAKES[mistake])
    if mistake in ("maxc_plus_one", "maxc_minus_one"):
        assert len(changed) >= 4, changed                                          # on every weight-class boundary it is placed at, not on one by luck
    if mistake == "stale_eperm":
        sol = S.model_answers("trips_small", mistake)[0]
        assert np.array_equal(sol[:S.GRID], right["trips_small"][:S.GRID])          # first trips have nothing to inherit
        assert (sol[S.GRID:] != right["trips_small"][S.GRID:]).any(axis=1).sum() >= 10


def test_wmax_above_k_is_not_observable():
    for name in ("k1", "k_below_order", "n1"):
        c = S.case(name)
        assert c.expect["K"] < c.order
        sol, recs = S.model_answers(name, "wmax_is_order")
        assert np.array_equal(sol, S.model_answers(name)[0]) and [r["tested"] for r in recs] == [r["tested"] for r in S.model_answers(name)[1]]
    assert S.case("k_below_order").expect["tested"] == 2 ** 3 - 1


def test_no_candidate_of_a_sweep_is_ever_valid():
    """the sweep is entered only when Gauss-Jordan's answer misses the syndrome, i.e. the system is inconsistent, and then nothing satisfies it"""
    for name in S.RUN:
        if S.case(name).modelled:
            for r in S.model_answers(name)[1]:
                assert not (r["first_valid"] or r["better_valid"] or r["invalid_after_valid_ignored"] or r["valid_over_smaller_invalid"]), name
    for mistake in ("le_valid", "valid_needs_metric"):
        for name in ("sel_tie", "sel_deep", "n64"):
            assert np.array_equal(S.model_answers(name, mistake)[0], S.model_answers(name)[0])


def test_selection_rule_on_made_up_lists():
    """`select` against the rule as the issue of record states it, branch by branch, on (weight, metric) lists no matrix produces"""
    sel = M.select
    # the first valid candidate replaces an invalid best whatever its metric (here: a larger one)
    best, f = sel(100, [(2, 90), (0, 95), (1, 10)])
    assert best == 1 and f["better_invalid"] == 1 and f["first_valid"] == 1 and f["valid_over_smaller_invalid"] == 1 and f["invalid_after_valid_ignored"] == 1
    assert sel(100, [(2, 90), (0, 95), (1, 10)], "valid_needs_metric")[0] == 2
    # later only a strictly smaller valid metric replaces it; equal keeps the earlier
    best, f = sel(100, [(0, 50), (0, 50), (0, 49), (0, 49), (0, 60)])
    assert best == 2 and f["first_valid"] == 1 and f["better_valid"] == 1 and f["tie_kept_earlier"] == 2
    assert sel(100, [(0, 50), (0, 50), (0, 49), (0, 49), (0, 60)], "le_valid")[0] == 3
    # invalid candidates: strictly smaller only, before the first valid one; equal keeps the earlier; nothing better keeps OSD-0
    assert sel(100, [(3, 100), (1, 99), (2, 99)])[0] == 1 and sel(100, [(3, 100), (1, 99), (2, 99)], "le_invalid")[0] == 2
    assert sel(100, [(3, 100), (3, 101)]) == (-1, dict.fromkeys(M.BRANCHES, 0) | {"tie_kept_earlier": 1})
    assert sel(100, [(3, 100), (3, 101)], "first_candidate_free")[0] == 0
    # IEEE: no comparison with NaN holds, nothing is below +inf but a finite number
    assert sel(M.NAN, [(1, 5)])[0] == -1 and sel(100, [(1, M.NAN)])[0] == -1 and sel(M.NAN, [(0, M.NAN), (0, 1)])[0] == 0
    assert sel(M.INF, [(1, M.INF), (1, 7)])[0] == 1 and sel(5, [(1, M.INF)])[0] == -1


def test_exact_metric_is_the_float_metric_on_eighths():
    """on multiples of 1/8 the model's integer metric, scaled back, is the double the kernel's sum gives, in either direction of summation"""
    rng = np.random.default_rng(5)
    for _ in range(50):
        n = int(rng.integers(1, 130))
        llr, sol, wt = S.eighths(rng, n), (rng.random(n) < 0.5).astype(np.int64), int(rng.integers(0, 30711))
        mt = M.Metric(llr)
        exact = mt(sol, wt) / mt.scale
        for order in (range(n), range(n - 1, -1, -1)):
            acc = 1e10 + wt * 1e8 if wt > 0 else 0.0
            for j in order:
                acc += float(sol[j]) * abs(llr[j])
            assert acc == exact
