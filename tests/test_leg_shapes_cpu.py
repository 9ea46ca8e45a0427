"""CPU side of tests/leg_shapes.py: every new family has the structure it claims, its place relative to its limit follows from the restated byte
counts (both sides of the four LDS lines and of both bounds of the block rule), the numpy model of guided decimation equals the scalar loop over the
header's steps on the small and the degenerate families (NaN and +inf keys, running out of columns), and the model's runs over all cases contain the
edges tests/test_leg_shapes_gpu.py is about."""
import numpy as np
import pytest

import graph_shapes as GS
import leg_shapes as LS
from test_decimation_cpu import scalar_decode

CASES = LS.all_cases()
BY_NAME = {c.name: c for c in CASES}
NEW = [c.name for c in CASES if c.new]
SCALAR = sorted({c.name for c in CASES if c.n <= 129 and LS.modes(c)[0]} | {"deg1_shared", "deg1_distinct", "decim_vg_last"})


def test_cases_are_deterministic_valid_csr_and_complete():
    again = LS.cases()
    assert [c.name for c in again] == [c.name for c in CASES]
    for a, b in zip(CASES, again):
        assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and a.n == b.n, a.name
        assert list(a.priors) == list(b.priors) and all(np.array_equal(a.priors[k], b.priors[k]) for k in a.priors), a.name
        assert a.indptr.dtype == np.int32 and a.indices.dtype == np.int32 and a.indptr[0] == 0 and a.indptr[-1] == len(a.indices), a.name
        assert (np.diff(a.indptr) >= 0).all() and (a.indices >= 0).all() and (a.indices < a.n).all(), a.name
        for i in range(a.m):                                                # CSR rows sorted, no repeated edge
            assert (np.diff(a.indices[a.indptr[i]:a.indptr[i + 1]]) > 0).all(), (a.name, i)
        assert a.priors and all(p.shape == (a.n,) and p.dtype == np.float64 and np.isfinite(p).all() for p in a.priors.values()), a.name
    # every family of graph_shapes the two decoders accept, with every finite prior (alldeg_wide: the three the classes are about and the -0.0)
    old = {c.name: c for c in GS.families()}
    assert {c.name for c in CASES if not c.new} == {k for k, c in old.items() if c.row_deg.max() <= 56}
    assert {"regular63", "reg63_m512", "reg63_m513", "small_irregular", "rowdeg56", "hub_col", "hub_row", "m1025"} <= set(BY_NAME)
    assert not {"rowdeg57", "rowdeg255", "rowdeg256"} & set(BY_NAME)
    for c in CASES:
        if not c.new and c.name != "alldeg_wide":
            assert list(c.priors) == list(old[c.name].priors), c.name
    w = BY_NAME["alldeg_wide"].priors
    assert (w["negative class"] < 0).any() and (w["zero class"] == 0).any() and (w["above clip"] > 20).any() and np.signbit(w["one -0.0"]).sum() == 1
    assert set(NEW) == {"decim_lds_last", "decim_lds_first", "relay_lds_last", "relay_lds_first", "decim_vg_last", "decim_refused", "relay_vg_last",
                        "relay_refused", "n1", "n31", "n32", "n33", "ties_512", "ties_1024"}
    # what the issue of these tests lists for the shared launch is among the cases: m above the block, column degree above 8, row degree 56
    assert any(c.m > 1024 and LS.modes(c)[0] for c in CASES) and any(c.col_deg.max() > 8 for c in CASES) and any(c.row_deg.max() == 56 for c in CASES)


@pytest.mark.parametrize("name", NEW)
def test_new_family_has_the_structure_it_claims(name):
    c = BY_NAME[name]
    k, rd, cd = c.claims, c.row_deg, c.col_deg
    assert (c.m, c.n) == (k["m"], k["n"])
    if "max_row" in k:
        assert rd.max() == k["max_row"]
    if "col_degs" in k:
        assert set(np.unique(cd).tolist()) == k["col_degs"]
    if "deg0" in k:                                                         # about 3000 columns have edges, the rest has none (as vglobal_*)
        assert (cd == 0).sum() == k["deg0"] and set(np.unique(cd).tolist()) == {0, 2, 4} and (rd > 0).all()
    if "full_rows" in k:                                                    # about 200 rows of degree 5 scattered over the index range, every other row empty
        assert (rd == k["full_deg"]).sum() == k["full_rows"] and (rd == 0).sum() == c.m - k["full_rows"]
        full = np.flatnonzero(rd)
        assert full.min() < c.m // 8 and full.max() > c.m - c.m // 8 and (full > 1024).sum() > 100 and cd.min() >= 9
    if name in ("n31", "n32", "n33"):
        assert (c.n + 31) // 32 == (1, 1, 2)[c.n - 31] and c.n < 64 and rd.min() > 1
    if name == "n1":
        assert rd.tolist() == [1]
    if k.get("ties"):
        tied = np.flatnonzero(cd == 0)
        prior = c.priors["tie class"]
        assert 2 * tied.size > c.n and (prior[tied] == LS.TIE_PRIOR).all() and rd.min() > 1 and rd.max() <= 56
        # the degree-0 class has the largest prior, beyond what a column with edges can reach in a round that starts from the priors ...
        others = np.abs(prior[cd > 0])
        assert LS.TIE_PRIOR > others.max() + cd.max() * max(p["alpha"] * max(p["clip_llr"], others.max()) for p in LS.DECIM_SETS.values())
        # ... scattered over the index range: the 64 lowest have 64 owner threads, the same number in every wave of the block, and every one of
        # those owners holds a further tied column (it rescans to a tie)
        low = tied[:64]
        nt = k["block"]
        assert nt == LS.block_threads(c.m, c.n) and low.max() < nt and tied[64] == nt and np.array_equal(tied[64:], np.arange(nt, c.n))
        assert np.array_equal(low // (nt // 64), np.arange(64)) and len(set(np.diff(low).tolist())) > 2
        assert np.bincount(low // 64, minlength=nt // 64).tolist() == [64 * 64 // nt] * (nt // 64)
        assert np.isin(low + nt, tied).all()


def test_pairs_differ_only_where_they_say():
    for a, b in (("decim_lds_last", "decim_lds_first"), ("relay_lds_last", "relay_lds_first")):
        a, b = BY_NAME[a], BY_NAME[b]
        assert b.n == a.n + 1 and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
    for a, b in (("decim_vg_last", "decim_refused"), ("relay_vg_last", "relay_refused")):
        a, b = BY_NAME[a], BY_NAME[b]
        assert b.m == a.m + 1 and np.array_equal(a.indptr, b.indptr[:-1]) and b.indptr[-1] == b.indptr[-2] and np.array_equal(a.indices, b.indices)


def test_every_limit_is_hit_on_both_sides():
    """The place of a family follows from the restated counts alone: its claimed (BPGD, Relay-BP) modes, that it is the last size that fits or the
    first that does not, and over all cases every mode of both decoders and both sides of both bounds of the block rule."""
    seen = set()
    for name in NEW:
        c = BY_NAME[name]
        line = c.claims.get("line")
        if not line:
            continue
        assert LS.modes(c) == c.claims["modes"], name
        count = LS.decim_lds_bytes if line["count"] == "decim" else LS.relay_lds_bytes
        step = 1 if line["fits"] else -1
        if line["limit"] == "lds":                                          # m = 300, n moves: everything in LDS
            here, there = count(c.m, c.n, False), count(c.m, c.n + step, False)
        else:                                                               # n = 64, m moves: posteriors in global memory
            here, there = count(c.m, c.n, True), count(c.m + step, c.n, True)
        assert (here <= LS.LDS_BYTES) == line["fits"] and (there <= LS.LDS_BYTES) != line["fits"], (name, here, there)
        seen.add((line["count"], line["limit"], line["fits"]))
    assert len(seen) == 8
    # the figures of the two counts at m = 300 and at n = 64 (computed from csrc/ by hand; a literal only here, the families search the rule)
    assert (BY_NAME["decim_lds_last"].n, BY_NAME["relay_lds_last"].n, BY_NAME["decim_vg_last"].m, BY_NAME["relay_vg_last"].m) == (18938, 15660, 6808, 6820)
    # between the two accept lines BPGD refuses what Relay-BP takes, and between the two LDS lines it keeps in LDS what Relay-BP does not
    assert all(LS.decim_mode(m, 64, 5) == 0 and LS.relay_mode(m, 64, 5) == 2 for m in range(6809, 6821))
    assert LS.modes(BY_NAME["relay_lds_first"]) == (1, 2) and LS.modes(BY_NAME["decim_refused"]) == (0, 2)
    have = [LS.modes(c) for c in CASES]
    assert {d for d, _ in have} == {0, 1, 2} and {r for _, r in have} == {0, 1, 2}
    assert LS.decim_mode(64, 700, 57) == 0 and LS.relay_mode(64, 700, 57) == 0 and LS.relay_mode(64, 700, 56) == 1
    blocks = {(c.m, c.n): LS.block_threads(c.m, c.n) for c in CASES}
    assert blocks[(512, 4096)] == 512 and blocks[(513, 4096)] == 1024 and blocks[(512, 4097)] == 1024
    assert sorted(set(blocks.values())) == [512, 1024]
    assert LS.block_threads(32, 1100) == 512 and LS.block_threads(32, 4200) == 1024 and LS.block_threads(6808, 64) == 1024


@pytest.mark.parametrize("name", SCALAR)
def test_model_equals_the_scalar_loop(name):
    """decimation_model.decim_decode against scalar_decode of tests/test_decimation_cpu.py, the header's steps on Python floats: the NaN and +inf
    key rule (deg1_shared, deg1_distinct, n1) and running out of columns (n <= 129 with per_round = 64) are checked against the steps, not only
    against the model itself."""
    c = BY_NAME[name]
    S = LS.syndromes(c)
    for pn, prior in c.priors.items():
        for sn, p in LS.DECIM_SETS.items():
            got, _ = LS.decim_reference(c, pn, sn)
            for b in range(LS.B):
                ref = scalar_decode(c.indptr, c.indices, c.n, S[b], prior, p["alpha"], p["clip_llr"], p["t_round"], p["max_rounds"], p["per_round"],
                                    p["fix_llr"])
                ctx = (name, pn, sn, b)
                assert np.array_equal(got[0][b], np.array(ref[0], np.int8)), ctx + ("err",)
                assert np.array_equal(got[1][b], np.array(ref[1]), equal_nan=True), ctx + ("llr",)
                assert (int(got[2][b]), int(got[3][b]), int(got[4][b]), int(got[5][b])) == ref[2:], ctx + ("conv / iters / rounds / fixed",)


def _key(v):
    a = np.abs(v)
    return np.where(np.isnan(a), 0.0, a)


def test_the_model_runs_contain_every_edge():
    """Conditions on the inputs (family, prior, parameter set, B = 4 syndromes of graph_shapes.syndromes), counted in cases: each must occur."""
    seen = dict.fromkeys(("nan selected", "two +inf tied in one selection", "tie across the cut", "tie across the cut and across waves", "fixed == n",
                          "fewer than per_round selected", "a wave without a candidate", "frozen decision flipped", "converged shot", "unconverged shot",
                          "rounds > 1", "cases"), 0)
    for c in CASES:
        if LS.modes(c)[0] == 0:
            continue
        for pn in c.priors:
            for sn, p in LS.DECIM_SETS.items():
                (err, llr, conv, iters, rounds, fixed), trace = LS.decim_reference(c, pn, sn)
                hit = dict.fromkeys(seen, False)
                hit["cases"] = True
                nt = LS.block_threads(c.m, c.n)
                done = np.zeros((LS.B, c.n), bool)
                sign = np.zeros((LS.B, c.n), bool)
                for b, r, cols, before in trace:
                    a = _key(before)
                    free = np.flatnonzero(~done[b])
                    # the stated order, whatever else is counted
                    assert cols.size == min(p["per_round"], free.size) and not done[b, cols].any()
                    assert all((a[cols[i]], -cols[i]) > (a[cols[i + 1]], -cols[i + 1]) for i in range(cols.size - 1)), (c.name, pn, sn, b, r)
                    rest = np.setdiff1d(free, cols)
                    assert rest.size == 0 or a[rest].max() <= a[cols].min()
                    hit["nan selected"] |= bool(np.isnan(before[cols]).any())
                    hit["two +inf tied in one selection"] |= int(np.isinf(before[cols]).sum()) >= 2
                    hit["fewer than per_round selected"] |= cols.size < p["per_round"]
                    hit["a wave without a candidate"] |= np.unique(free % nt // 64).size < nt // 64
                    out_tied = rest[a[rest] == a[cols].min()] if rest.size else rest
                    if out_tied.size:
                        hit["tie across the cut"] = True
                        in_tied = cols[a[cols] == a[cols].min()]
                        assert out_tied.min() > in_tied.max()                 # the lower columns were taken
                        hit["tie across the cut and across waves"] |= len({int(j % nt) // 64 for j in np.concatenate([in_tied, out_tied])}) > 1
                    if c.claims.get("ties") and (r == 0 or sn == "3x4x64"):
                        # the first selection is the lowest tied columns; with per_round = 64 and t_round = 3 every selection takes the next 64
                        # (the last iterations of a round clip, so no column with edges passes |prior| + 3 * alpha * clip_llr < TIE_PRIOR)
                        tied = np.flatnonzero(c.col_deg == 0)
                        k = p["per_round"]
                        assert np.array_equal(cols, tied[k * r:k * r + k]), (c.name, sn, b, r)
                        if k == 64 and r == 0:                                # exactly the 64 lowest tied columns: owners in every wave
                            assert cols.size == 64 and {int(j) // 64 for j in cols} == set(range(nt // 64))
                    sign[b, cols] = before[cols] < 0.0
                    done[b, cols] = True
                assert np.array_equal(done.sum(axis=1), fixed)
                hit["fixed == n"] = bool((fixed == c.n).any())
                hit["frozen decision flipped"] = bool((done & (sign != (err == 1))).any())
                hit["converged shot"], hit["unconverged shot"], hit["rounds > 1"] = bool(conv.any()), bool((conv == 0).any()), bool((rounds > 1).any())
                for k, v in hit.items():
                    seen[k] += bool(v)
    for k, v in seen.items():
        print(f"{k}: {v} case(s)")
    assert all(v >= 1 for v in seen.values()), seen
    assert seen["cases"] >= 3 * len([c for c in CASES if LS.modes(c)[0]])
