"""The layered graph families of tests/window_shapes.py without a GPU: every family has the structure it claims, the numpy model
(tests/window_model.py) cuts the windows an independent restatement on the dense matrix cuts, and the inputs of tests/test_window_shapes_gpu.py
exercise what that module relies on (converged and OSD-0 windows, unsatisfied shots, every decode path, both sides of the OSD-0 size limits)."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_shapes as GS  # noqa: E402
import window_model as WM  # noqa: E402
import window_shapes as WS  # noqa: E402

FAMILIES = WS.families()
BY_NAME = {c.name: c for c in FAMILIES}
NAMES = ["lr1", "periodic_r42", "small_irregular", "mid_lr33", "wide_lr130", "heavy_rows", "gaps", "one_layer", "prior_variants"]
_REF = {}


def reference(orc, case, prior, W, C):
    """(model, syndromes, the model's five outputs) of one configuration at WS.SHOTS shots and WS.MAX_ITER; computed once"""
    key = (case.name, prior, W, C)
    if key not in _REF:
        mo = WS.model(case, prior, W, C)
        S = WS.syndromes(case, WS.SHOTS)
        _REF[key] = (mo, S, mo.decode(orc, S, max_iter=WS.MAX_ITER))
    return _REF[key]


def decoded(case):
    return [(p, W, C) for p in case.priors for W, C in case.configs if (W, C) not in case.refused]


def dense(case):
    H = np.zeros((case.m, case.n), np.int8)
    H[np.repeat(np.arange(case.m), np.diff(case.indptr)), case.indices] = 1
    return H


def test_the_families_and_their_configurations():
    assert [c.name for c in FAMILIES] == NAMES
    assert set(a for c in FAMILIES for a in c.axes) == set(WS.AXES)
    again = WS.families()
    for a, b in zip(FAMILIES, again):                                          # deterministic from the seed
        assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
        assert all(np.array_equal(a.priors[k].view(np.uint64), b.priors[k].view(np.uint64)) for k in a.priors)
        assert np.array_equal(WS.syndromes(a, 5), WS.syndromes(b, 5))
    for c in FAMILIES:
        L = c.layers
        need = [(1, 1), (2, 1), (2, 2), (3, 2), (4, 3), (L, L), (L + 3, 2), (L - 1, L - 1)]
        assert all(wc in c.configs for wc in need if wc[0] >= 1), c.name
        S = WS.syndromes(c, WS.SHOTS)
        assert S.shape == (WS.SHOTS, c.m) and not S[-1].any() and set(np.unique(S)) <= {0, 1}
    assert (8, 2) in BY_NAME["wide_lr130"].configs


@pytest.mark.parametrize("name", NAMES)
def test_claims(name):
    c = BY_NAME[name]
    lr, Lyr, claims = c.layer_rows, c.layers, dict(c.claims)
    assert c.m == lr * Lyr and c.indptr[0] == 0 and c.indptr[-1] == len(c.indices) and (c.indices >= 0).all() and (c.indices < c.n).all()
    for i in range(c.m):
        assert (np.diff(c.indices[c.indptr[i]:c.indptr[i + 1]]) > 0).all(), f"row {i} is not sorted or repeats an edge"
    H = dense(c)
    rd, cd = H.sum(axis=1), H.sum(axis=0)
    first = np.where(cd > 0, H.argmax(axis=0) // lr, 0)
    last = np.where(cd > 0, (c.m - 1 - H[::-1].argmax(axis=0)) // lr, 0)
    span = last - first
    assert set(np.unique(span)) <= {0, 1}
    tau, mspan = WM.column_layers(WM.Matrix(c.indptr, c.indices, c.n), lr)
    assert np.array_equal(tau, first) and np.array_equal(mspan, span)
    born = np.bincount(first[cd > 0], minlength=Lyr)
    assert np.array_equal(born, np.diff(c.start)) and (np.diff(first[cd > 0]) >= 0).all()      # the columns of a layer are one index range
    assert all(np.isfinite(p).all() and p.shape == (c.n,) for p in c.priors.values())
    own = lambda t: H[t * lr:(t + 1) * lr, c.start[t]:c.start[t + 1]]                          # noqa: E731
    seen = set()
    for k, v in claims.items():
        seen.add(k)
        if k == "max_row":
            assert rd.max() <= v
        elif k == "min_max_row":
            assert rd.max() >= v
        elif k == "max_col":
            assert cd.max() <= v
        elif k == "born_range":
            assert born.min() == v[0] and born.max() == v[1]
        elif k == "spans":
            assert (span[cd > 0] == 0).any() and (span == 1).any()
        elif k == "all_span":
            assert (span[:c.start[Lyr - 1]] == 1).all() and (span[c.start[Lyr - 1]:] == 0).all()
        elif k == "empty_cols":
            assert (cd == 0).sum() == v and (cd[c.n - v:] == 0).all()
        elif k == "periodic":
            for t in range(1, Lyr):
                assert np.array_equal(own(t), own(0))
                if t + 1 < Lyr:
                    assert np.array_equal(H[(t + 1) * lr:(t + 2) * lr, c.start[t]:c.start[t + 1]], H[lr:2 * lr, :c.start[1]])
        elif k == "own_regular":
            for t in range(Lyr):
                assert (own(t).sum(axis=1) == v[0]).all() and (own(t).sum(axis=0) == v[1]).all()
            assert not GS.regular_takes(rd, cd)                                               # the whole matrix is not regular
        elif k == "heavy":
            for row, D in v.items():
                assert rd[row] == D and (first[np.flatnonzero(H[row])] == row // lr).all()
            assert sorted(rd)[-len(v):] == sorted(v.values())
        elif k == "empty_rows":
            assert (rd == 0).sum() == v and (rd[4::5] == 0).all()
        elif k == "twin_rows":
            assert rd[v[0]] > 0 and np.array_equal(H[v[0]], H[v[1]]) and v[0] // lr == v[1] // lr
        elif k == "unborn_layers":
            assert tuple(np.flatnonzero(born == 0)) == v and Lyr - 1 in v
        elif k == "one_layer":
            assert Lyr == 1
        else:
            raise AssertionError(f"unknown claim {k}")
    assert seen == set(claims)
    if name != "small_irregular":
        assert (cd > 0).all()
    # refusals: exactly the configurations in which the model has a window without columns, named by the first such window's layer
    for W, C in c.configs:
        zero = [s["a"] for s in WS.model(c, next(iter(c.priors)), W, C).stages if s["cols"].size == 0]
        assert (zero[0] if zero else None) == c.refused.get((W, C)), (W, C, zero)
    if name == "gaps":
        assert set(c.refused) == {(1, 1), (Lyr - 1, Lyr - 1)} and c.refused[(Lyr - 1, Lyr - 1)] == Lyr - 1
    if name == "small_irregular":
        assert ((cd == 0) & (c.priors["negative class"] < 0)).sum() >= 2 and ((cd == 0) & (c.priors["negative class"] > 0)).any()
    if name == "prior_variants":
        u = c.priors["uniform"]
        for k, p in c.priors.items():
            diff = np.flatnonzero(p.view(np.uint64) != u.view(np.uint64))
            if k in ("one ulp", "one -0.0"):
                assert diff.size == 1 and first[diff[0]] == 3                                  # one interior column
        assert c.priors["one ulp"].max() == np.nextafter(4.0, 5.0) and np.signbit(c.priors["one -0.0"]).sum() == 1
        assert len(set(c.priors["all distinct"])) == c.n and (c.priors["above clip"] > 20.0).any()


@pytest.mark.parametrize("name", NAMES)
def test_model_against_plain_slicing(oracle, name):
    c = BY_NAME[name]
    lr, Lyr = c.layer_rows, c.layers
    H = dense(c)
    cd = H.sum(axis=0)
    tau = np.where(cd > 0, H.argmax(axis=0) // lr, 0)
    M = WM.Matrix(c.indptr, c.indices, c.n)
    for prior, W, C in decoded(c):
        mo, S, (err, conv, iters, osd, unsat) = reference(oracle, c, prior, W, C)
        k, done = 0, np.zeros(c.n, int)
        while True:                                                          # rule 3 of the header, restated
            a = k * C
            end, is_last = min(a + W, Lyr), a + W >= Lyr
            st = mo.stages[k]
            cols = np.flatnonzero((tau >= a) & (tau < end))
            assert (st["a"], st["end"], st["last"]) == (a, end, is_last) and np.array_equal(st["cols"], cols)
            block = np.zeros((st["r1"] - st["r0"], cols.size), np.int8)
            block[np.repeat(np.arange(len(st["indptr"]) - 1), np.diff(st["indptr"])), st["indices"]] = 1
            assert np.array_equal(block, H[a * lr:end * lr][:, cols]), (prior, W, C, k)
            assert np.array_equal(st["prior"].view(np.uint64), c.priors[prior][cols].view(np.uint64))
            done[cols[(tau[cols] < a + C) | is_last]] += 1
            assert np.array_equal(st["cols"][st["committed"]], cols[(tau[cols] < a + C) | is_last])
            k += 1
            if is_last:
                break
        assert k == len(mo.stages) and (done == 1).all(), (prior, W, C)       # every column is committed exactly once
        assert np.array_equal(mo.r_final, (S & 1) ^ M.parity(err)) and np.array_equal(unsat, mo.r_final.any(axis=1).astype(np.uint8))
        assert np.array_equal(conv + osd, np.full(len(S), k, np.int32)) and (iters >= k).all()


def test_inputs_exercise_what_the_gpu_module_relies_on(oracle):
    paths, sizes = set(), set()
    for c in FAMILIES:
        nconv = nosd = 0
        for prior, W, C in decoded(c):
            mo, S, (err, conv, iters, osd, unsat) = reference(oracle, c, prior, W, C)
            nconv, nosd = nconv + int(conv.sum()), nosd + int(osd.sum())
            paths |= WS.expected_paths(c, prior, W, C)
            sizes |= {(s["r1"] - s["r0"], s["cols"].size) for s in mo.stages}
            if c.name == "gaps":
                assert unsat.any() and not unsat.all(), (prior, W, C)
                assert unsat[0] == 1 and unsat[-1] == 0
            if W >= c.layers:                                                # rule 7: one window, the whole-graph decode
                det, cv, llr, it = oracle.minsum_decode_batch(c.indptr, c.indices, c.n, S, c.priors[prior], max_iter=WS.MAX_ITER)
                for b in np.flatnonzero(cv == 0):
                    det[b] = oracle.osd0(c.indptr, c.indices, c.n, S[b], llr[b], det[b])
                assert len(mo.stages) == 1 and np.array_equal(err, det) and np.array_equal(conv, cv.astype(np.int32)) and np.array_equal(iters, it + 1)
        assert nconv > 0 and nosd > 0, c.name
    c = BY_NAME["small_irregular"]
    empty = np.flatnonzero(np.bincount(c.indices, minlength=c.n) == 0)
    for W, C in c.configs:
        err = reference(oracle, c, "negative class", W, C)[2][0]
        neg = empty[c.priors["negative class"][empty] < 0]
        assert (err[:, neg] == 1).all() and not err[:, np.setdiff1d(empty, neg)].any()      # empty columns keep the sign of their prior
    assert paths == {"REGULAR", "RESIDENT", "WG2", "WG", "STREAM"}
    assert WS.expected_paths(BY_NAME["periodic_r42"], "uniform", 1, 1) == {"REGULAR"}
    assert {"WG", "STREAM"} <= WS.expected_paths(BY_NAME["heavy_rows"], "uniform", 2, 1)
    assert "WG2" not in set().union(*[WS.expected_paths(BY_NAME["prior_variants"], "all distinct", W, C) for W, C in BY_NAME["prior_variants"].configs])
    small = lambda s: s[0] <= 128 and s[1] <= 1024                            # noqa: E731  (the one-wave OSD-0 kernel)
    assert any(small(s) for s in sizes) and any(s[0] > 128 and s[1] <= 1024 for s in sizes) and any(s[1] > 1024 for s in sizes)
    assert (99, 450) in sizes and (132, 600) in sizes                         # mid_lr33: W = 3 is the last one-wave window, W = 4 the first beyond
    assert any(not small(s) and s[0] <= 1024 for s in sizes) and any(s[0] > 1024 for s in sizes)
    assert (1040, 5600) in sizes and (1, 2) in sizes


def test_sharing_follows_the_prior_slice():
    c = BY_NAME["prior_variants"]
    for W, C in c.configs:
        g = {p: WS.model(c, p, W, C).distinct_graphs() for p in c.priors}
        nwin = len(WS.model(c, "uniform", W, C).stages)
        assert g["all distinct"] == nwin and g["uniform"] <= g["one ulp"] <= g["uniform"] + W and g["one -0.0"] == g["one ulp"], (W, C, g)
        if nwin > 1:
            assert g["one ulp"] > g["uniform"] or g["uniform"] == nwin, (W, C, g)
    assert WS.model(c, "uniform", 2, 1).distinct_graphs() == 1 and WS.model(c, "one ulp", 2, 1).distinct_graphs() == 3
    # an aperiodic graph: no two windows coincide
    for name in ("small_irregular", "mid_lr33", "heavy_rows"):
        a = BY_NAME[name]
        for W, C in a.configs:
            mo = WS.model(a, "uniform", W, C)
            assert mo.distinct_graphs() == len(mo.stages), (name, W, C)


def test_big_batch(oracle):
    c, prior, (W, C), S, max_iter = WS.big_batch(FAMILIES)
    assert len(S) == 8200 and max_iter == 2
    mo = WS.model(c, prior, W, C)
    t0 = time.perf_counter()
    trace = []
    out = mo.decode(oracle, S, max_iter=max_iter, trace=trace)
    took = time.perf_counter() - t0
    unconverged = [int((cv == 0).sum()) for _, _, _, cv in trace]
    print(f"big batch: {c.name} {prior} ({W}, {C}): {took:.2f} s, unconverged per window {unconverged}")
    assert max(unconverged) > 2048 and min(unconverged) < 8200               # the OSD-0 tickets of the one-wave kernel come into play
    assert out[1].any() and out[3].any()
