"""CPU side of the graph-shape sweep (tests/graph_shapes.py): every family has the structure it claims, the decoder form it claims follows from the
selection rules, the generator is deterministic and valid for qldpc_graph_create, the CPU checker's outputs meet the non-vacuity conditions the GPU
module relies on, and the checker reproduces what the reference computed on six of the families (tests/golden/wg_shapes.npz)."""
import os

import numpy as np
import pytest

import graph_shapes as GS
from conftest import GOLDEN

FAMILIES = GS.families()
BY_NAME = {c.name: c for c in FAMILIES}


def test_generator_is_deterministic_and_valid_csr():
    again = GS.families()
    assert [c.name for c in again] == [c.name for c in FAMILIES] and len(FAMILIES) >= 45
    for a, b in zip(FAMILIES, again):
        assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and a.n == b.n, a.name
        assert list(a.priors) == list(b.priors) and all(np.array_equal(a.priors[k], b.priors[k]) for k in a.priors), a.name
        assert np.array_equal(GS.syndromes(a, 5), GS.syndromes(b, 5)), a.name
        # qldpc_graph_create's rules: indptr[0] = 0, monotone, columns in range and strictly increasing per row
        assert a.indptr.dtype == np.int32 and a.indices.dtype == np.int32 and a.indptr[0] == 0 and a.indptr[-1] == len(a.indices)
        assert (np.diff(a.indptr) >= 0).all() and (a.indices >= 0).all() and (a.indices < a.n).all(), a.name
        inner = np.ones(len(a.indices), bool)
        inner[a.indptr[1:-1][a.indptr[1:-1] < len(a.indices)]] = False
        inner[0:1] = False
        assert (np.diff(a.indices)[inner[1:]] > 0).all(), a.name
        for pr in a.priors.values():
            assert pr.shape == (a.n,) and pr.dtype == np.float64, a.name


@pytest.mark.parametrize("name", sorted(BY_NAME))
def test_family_has_the_structure_and_the_path_it_claims(name):
    c = BY_NAME[name]
    rd, cd = GS.degrees(c.indptr, c.indices, c.n)
    k = c.claims
    assert k, "a family states what it is about"
    checks = {"max_row": lambda v: rd.max() == v, "max_col": lambda v: cd.max() == v, "m": lambda v: c.m == v, "n": lambda v: c.n == v,
              "nch": lambda v: (c.n + 63) // 64 == v, "col_degs": lambda v: set(np.unique(cd).tolist()) == v, "min_deg0": lambda v: (cd == 0).sum() >= v,
              "nnz_odd": lambda v: (c.nnz % 2 == 1) == v, "max_row_le": lambda v: rd.max() <= v, "max_col_le": lambda v: cd.max() <= v,
              "empty_rows": lambda v: (rd == 0).sum() == v and rd[-1] == 0 and (rd[17:119:17] == 0).all(),
              "twin_rows": lambda v: np.array_equal(c.indices[c.indptr[v[0]]:c.indptr[v[0] + 1]], c.indices[c.indptr[v[1]]:c.indptr[v[1] + 1]]) and rd[v[0]] > 1,
              "other_rows": lambda v: (np.sort(rd)[:-1] == v).all(), "regular": lambda v: (rd == v[0]).all() and (cd == v[1]).all(),
              "regular_team": lambda v: (max(c.m, (c.n + 1) // 2) <= GS.REGULAR_TEAM) == v and max(c.m, (c.n + 1) // 2) == GS.REGULAR_TEAM + (0 if v else 1),
              "wg2_lds_fits": lambda v: (GS.wg2_lds_bytes(c.n, c.nnz) <= GS.LDS_BYTES) == v and (GS.wg2_lds_bytes(c.n + (1 if v else -1), c.nnz) <= GS.LDS_BYTES) != v,
              "wg_all_lds": lambda v: (GS.wg_lds_bytes(c.m, c.n, False) <= GS.LDS_BYTES) == v and (GS.wg_lds_bytes(c.m, c.n + (1 if v else -1), False) <= GS.LDS_BYTES) != v}
    for key, want in k.items():
        if key in checks:
            assert checks[key](want), (name, key, want, int(rd.max()), int(cd.max()), c.nnz)
    ones = np.flatnonzero(rd == 1)
    if "deg1_rows" in k:
        cols = c.indices[c.indptr[ones]]
        assert len(ones) == k["deg1_rows"] and (len(set(cols.tolist())) < len(cols)) == k["deg1_shared"]
        if k["deg1_shared"]:                                            # ... with opposite syndrome bits pinned on the two that share a column
            i, j = [int(r) for r in ones if (cols == c.indices[c.indptr[r]]).sum() == 2]
            assert c.pinned_syndrome[i] != c.pinned_syndrome[j]
    elif c.expected_path in ("WG2", "WG") and name != "hub_row":
        assert len(ones) == 0, name
    for pn, pr in c.priors.items():
        _, pure, run = GS.wg2_chunks(cd, pr)
        if "mixed" in k:                                                # the mixed-chunk count under the (degree, prior bits, index) sort
            assert int((~pure).sum()) == k["mixed"][pn] and len(pure) == 17
        if k.get("runs_all_one") == pn:
            assert pure.all() and (run == 1).all()
        if k.get("longest_run") and pn == "uniform":
            assert run.max() == k["longest_run"] and run.max() > 200
        # the claimed decoder form follows from the selection rules; the small families stay out of the resident kernel by their own structure
        assert GS.rule_path(c.indptr, c.indices, c.n, pr, damping=c.damping) == c.expected[pn], (name, pn)
        if c.expected[pn] == "WG2":
            assert GS.rule_path(c.indptr, c.indices, c.n, pr, host_prior=False) == "WG" and GS.rule_path(c.indptr, c.indices, c.n, pr, table_flags=True) == "WG"
    if c.expected_path in ("WG2", "WG") and c.m <= 64:
        assert rd.max() > 8 or cd.max() > 4, name


def test_regular_kernel_limits_follow_from_the_rules():
    """plan_regular / regular_supported of csrc/minsum_regular.hip: a team of at most 512 threads, at most 1024 iterations, clip >= 0.  The pair
    reg63_m512 / reg63_m513 differs by one check and is regular on both sides; beyond either limit the resident kernel takes the graph."""
    a, b, small = BY_NAME["reg63_m512"], BY_NAME["reg63_m513"], BY_NAME["regular63"]
    assert (a.m, a.n, b.m, b.n) == (512, 1024, 513, 1026)
    for c in (a, b, small):
        rd, cd = GS.degrees(c.indptr, c.indices, c.n)
        assert GS.regular_takes(rd, cd) and (rd.max(), cd.max()) == (6, 3), c.name
    assert a.expected_path == "REGULAR" and b.expected_path == "RESIDENT"
    for c in (a, small):
        pr = c.priors["uniform"]
        assert GS.rule_path(c.indptr, c.indices, c.n, pr, max_iter=1024) == "REGULAR" and GS.rule_path(c.indptr, c.indices, c.n, pr, max_iter=1025) == "RESIDENT"
        assert GS.rule_path(c.indptr, c.indices, c.n, pr, clip=0.0) == "REGULAR" and GS.rule_path(c.indptr, c.indices, c.n, pr, clip=-1.0) == "RESIDENT"
        assert GS.rule_path(c.indptr, c.indices, c.n, pr, damping=0.8) == "REGULAR" and GS.rule_path(c.indptr, c.indices, c.n, pr, host_prior=False) == "REGULAR"
    assert GS.rule_path(b.indptr, b.indices, b.n, b.priors["uniform"], max_iter=1) == "RESIDENT"


def test_pairs_differ_only_where_they_say():
    a, b = BY_NAME["lds_wg2"], BY_NAME["lds_wg"]
    assert b.n == a.n + 1 and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
    a, b = BY_NAME["mixed_rule"].priors["admissible"], BY_NAME["mixed_rule"].priors["one more"]
    assert len(np.unique(a)) + 1 == len(np.unique(b))
    w = BY_NAME["alldeg_wide"]
    assert len(np.unique(w.priors["two values"])) == 2 and len(np.unique(w.priors["12 values"])) == 12
    assert (w.priors["negative class"] < 0).any() and (w.priors["zero class"] == 0).any() and (w.priors["above clip"] > 20).any()
    assert np.signbit(w.priors["one -0.0"]).sum() == 1 and len(np.unique(w.priors["all distinct"])) == w.n
    assert sum(c.golden for c in FAMILIES) == 6 and all(c.m <= 64 and c.n <= 700 for c in FAMILIES if c.golden)


@pytest.mark.parametrize("name", sorted(BY_NAME))
def test_checker_outputs_are_not_vacuous(oracle, name):
    """What the GPU module compares against has something in it: per family (over its priors, B = 37, max_iter = 30) a converged shot, an unconverged
    one and one that stopped at iteration 3 or later; NaN posteriors where two degree-1 checks disagree on a column."""
    c = BY_NAME[name]
    conv, unconv, late, nan = 0, 0, 0, False
    S = GS.syndromes(c, 37)
    assert S[-1].sum() == 0 and len(np.unique(S, axis=0)) >= min(4, 2 ** c.m)
    for pr in c.priors.values():
        e, cv, llr, it = oracle.minsum_decode_batch(c.indptr, c.indices, c.n, S, pr, max_iter=30, damping=c.damping)
        cv = np.asarray(cv).astype(bool)
        conv += int(cv.sum()); unconv += int((~cv).sum()); late += int((np.asarray(it) >= 3).sum())
        nan = nan or bool(np.isnan(llr).any())
    assert conv >= 1 and unconv >= 1 and late >= 1, (name, conv, unconv, late)
    assert nan == bool(c.claims.get("nan")), name


def test_checker_reproduces_the_reference_on_six_families(oracle):
    """tests/golden/wg_shapes.npz (tests/golden/make_golden.py --only wgshapes): the reference's own decoder on rows of degree 40 and 57, column degrees
    0 .. 8, two degree-1 checks on one column, odd nnz and nch = 11.  The generator is the single source of the graphs: the fixture stores what it
    returned, and they still agree."""
    with np.load(os.path.join(GOLDEN, "wg_shapes.npz")) as d:
        G = {k: d[k] for k in d.files}
    names = [str(x) for x in G["families"]]
    assert sorted(names) == sorted(c.name for c in FAMILIES if c.golden)
    for name in names:
        c = BY_NAME[name]
        g = lambda k: G[f"{name}__{k}"]          # noqa: E731
        pn = str(g("prior_name"))
        assert np.array_equal(g("indptr"), c.indptr) and np.array_equal(g("indices"), c.indices) and int(g("n")) == c.n, name
        assert np.array_equal(g("prior"), c.priors[pn]) and np.array_equal(g("syndromes"), GS.syndromes(c, 8)), name
        out = oracle.minsum_decode_batch(c.indptr, c.indices, c.n, g("syndromes"), g("prior"), max_iter=int(g("max_iter")))
        for x, y, what in zip(out, (g("err"), g("conv"), g("llr"), g("iter")), ("err", "conv", "llr", "iter")):
            assert np.array_equal(np.asarray(x).astype(y.dtype), y, equal_nan=(what == "llr")), (name, what)
        assert name != "deg1_shared" or np.isnan(g("llr")).any()
