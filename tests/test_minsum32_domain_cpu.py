"""CPU suite of the f32 decoder's domain (tests/minsum32_shapes.py): the restated host rules on the bundled matrices, every family where it claims to
sit, the pair on every line on opposite sides of it, the numpy model (tests/minsum32_model.py) against the scalar f32 loop of
tests/test_minsum32_cpu.py on every new family (none is skipped), that nothing overflows where the clean form's bound says nothing does, and the
last-pass pair."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import minsum32_model as MM  # noqa: E402
import minsum32_shapes as MS  # noqa: E402
from test_minsum32_cpu import same, scalar_decode, sector  # noqa: E402

CASES = MS.all_cases()
BY_NAME = {c.name: c for c in CASES}
ACCEPTED = [c.name for c in CASES if c.claims["accepted"]]
LINES = [("LDS, columns", "cols_last", "cols_refused"), ("LDS, rows", "rows_last", "rows_refused"), ("one workgroup per CU", "two_wg_last", "one_wg_first"),
         ("alpha32 <= 1024", "alpha_1024", "alpha_above"), ("clip32 <= 2^100", "clip_2p100", "clip_2p101"), ("|prior32| <= 2^100", "prior_2p100", "prior_above"),
         ("|prior32| <= 2^100 after rounding", "prior_rounds_to_2p100", "prior_above")]


# families in which the model finds no shot that converges later than iteration 0, at an error weight of 1 .. 9 on top of the prior's hard decision
NO_LATE_CONVERGENCE = {"alpha_1024": "at alpha 1024 every message dwarfs the prior: a shot converges at once or oscillates", "alpha_above": "as alpha_1024",
                       "no_edges": "no message at all"}


@pytest.mark.parametrize("tag,s,lds,block,is_clean", [("circ72", "Z", None, None, True), ("circ72", "X", None, None, False), ("circ144", "Z", None, None, True),
                                                      ("circ288", "Z", 153824, 1024, True)])
def test_restated_rules_on_the_bundled_matrices(tag, s, lds, block, is_clean):
    """what tests/test_minsum32_gpu.py and the header pin: circ72 Z clean and X not (degree-1 rows), two workgroups for circ144, 153 824 bytes and one
    workgroup of 1024 threads for circ288 Z"""
    ip, ix, n, prior = sector(tag, s)
    m = len(ip) - 1
    got = MS.lds_bytes(m, n)
    assert MS.accepted(m, n, int(np.diff(ip).max())) and got <= MS.LDS_BYTES and (lds is None or got == lds)
    assert MS.clean(prior, MM.alpha_table32(50, "dynamical", 1.0).astype(np.float64), 20.0, np.diff(ip)) == is_clean
    assert not MS.clean(prior, [1.0], 20.0, np.diff(ip), flags=(MS.GENERIC,))
    if block:
        assert MS.first_block(m, n, got) == block
    else:
        assert MS.LDS_BYTES // got >= 2 and MS.first_block(m, n, got) == 512
    assert not MS.accepted(9000, 9000, 1) and not MS.accepted(70000, 70000, 1) and not MS.accepted(64, 700, 57)        # the refusals test_minsum32_gpu.py pins


def test_the_clean_rule_by_hand():
    deg = np.array([2, 3, 0])
    ok = dict(prior=[1.0, -2.0], alphas=[0.5, 1024.0], clip=20.0, row_deg=deg)
    assert MS.clean(**ok)
    for kw in (dict(alphas=[0.5, 0.0]), dict(alphas=[-0.5]), dict(alphas=[np.nan]), dict(alphas=[1024.0001]), dict(prior=[np.nan, 1.0]), dict(prior=[np.inf, 1.0]),
               dict(prior=[1.0, -1e31]), dict(clip=1e31), dict(row_deg=np.array([2, 1])), dict(flags=(MS.GENERIC,))):
        assert not MS.clean(**{**ok, **kw}), kw
    assert MS.clean(**{**ok, "alphas": [1024.0 + 1e-5]})                       # rounds to 1024 as an f32
    assert MS.next32(1024.0) == 1024.0 + 2.0 ** -13 and MS.next32(MS.TWO100) == 2.0 ** 100 + 2.0 ** 77
    assert [MS.first_block(m, n, 1000) for m, n in ((256, 2055), (257, 64), (64, 2056))] == [256, 512, 512] and MS.first_block(64, 64, 81921) == 1024


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_every_family_sits_where_it_claims(name):
    c = BY_NAME[name]
    e = MS.expected(c)
    print(name, c.m, c.n, e)
    for key in ("accepted", "clean", "first_block"):
        assert e[key] == c.claims[key], key
    assert (e["lds_bytes"] <= MS.LDS_BYTES) == e["accepted"] and c.n < 65535 and c.row_deg.max(initial=0) <= MS.ROW_DEG
    for flags in c.runs:
        assert MS.expected(c, flags)["clean"] == (c.claims["clean"] and MS.GENERIC not in flags)
    if c.claims.get("line") == "clean" or name == "extreme":
        assert not (c.row_deg == 1).any() and np.isfinite(c.prior).all()
    if name == "rows_1500":
        assert (c.row_deg == 0).sum() >= 10 and (c.row_deg == 1).sum() >= 10 and (np.bincount(c.indices, minlength=c.n) == 0).sum() >= 50
        assert -(-c.m // 256) >= 5                                              # the row loop of a 256-thread workgroup takes five or more trips
    if name == "extreme":
        assert np.bincount(c.indices).max() == 300 and np.all(np.abs(c.prior) == MS.TWO100) and c.alpha == ("const", 1024.0) and c.clip == MS.TWO100


@pytest.mark.parametrize("line,near,far", LINES, ids=[t[0] for t in LINES])
def test_the_pair_on_every_line_is_one_step_apart_and_on_opposite_sides(line, near, far):
    a, b = BY_NAME[near], BY_NAME[far]
    ea, eb = MS.expected(a), MS.expected(b)
    if line.startswith("LDS"):
        assert ea["accepted"] and not eb["accepted"] and eb["lds_bytes"] > MS.LDS_BYTES >= ea["lds_bytes"]
        assert (b.m, b.n) in ((a.m + 1, a.n), (a.m, a.n + 1)) and b.nnz == a.nnz
        assert a.n < 65534                                                      # the refusal on the far side is the LDS one, not the u16 one
    elif line.startswith("one"):
        assert b.n == a.n + 1 and (ea["one_wg"], eb["one_wg"]) == (False, True) and (ea["first_block"], eb["first_block"]) == (512, 1024)
    else:
        assert ea["clean"] and not eb["clean"] and np.array_equal(a.indices, b.indices)
        d32 = np.flatnonzero(np.asarray(a.prior).astype(np.float32) != np.asarray(b.prior).astype(np.float32))
        assert (a.alpha != b.alpha) + (a.clip != b.clip) + (d32.size > 0) == 1 and d32.size <= 1
    if near == "prior_rounds_to_2p100":
        assert np.abs(a.prior).max() > MS.TWO100 and np.abs(np.asarray(a.prior).astype(np.float32)).max() == np.float32(MS.TWO100)


@pytest.mark.parametrize("name", ACCEPTED)
def test_model_is_the_scalar_loop_and_the_shots_are_not_trivial(name):
    c = BY_NAME[name]
    synd = MS.shots(c)
    ref = MS.reference(c)
    assert 0 < ref[1].sum() < MS.B, (name, "every family needs a shot that converges and one that does not")
    assert np.all(ref[3][ref[1] == 0] == c.max_iter - 1)
    # ... and one that converges after iteration 0, from messages that are no longer those of the first pass (the families' `light` weights)
    assert ((ref[1] == 1) & (ref[3] >= 1)).any() == (name not in NO_LATE_CONVERGENCE), (name, ref[1], ref[3])
    al = MM.alpha_table32(c.max_iter, c.alpha[0], c.alpha[1])
    for b in (1, 4, 5, 6):
        want = scalar_decode(c.indptr, c.indices, c.n, c.prior, synd[b], c.max_iter, al, c.clip)
        assert same([r[b] for r in ref], want), (name, b)
    if name == "extreme":
        # the bound that licenses the clean form: |V| <= max_col_deg * alpha * max(|prior|, clip) + |prior| < 2^128, so nothing is inf or NaN
        assert np.isfinite(ref[2]).all() and np.abs(ref[2]).max() <= (300 * 1024 + 1) * MS.TWO100 and np.abs(ref[2]).max() > 2.0 ** 110
    if c.claims["clean"]:
        assert np.isfinite(ref[2]).all(), name


def test_the_last_pass_pair_exists():
    """at LAST_PASS['max_iter'] one shot of the pool first satisfies its syndrome in the pass it == max_iter, which only tests (conv 1, iter max_iter - 1), and
    another needs exactly one iteration more (conv 0, the same iter)"""
    c, T = MS.queue_case(), MS.LAST_PASS["max_iter"]
    assert 2 <= T <= 9
    pool = MS.last_pass_pool(c, MS.LAST_PASS["weight"], MS.LAST_PASS["pool"])
    hit, short = MS.LSH.last_pass_pair(lambda s, t: MS.model_decode(c, s, max_iter=t), pool, T)
    print("f32, max_iter", T, "converge in the last pass:", hit.tolist(), "one iteration short:", short.tolist())
    assert hit.size and short.size
    b = int(short[0])
    for t, conv, it in ((T, 0, T - 1), (T + 1, 1, T)):
        got = scalar_decode(c.indptr, c.indices, c.n, c.prior, pool[b], t, MM.alpha_table32(t, "dynamical", 1.0), 20.0)
        assert (got[1], got[3]) == (conv, it)
    got = scalar_decode(c.indptr, c.indices, c.n, c.prior, pool[int(hit[0])], T, MM.alpha_table32(T, "dynamical", 1.0), 20.0)
    assert (got[1], got[3]) == (1, T - 1)
