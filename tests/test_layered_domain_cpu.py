"""CPU suite of the layered decoder's domain (tests/layered_shapes.py): the restated host rules on the bundled matrices, every family where it claims
to sit, the pair on every line on opposite sides of it, the numpy model (tests/layered_model.py) against the literal serial loop of
tests/test_layered_cpu.py on every new family (none is skipped), what the equal-magnitude shots can and cannot see, and the last-pass pair."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_shapes as GS  # noqa: E402
import layered_model as LM  # noqa: E402
import layered_shapes as LSH  # noqa: E402
from test_layered_cpu import SIZES, same, sector, serial_decode  # noqa: E402

CASES = LSH.all_cases()
BY_NAME = {c.name: c for c in CASES}
ACCEPTED = [c.name for c in CASES if c.claims["form"] is not None]
# (line, the family on its near side, the family on its far side, what the two differ in)
LINES = [("V | VG, by n at m = 300", "v_last", "vg_first", "n"), ("u16 | i32 indices", "n65535", "n65536", "n"),
         ("V+idx | V, by nnz at n = 16000", "idx_last", "idx_global_first", "nnz"), ("VG+idx | VG, by nnz at n = 24000", "vg_idx_last", "vg_only_first", "nnz"),
         ("V | VG, by rows at n = 64", "rows_v_last", "rows_vg_first", "rows"), ("VG | refused, by rows at n = 64", "rows_vg_last", "rows_refused", "rows"),
         ("block 256 | 512", "block_nnz512", "block_nnz513", "nnz"), ("block 512 | 1024", "block_nnz1024", "block_nnz1025", "nnz")]


# families in which the model finds no shot that converges later than iteration 0, at an error weight of 1 .. 9 on top of the prior's hard decision
NO_LATE_CONVERGENCE = {"rows_v_last": "n = 64 with some 175 rows of degree 2 per column: a consistent syndrome is decoded in the first iteration", "rows_vg_first": "as rows_v_last",
                       "rows_vg_last": "as rows_v_last", "no_edges": "no message at all"}


# what check() of tests/test_layered_gpu.py reads from qldpc_layered_decoder_info on the bundled matrices: LDS bytes, threads, workgroups per CU, the lg set
BUNDLED = {("circ72", "Z"): (40864, 256, 3, {3, 4}), ("circ72", "X"): (42304, 256, 3, {3, 4, 6}),
           ("circ144", "Z"): (158880, 1024, 1, {3, 4, 5, 6}), ("circ144", "X"): (161824, 1024, 1, {3, 4, 5})}


@pytest.mark.parametrize("tag,s", sorted(SIZES))
def test_restated_rules_on_the_bundled_matrices(tag, s):
    """what tests/test_layered_gpu.py pins on circ72 / circ144: everything in LDS, the layer count of the greedy colouring, the figures above"""
    ip, ix, n, prior = sector(tag, s)
    c = LSH._case(f"{tag}{s}", ip, ix, n, None, {})
    e = LSH.expected(c)
    assert e["accepted"] and e["form"] == "V+idx" and not e["v_global"] and e["lds_indices"] and e["layers"] == len(SIZES[(tag, s)])
    assert (e["lds_bytes"], e["block"], e["grid_per_cu"], e["lgs"]) == BUNDLED[(tag, s)]


def test_restated_rules_on_the_graph_shapes():
    """... and on the structured graphs: hub_col has a layer per row, vglobal_beyond_* move the posteriors out"""
    fam = {c.name: c for c in GS.families()}
    for name, vg in (("vglobal_beyond_plain", True), ("vglobal_beyond_damped", True), ("hub_col", False)):
        f = fam[name]
        e = LSH.expected(LSH._case(name, f.indptr, f.indices, f.n, None, {}))
        assert e["accepted"] and e["v_global"] == vg, name
        if name == "hub_col":
            assert e["layers"] == 300 and e["max_layer_rows"] == 1
    f = fam["rowdeg57"]
    assert not LSH.expected(LSH._case("rowdeg57", f.indptr, f.indices, f.n, None, {}))["accepted"]
    assert LSH.form(6000, 6000, 1, 6000)[0] is None                            # the refusal tests/test_layered_gpu.py pins: 6000 rows of degree 1


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_every_family_sits_where_it_claims(name):
    c = BY_NAME[name]
    e = LSH.expected(c)
    print(name, {k: e[k] for k in ("form", "lds_bytes", "block", "lgs", "layers", "nslots", "grid_per_cu")})
    assert e["form"] == c.claims["form"] and e["accepted"] == (c.claims["form"] is not None)
    assert e["block"] == c.claims["block"] and e["lgs"] == c.claims["lgs"]
    for key in ("stops", "wraps"):
        if key in c.claims:
            assert e[key] == c.claims[key], key
    assert (e["lds_bytes"] <= LSH.LDS_BYTES) == e["accepted"]
    assert np.all(np.diff(c.indptr) <= LSH.ROW_DEG) and LM.layers_valid(c.indptr, c.indices, c.n, LSH.structure(c.indptr, c.indices, c.n, c.row_layer)[0])
    for i in range(c.m):                                                       # canonical CSR
        assert np.all(np.diff(c.indices[c.indptr[i]:c.indptr[i + 1]]) > 0)


@pytest.mark.parametrize("line,near,far,axis", LINES, ids=[t[0] for t in LINES])
def test_the_pair_on_every_line_is_one_step_apart_and_on_opposite_sides(line, near, far, axis):
    a, b = BY_NAME[near], BY_NAME[far]
    ea, eb = LSH.expected(a), LSH.expected(b)
    if axis == "n":
        assert b.n == a.n + 1 and np.array_equal(a.indices, b.indices) and np.array_equal(a.indptr, b.indptr)
    elif axis == "nnz":
        assert b.nnz == a.nnz + 1 and (a.n, a.m, ea["layers"]) == (b.n, b.m, eb["layers"])
    else:
        assert eb["nslots"] == ea["nslots"] + 1 and a.n == b.n
    if "block" in line:
        assert (ea["block"], eb["block"]) == tuple(int(x) for x in line[6:].split(" | "))
        assert a.nnz // ea["layers"] in (512, 1024) and ea["layers"] == 1
    else:
        assert ea["form"] != eb["form"] and LSH.FORMS.index(ea["form"]) < (LSH.FORMS.index(eb["form"]) if eb["form"] else 4)
    if far == "rows_refused":
        assert not eb["accepted"] and ea["form"] == "VG" and eb["lds_bytes"] > LSH.LDS_BYTES >= ea["lds_bytes"]


def test_the_lane_rule_by_hand():
    """lane_bits at the values the header's sentence gives: eight edges per lane first, then doubling under the three conditions"""
    assert [LSH.lane_bits(1000, d, 256)[0] for d in (1, 8, 9, 16, 17, 32, 33, 56)] == [0, 0, 1, 1, 2, 2, 3, 3]          # nothing fits beside: the minimum
    assert LSH.lane_bits(1, 56, 256) == (6, "edge") and LSH.lane_bits(4, 33, 256) == (6, "edge") and LSH.lane_bits(5, 56, 256) == (5, "fit")
    # the cap alone stops nothing at a degree the decoder accepts: over every (rows, degree <= 56, workgroup size) it is never the reason
    assert not any(LSH.lane_bits(cnt, d, blk)[1] == "cap" for cnt in range(1, 40) for d in range(1, LSH.ROW_DEG + 1) for blk in (256, 512, 1024))
    assert LSH.lane_bits(1, 65, 256) == (6, "cap")                             # ... it would be for a row of 65 edges, which creation refuses
    assert LSH.lane_bits(16, 56, 256) == (4, "fit") and LSH.lane_bits(17, 56, 256) == (3, "fit") and LSH.lane_bits(2, 5, 256) == (3, "edge")
    assert LSH.lane_bits(64, 8, 256) == (2, "fit") and LSH.lane_bits(64, 8, 512) == (3, "edge") and LSH.lane_bits(3, 1, 1024) == (0, "edge")
    assert [LSH.block(z, 1) for z in (0, 512, 513, 1024, 1025)] == [256, 256, 512, 512, 1024] and LSH.block(2049, 2) == 512 and LSH.block(0, 0) == 256
    assert LSH.grid_per_cu(6032, 256) == 8 and LSH.grid_per_cu(6032, 1024) == 2 and LSH.grid_per_cu(100000, 256) == 1 and LSH.grid_per_cu(163328, 1024) == 1


@pytest.mark.parametrize("name", ACCEPTED)
def test_model_is_the_serial_loop_and_the_shots_are_not_trivial(name):
    """two shots per prior against tests/test_layered_cpu.serial_decode in (layer, row) order; with the uniform prior the two shots whose first pass
    ties in every check (a single 1, all zero)"""
    c = BY_NAME[name]
    synd = LSH.shots(c)
    assert len({s.tobytes() for s in synd}) >= (7 if c.nnz else 4)        # (the prior's own syndrome is the zero one where no prior entry is negative)
    order = np.argsort(LSH.structure(c.indptr, c.indices, c.n, c.row_layer)[0], kind="stable")
    for pn, picks in (("normal", (1, 6)), ("uniform", (4, 7))):
        ref = LSH.reference(c, pn)
        assert 0 < ref[1].sum() < LSH.B, (name, pn, "every family needs a shot that converges and one that does not")
        if pn == "normal":                                                     # (under the uniform prior the ties are the point, not the convergence)
            assert ((ref[1] == 1) & (ref[3] >= 1)).any() == (name not in NO_LATE_CONVERGENCE), (name, ref[1], ref[3])
        for b in picks:
            want = serial_decode(c.indptr, c.indices, c.n, c.priors[pn], synd[b], order, c.max_iter, LM.alpha_table(c.max_iter, "dynamical", 1.0), 20.0)
            assert same([r[b] for r in ref], want), (name, pn, b)


# ---------------------------------------------------------------------------------------- equal magnitudes
class LastPosition(LM.LayeredModel):
    """the model with an argmin that names the LAST position of a tied minimum"""
    @staticmethod
    def two_minima(ab):
        pos = ab.shape[2] - 1 - np.argmin(ab[:, :, ::-1], axis=2)
        min1 = np.take_along_axis(ab, pos[..., None], axis=2)[..., 0]
        rest = ab.copy()
        np.put_along_axis(rest, pos[..., None], np.inf, axis=2)
        return pos, min1, rest.min(axis=2)


class LosesTheTwin(LM.LayeredModel):
    """the model with a combine that takes a second copy of the minimum for the same element: min2 becomes the smallest value ABOVE min1"""
    @staticmethod
    def two_minima(ab):
        pos, min1, _ = LM.LayeredModel.two_minima(ab)
        return pos, min1, np.where(ab > min1[..., None], ab, np.inf).min(axis=2)


@pytest.mark.parametrize("name", ["lanes_wrap", "lanes_mixed", "lanes_whole_wave", "core300"])
def test_what_the_equal_magnitude_shots_see(name):
    """With a uniform prior every |Q| of the first pass is equal, in every check and across all the lanes of a check.  What that pins is min2: the
    minimum occurs twice, so min2 = min1, and a cross-lane combine that drops the second copy of a tied minimum changes the posteriors -- asserted
    here on the model.  What it cannot pin is WHICH tied position the argmin names: wherever two positions tie for the minimum, min2 = min1 and every
    edge gets the same magnitude, so 'last position' gives the same bits as 'first position' on any input -- asserted here too, which is why no
    test of this suite tries to tell the two apart."""
    c = BY_NAME[name]
    synd = LSH.shots(c)[[4, 7]]
    make = lambda cls: cls(c.indptr, c.indices, c.n, c.priors["uniform"], row_layer=c.row_layer)      # noqa: E731
    ref = make(LM.LayeredModel).decode(synd, max_iter=c.max_iter)
    assert same(ref, [r[[4, 7]] for r in LSH.reference(c, "uniform")])
    assert same(make(LastPosition).decode(synd, max_iter=c.max_iter), ref)
    lost = make(LosesTheTwin).decode(synd, max_iter=c.max_iter)
    assert not np.array_equal(lost[2], ref[2], equal_nan=True)
    # on a prior without ties the last-position model is still the model (no tie, one argmin): the subclass changes nothing but the tie rule
    normal = lambda cls: cls(c.indptr, c.indices, c.n, c.priors["normal"], row_layer=c.row_layer).decode(LSH.shots(c)[[1]], max_iter=c.max_iter)  # noqa: E731
    assert same(normal(LastPosition), normal(LM.LayeredModel))


# ---------------------------------------------------------------------------------------- the last pass
def test_the_last_pass_pair_exists():
    """at LAST_PASS['max_iter'] one shot of the pool first satisfies its syndrome after the last layer of the last iteration (conv 1, iter max_iter - 1) and
    another needs exactly one iteration more (conv 0, the same iter)"""
    c, T = LSH.queue_graph(), LSH.LAST_PASS["max_iter"]
    assert 2 <= T <= 9
    pool = LSH.last_pass_pool(c, LSH.LAST_PASS["weight"], LSH.LAST_PASS["pool"])
    model = LM.LayeredModel(c.indptr, c.indices, c.n, c.priors["normal"])
    hit, short = LSH.last_pass_pair(lambda s, t: model.decode(s, max_iter=t), pool, T)
    print("layered, max_iter", T, "converge in the last pass:", hit.tolist(), "one iteration short:", short.tolist())
    assert hit.size and short.size
    b = int(short[0])
    order = np.argsort(model.row_layer, kind="stable")
    for t, conv, it in ((T, 0, T - 1), (T + 1, 1, T)):
        got = serial_decode(c.indptr, c.indices, c.n, c.priors["normal"], pool[b], order, t, LM.alpha_table(t, "dynamical", 1.0), 20.0)
        assert (got[1], got[3]) == (conv, it)
    got = serial_decode(c.indptr, c.indices, c.n, c.priors["normal"], pool[int(hit[0])], order, T, LM.alpha_table(T, "dynamical", 1.0), 20.0)
    assert (got[1], got[3]) == (1, T - 1)
