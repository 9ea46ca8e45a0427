"""The OSD-CS cases of tests/osd_cs_shapes.py without a GPU.  The library's own layout (osd_cs_layout, csrc/osd_plan.h: pure arithmetic, no HIP header) is
printed by a stand-alone host program (tests/osd_cs_layout_main.cpp, compiled with the compiler the library is built with) and held against the mirror
cs_layout at every family and order, at hand-computed points on both sides of every edge and on a seeded sweep of the whole range.  With the numpy model
alone: every family has the rank, non-pivot count, row words, threads and sort forms it is labelled with, every shot lies on the side of the column space
its class says, and OSD-0, a single and a pair each win somewhere under every weight set, on a family of each sort form."""
import os
import subprocess

import numpy as np
import pytest

import osd_cs_model as M
import osd_cs_shapes as CS
import osd_shapes as OS

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "qldpc-branched-off_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")          # csrc/Makefile's default
SWEEP = 200_000
# (m, n, order) -> (lds bytes, sort in global memory), worked out on paper from osd_cs_layout; the tail behind U is
# 128 + 2 * round_up(2 m, 8) + 64 * 8 mw + max(order, 1) * 8 mw + round_up(4 * ceil(n / 32), 16) + 2048 + 16
HAND = {
    # m = 130 (3 words), order 0: tail 128 + 528 + 1536 + 24 + 1488 + 2064 = 5768; sort scratch round_up(12 n + 16528, 16) = 158064 at n = 11794
    (130, 11794, 0): (163832, False), (130, 11794, 1): (163832, False),
    (130, 11794, 2): (3168 + 5792, True),                            # 24 bytes of TR more: 163856 > 163840, so U alone (132 * 3 * 8 = 3168)
    (130, 11795, 0): (3168 + 5768, True),                            # 12 * 11795 + 16528 = 158068 -> 158080, + 5768 = 163848
    # m = 1024 (16 words), U = 1026 * 128 = 131328.  order 0: tail 128 + 4096 + 8192 + 128 + 1376 + 2064 = 15984, sort 12 * 10944 + 16528 = 147856
    (1024, 10944, 0): (163840, False), (1024, 10945, 0): (131328 + 15984, True),
    # order 64: TR 8192, pflag 1296: tail 23968; sort 12 * 10278 + 16528 = 139864 -> 139872
    (1024, 10278, 64): (163840, False), (1024, 10279, 64): (131328 + 23968, True), (1024, 10279, 63): (139888 + 23840, False),
    (1024, 10600, 0): (143728 + 15936, False), (1024, 10600, 64): (131328 + 24000, True),          # pflag 1328
    # the largest accepted matrix at the largest order: pflag 8192, tail 30864
    (1024, 65535, 64): (162192, True), (1, 1, 0): (16544 + 128 + 8 + 8 + 512 + 8 + 16 + 2064, False),
    # beyond what OSD-CS accepts, where the layout itself gives up: m = 1100 has 18 words, U = 1102 * 144 = 158688
    (1100, 100, 0): (0, None),
}


def test_mirror_at_hand_computed_points():
    for (m, n, order), (lds, gsort) in HAND.items():
        assert CS.cs_layout(m, n, order)[:2] == (lds, gsort), (m, n, order, CS.cs_layout(m, n, order))
    assert (CS.N_CS_130_0, CS.N_CS_1024_0, CS.N_CS_1024_64) == (11794, 10944, 10278)          # the sort goes to global memory at 11795 / 10945 / 10279
    assert CS.N_CS_1024_64 < CS.N_CS_MID <= CS.N_CS_1024_0
    assert [CS.cs_layout(m, 640, 7)[2] for m in (1, 254, 255, 318, 319, 958, 959, 1024)] == [256, 256, 320, 320, 384, 960, 1024, 1024]
    assert CS.cs_accepts(1024, 65535) and not CS.cs_accepts(1025, 100) and not CS.cs_accepts(100, 65536)


def mirror_line(m, n, order):
    lds, gsort, block = CS.cs_layout(m, n, order)
    offs = CS.cs_offsets(m, n, order, gsort is not False)[0]          # (a refusal leaves the offsets of the last form tried)
    return "%d %d %d " % (lds, bool(gsort), block) + " ".join(map(str, offs))


def sweep_points():
    """m <= 1100, n <= 66 000, every order: a third uniform, a third with m and n crowded around the sizes where something changes, a third at most three
    columns from the edge between the two sort forms of their (m, order)"""
    rng = np.random.default_rng(OS.SEED)
    t = SWEEP // 3
    edge_m = np.array([1, 63, 64, 65, 130, 254, 255, 958, 959, 960, 961, 1008, 1022, 1023, 1024])
    order = np.concatenate([rng.integers(0, 65, 2 * t), rng.choice([0, 1, 2, 7, 63, 64], t)])
    m = np.concatenate([rng.integers(1, 1101, t), np.clip(rng.choice([64, 256, 960, 1024], t) + rng.integers(-3, 4, t), 1, None), rng.choice(edge_m, t)])
    n = np.concatenate([rng.integers(1, 66001, t), np.clip(rng.choice([64, 10279, 10945, 11795, 65535], t) + rng.integers(-3, 4, t), 1, None), np.zeros(t, np.int64)])
    edges = {}
    for i in range(2 * t, 3 * t):
        key = (int(m[i]), int(order[i]))
        if key not in edges:
            edges[key] = CS.n_edge(*key)
        n[i] = edges[key] + rng.integers(-2, 4)
    return list(zip(m.tolist(), n.tolist(), order.tolist()))


def test_layout_equals_the_mirror_everywhere(tmp_path):
    exe = str(tmp_path / "osd_cs_layout_main")
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-I", CSRC, os.path.join(HERE, "osd_cs_layout_main.cpp"), "-o", exe], check=True)
    families = [(f.m, f.n, o) for f in map(CS.family, CS.TABLE) for o in sorted(set(CS.EDGE_ORDERS + tuple(f.orders)))]
    points = list(HAND) + families + sweep_points()
    assert len(points) >= SWEEP - 2 + len(families)
    out = subprocess.run([exe], input="".join("%d %d %d\n" % p for p in points), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(points)
    forms = {False: 0, True: 0, None: 0}
    for p, line in zip(points, out):
        assert line == mirror_line(*p), (p, line, mirror_line(*p))
        gsort = CS.cs_layout(*p)[1]
        forms[gsort] += 1
        # no matrix OSD-CS accepts by size is refused for LDS, at any order: the refusal branch of osdcs_layout (csrc/osd_cs.hip) is not reached
        assert gsort is not None or p[0] > 1024, p
    assert forms[False] > 10_000 and forms[True] > 10_000 and forms[None] > 1_000
    for (m, n, order), (lds, gsort) in HAND.items():
        assert out[points.index((m, n, order))].split()[:2] == [str(lds), str(int(bool(gsort)))]


def test_the_largest_layout_with_the_sort_in_global_memory_fits():
    """why that branch cannot be reached: the global-sort form grows with m, n and the order, and at the largest of all three it is 162 192 bytes"""
    assert CS.cs_offsets(1024, 65535, 64, True)[1] == 162192 <= OS.LDS_MAX
    for m, n, order in ((1024, 65535, 64), (1023, 65535, 64), (961, 65535, 64), (1024, 1, 64)):
        assert CS.cs_offsets(m, n, order, True)[1] <= 162192


def test_weight_sets():
    for name in ("m254", "cs130_nover", "m1x70", "empty130x20"):
        f = CS.family(name)
        pri, eq, mix = (CS.weights(f, k) for k in CS.WEIGHT_SETS)
        assert (pri > 0).all() and np.unique(pri).size == f.n
        assert (eq == 1.0).all()
        q = M.quantise(mix)
        assert np.isfinite(mix).all() and (mix < 0).any() and (mix == 0).any() and (q == 0).any()
        assert (q == 2 ** 40).sum() == 2 and (q == -(2 ** 40)).sum() == 2 and (np.abs(mix) == 3e6).sum() == 2 and (np.abs(mix) == 1e300).sum() == 2


@pytest.mark.parametrize("name", list(CS.TABLE))
def test_family_labels_and_sides_of_the_column_space(name):
    """the labels against the mirror and the model; the random syndrome is outside the column space on every shot (by the model and by the family's own
    witness) and no other class is, on any shot"""
    f = CS.family(name)
    assert (f.m + 63) // 64 == f.mw and OS._wide_block(f.m) == f.block and CS.cs_layout(f.m, f.n, 0)[2] == f.block
    assert f.rank + f.nonpivot == f.n
    assert CS.cs_accepts(f.m, f.n) == (not f.refused)
    if f.refused:
        e = M.eliminate(CS.model_graph(f), np.zeros(f.m, np.int8), np.zeros(f.n), np.zeros(f.n, np.int8))
        assert len(e["pivots"]) == f.rank
        return
    assert "".join("G" if CS.cs_layout(f.m, f.n, o)[1] else "L" for o in f.orders) == f.forms
    s, elims = CS.batch(name), CS.eliminations(name)
    assert len(elims) == len(s.cls) == f.per_class * len(CS.classes_of(f))
    assert ("random syndrome" in s.cls) == (f.rank < f.m and f.null_rows is not None)
    for b, e in enumerate(elims):
        assert len(e["pivots"]) == f.rank, (name, b)
        assert e["outside"] == (s.cls[b] == "random syndrome"), (name, b, s.cls[b])
    if f.null_rows is not None:
        assert np.array_equal(OS.outside(f, s.synd ^ OS._syndromes(f, s.hard)), s.cls == "random syndrome")
    settled = s.cls == "settled"
    assert np.array_equal(OS._syndromes(f, s.hard[settled]), s.synd[settled])
    if f.kind == "identfirst":         # three whole chunks of identity columns lead the order wherever the |llr| are not all equal
        for b in np.flatnonzero(s.cls == "sparse error"):
            assert (np.sort(M.column_order(s.llr[b])[:f.m]) == np.arange(f.n - f.m, f.n)).all()
    if name == "tall300x41":
        A = OS.dense(f)
        assert np.array_equal(A[:, 0], A[:, 40])
    if name == "h300_d290":
        assert f.max_col_deg == 290


@pytest.mark.parametrize("form", ["L", "G"])
@pytest.mark.parametrize("wset", CS.WEIGHT_SETS)
def test_every_kind_of_winner_occurs(form, wset):
    """conditions on the inputs, by the model alone: OSD-0 kept, a single and a pair each win at least once among the family's shots"""
    name = CS.WINNER_FAMILIES[form]
    f = CS.family(name)
    assert set(f.forms) == {form}
    seen = {"osd0": 0, "single": 0, "pair": 0}
    for order, (sol, flips, outside, osd0, cost) in CS.answers(name, wset).items():
        for k, v in CS.winners(flips, outside).items():
            seen[k] += v
        if order <= 1:
            assert (flips[:, 1] == -1).all()
    assert min(seen.values()) > 0, (name, wset, seen)


def test_shared_eliminations_score_as_the_model_does():
    """the helper that scores one elimination under every weight set and order gives what M.osd_cs_batch gives from scratch"""
    for name, wset, order in (("n65", "mixed", 7), ("m65x150", "equal", 64), ("tall300x41", "priors", 2)):
        f, s = CS.family(name), CS.batch(name)
        sol, flips, outside, osd0, cost = CS.answers(name, wset)[order]
        msol, mflips, mout, mosd0 = M.osd_cs_batch(CS.model_graph(f), s.synd, s.llr, s.hard, CS.weights(f, wset), order)
        assert np.array_equal(outside, mout) and np.array_equal(osd0, mosd0) and np.array_equal(flips, mflips)
        assert np.array_equal(sol[~outside], msol[~outside]) and np.array_equal(sol[outside], mosd0[outside])


def test_big_batches():
    f = CS.family(CS.BIG_FAMILY)
    assert CS.BIG_BATCH > 512
    s = CS.big_batch("classes")
    assert len(s.cls) == CS.BIG_BATCH and set(s.cls) == set(CS.classes_of(f)) and "random syndrome" in s.cls
    out = OS.outside(f, s.synd ^ OS._syndromes(f, s.hard))
    assert np.array_equal(out, s.cls == "random syndrome")
    o = CS.big_batch("outside")
    assert o.synd.shape[0] == CS.BIG_BATCH and OS.outside(f, o.synd ^ OS._syndromes(f, o.hard)).all()
