"""The families of tests/lsd_domain_shapes.py without a GPU: the model's answers reach every edge the families are named for (asserted here on the
model, so that tests/test_lsd_domain_gpu.py can hold the kernel to answers that are known to cross them), the star shots also equal their closed form
(which checks the model), every flag-0 answer reproduces its syndrome, `accepted` holds on both sides of every computed edge, and the layout mirror
equals csrc/lsd_plan.h at the families' own (m, n, max_col_deg, max_rows) and their neighbours."""
import os
import subprocess

import numpy as np
import pytest

import lsd_domain_shapes as D
import lsd_shapes as LS
import osd_shapes as OS

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "qldpc-branched-off_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")          # csrc/Makefile's default


def _runs(names=D.NAMES):
    """every (family, bits_per_step, max_rows, shot, info, trace) of the given families"""
    for name in names:
        for bps, cap in D.params(name):
            _, info, traces = D.answers(name, bps, cap)
            for b in range(info.shape[0]):
                yield name, bps, cap, b, tuple(int(v) for v in info[b]), traces[b]


@pytest.mark.parametrize("name", D.NAMES)
def test_flag0_answers_reproduce_the_syndrome_and_are_at_least_half(name):
    f, G, sh = D.family(name), D.graph(name), D.shots(name)
    assert 4 <= sh.synd.shape[0] <= 12
    done = total = 0
    for bps, cap in D.params(name):
        sol, info, traces = D.answers(name, bps, cap)
        assert LS.supported(f.m, f.n, f.max_col_deg, cap) and D.accepted(f.m, f.n, f.max_col_deg, cap)
        for b in range(info.shape[0]):
            total += 1
            if info[b, 0] != 0:
                assert not info[b, 1:].any()
                continue
            done += 1
            assert np.array_equal(G.parity(sol[b]), sh.synd[b] & 1), (name, bps, cap, b)
            assert info[b, 2] <= cap and info[b, 3] == len(traces[b].get("A", [])) == sum(traces[b].get("lists", []))
    print(name, "flag 0:", done, "of", total)
    assert 2 * done >= total


@pytest.mark.parametrize("name", sorted(D.STARS))
def test_star_shots_equal_their_closed_form(name):
    f, sh = D.family(name), D.shots(name)
    assert f.max_col_deg == (2 if D.STARS[name][1] else 1) and np.all(np.diff(f.indptr)[:D.STARS[name][0]] == D.STARS[name][1] + 1)
    assert not sh.hard.any()
    for bps, cap in D.params(name):
        _, info, traces = D.answers(name, bps, cap)
        for b, ranks in enumerate(sh.ranks):
            assert sh.synd[b].sum() == len(ranks)
            want, lists = D.star_closed_form(f, ranks, bps, cap)
            assert tuple(info[b]) == want and traces[b].get("lists", []) == lists, (name, bps, cap, b, info[b], want)


def test_star_edges_are_reached():
    runs = list(_runs(sorted(D.STARS)))
    ok = [r for r in runs if r[4][0] == 0]
    equal = {name: [b for b, rec in enumerate(D.STARS[name][2]) if rec == "equal"] for name in D.STARS}
    lists = lambda rs: {n for r in rs for n in r[5].get("lists", [])}          # noqa: E731
    # the round list on both sides of the LDS capacity, beyond the threads of a workgroup and far beyond; once with every key equal
    assert {128, 129, 257, 1024} <= lists(ok) and max(lists(ok)) == 1024
    assert {128, 129, 257, 1024} <= lists(r for r in ok if r[3] in equal[r[0]])
    assert any(len(set(r[5]["lists"])) > 1 and max(r[5]["lists"]) > LS.LIST_CAP >= min(r[5]["lists"]) for r in ok)      # both forms in one shot
    # final |R| on both sides of the 256 threads; max_rows == |R| beside max_rows == |R| - 1 at 256, 257 and 1024
    assert {256, 257, 258, 1024} <= {r[4][2] for r in ok}
    for size in (256, 257, 1024):
        at = {(r[0], r[1], r[3]) for r in ok if r[2] == size and r[4][2] == size}
        below = {(r[0], r[1], r[3]) for r in runs if r[2] == size - 1 and r[4][0] == 1}
        assert at & below, size
    # all 1024 rows of a matrix at the largest cap
    f = D.family("s512d1")
    assert f.m == 1024 and tuple(D.answers("s512d1", 1, 1024)[1][0]) == (0, 2, 1024, 1024) and tuple(D.answers("s512d1", 2, 1024)[1][0]) == (0, 1, 1024, 1024)
    # 513 seeds: under the cap after round 1, stopped by the rows of round 2
    _, info, traces = D.answers("s513d2", 1, 1024)
    assert D.shots("s513d2").synd[0].sum() == 513 and tuple(info[0]) == (1, 0, 0, 0) and traces[0]["lists"] == [513, 300]
    assert [sum(r for r, _ in cl) for cl in traces[0]["clusters"]] == [513, 813]
    # T b starts as whole words: exactly 64 k seeds
    seeds = {int(D.shots(r[0]).synd[r[3]].sum()) for r in ok}
    assert {64, 128, 192, 256, 320, 512, 1024} <= seeds
    # row degrees around the scan's unroll of four, and the long rows
    assert {1, 2, 3, 4, 5, 8, 301} <= {D.STARS[n][1] + 1 for n in D.STARS}
    long = [r for r in ok if r[0] == "s2d300" and r[1] == 64]
    assert any(max(D.shots("s2d300").ranks[r[3]].values()) > 64 and r[4][1] >= 2 for r in long)
    assert any(r[4][1] > 40 for r in ok if r[0] == "s2d300" and r[1] == 7)      # (and dozens of rounds on one long row)


def test_large_random_wide_heavy_and_tall_edges_are_reached():
    E = D.edges()
    ok = [r for r in _runs(("ident1024", "dep_wide")) if r[4][0] == 0]
    assert any(r[4][2] > 960 for r in ok if r[0] == "ident1024") and any(r[4][2] > 960 for r in ok if r[0] == "dep_wide")      # 16 row words in use
    assert any(max(r[5]["pivots"]) > 8192 for r in ok if r[0] == "dep_wide")
    assert any(max(r[5]["lists"]) > 256 for r in ok) and any(max(r[5]["lists"]) > 256 and r[4][1] > 1 for r in ok)
    f = D.family("dep_wide")
    assert (f.m, f.n, f.max_col_deg) == (D.M_DEP, E.n_wide, E.cd_wide) and LS.layout(f.m, f.n, f.max_col_deg, D.CAP) == LS.LDS_MAX      # the whole 160 KiB
    # the last column index
    f, sh = D.family("u200"), D.shots("u200")
    assert (f.n, f.max_col_deg, D.default_cap("u200")) == (65534, E.cd_u200, E.cap_u200) and E.cap_u200 > 896      # (15 row words)
    assert int(np.argmin(np.abs(sh.llr[0]))) == 65533
    for bps, cap in D.params("u200"):
        _, info, traces = D.answers("u200", bps, cap)
        assert info[0, 0] == 0 and traces[0]["A"][0] == 65533 and 65533 in traces[0]["pivots"]
        assert all(max(t["A"]) > 8192 for t in traces)                       # columns of A beyond the first 256 words of the bit table
    # the heavy column: three seeds, one cluster with all its rows after round 1; the cap below that stops it
    for name in ("heavy64", "heavy65", "heavy130"):
        f, G, sh = D.family(name), D.graph(name), D.shots(name)
        extra = D.TABLE[name][3]
        assert f.max_col_deg == extra and int(np.argmin(np.abs(sh.llr[0]))) == 0
        where = np.searchsorted(G.rows_of(0), sh.rows) // 64
        assert len(set(where)) == min(3, (extra + 63) // 64)                 # (extra = 130: one seed in each of the three chunks)
        for (bps, cap), stopped in zip(D.params(name), (False, True, False)):
            _, info, traces = D.answers(name, bps, cap)
            assert traces[0]["clusters"][0] == [(1, 0)] * 3
            if stopped:
                assert cap < 3 + extra and tuple(info[0]) == (1, 0, 0, 0) and traces[0]["lists"] == [1]
            else:
                assert info[0, 0] == 0 and traces[0]["A"][0] == 0 and max(r for r, _ in traces[0]["clusters"][1]) >= extra
    assert LS.rows_per_round(D.answers("heavy130", 1, 129)[2][0]) == [3]
    # twins: dependent columns with tied keys in a list that is sorted in global scratch -- the lesser index pivots; one ulp apart, the lesser key
    sh = D.shots("twins130")
    sol, info, traces = D.answers("twins130", 2, D.CAP)
    assert [tuple(i) for i in info] == [(0, 1, 130, 260), (0, 1, 130, 260), (0, 1, 64, 128), (0, 1, 65, 130), (0, 1, 130, 260)]
    for b, k in enumerate((130, 130, 64, 65, 130)):
        first = 1 if b == 4 else 0
        assert traces[b]["pivots"] == sorted(traces[b]["pivots"], key=traces[b]["A"].index) and set(traces[b]["pivots"]) == set(range(first, 2 * k, 2))
        assert np.array_equal(np.flatnonzero(sol[b]), np.arange(first, 2 * k, 2))
    assert [tuple(i) for i in D.answers("twins130", 2, 129)[1][[0, 3]]] == [(1, 0, 0, 0), (0, 1, 65, 130)]
    # tall: flag 0 and flag 2 on the largest matrix OSD-0 takes
    f = D.family("tall")
    assert (f.m, f.max_col_deg) == (E.m_tall, E.cd_tall) and OS.rule_path(f.m, f.n, f.max_col_deg).path == "GLOBAL" and (np.diff(f.indptr) == 0).sum() > f.m // 2
    assert {r[4][0] for r in _runs(("tall",))} == {0, 2}


def _edge_points():
    """(m, n, cdeg, max_rows, accepted, layout fits) on both sides of every computed edge"""
    E = D.edges()
    return [(D.M_DEP, E.n_wide, E.cd_wide, D.CAP, True, True), (D.M_DEP, E.n_wide + 1, E.cd_wide, D.CAP, False, False),
            (200, 65534, E.cd_u200, E.cap_u200, True, True), (200, 65534, E.cd_u200, E.cap_u200 + 1, False, False), (200, 65535, E.cd_u200, 1, False, False),
            (E.m_tall, 64, E.cd_tall, 512, True, True), (E.m_tall + 1, 64, E.cd_tall, 512, False, True),
            (65535, 64, E.cd_tall, E.cap_65535, False, True), (65535, 64, E.cd_tall, E.cap_65535 + 1, False, False), (65535, 64, E.cd_tall, 1, False, True),
            (65536, 64, E.cd_tall, 1, False, False), (65535, 300, 4, 384, False, True), (65535, 300, 4, 385, False, False)]


def test_accepted_on_both_sides_of_every_edge():
    E = D.edges()
    assert (E.m_tall, E.cap_65535) == (30710, 384)                           # (what the two mirrors give today; nothing reads these numbers)
    for m, n, cd, rows, ok, fits in _edge_points():
        assert D.accepted(m, n, cd, rows) == ok and LS.supported(m, n, cd, rows) == fits, (m, n, cd, rows)
        assert ok == (fits and not OS.rule_path(m, n, cd).refused)
    assert OS.elim_lds(E.m_tall, 64) <= OS.ELIM_MAX < OS.elim_lds(E.m_tall + 1, 64)
    for name in D.NAMES:                                                     # every family: accepted, and what OSD-0 makes of its flagged shots
        f = D.family(name)
        assert not OS.rule_path(f.m, f.n, f.max_col_deg).refused


def test_layout_mirror_at_the_families(tmp_path):
    exe = str(tmp_path / "lsd_layout_main")
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-I", CSRC, os.path.join(HERE, "lsd_layout_main.cpp"), "-o", exe], check=True)
    points = [p[:4] for p in _edge_points()]
    for name in D.NAMES:
        f = D.family(name)
        for _, cap in D.params(name):
            for dm, dn, dc, dr in ((0, 0, 0, 0), (1, 0, 0, 0), (-1, 0, 0, 0), (0, 1, 0, 0), (0, -1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (0, 0, 0, -1)):
                if cap + dr >= 1 and f.max_col_deg + dc >= 0:
                    points.append((f.m + dm, f.n + dn, f.max_col_deg + dc, cap + dr))
    out = subprocess.run([exe], input="".join("%d %d %d %d\n" % p for p in points), capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(points) > 300
    for p, line in zip(points, out):
        lds, ok, off_misc = (int(x) for x in line.split())
        assert lds == LS.layout(*p) and off_misc == lds - 256 and bool(ok) == LS.supported(*p), (p, line)
