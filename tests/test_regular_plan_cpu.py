"""The LDS carve of the regular min-sum kernel (csrc/regular_plan.h: pure arithmetic, no HIP header) against a carve restated here (no GPU): a
stand-alone host program (tests/regular_plan_main.cpp) is compiled once with the compiler the library is built with and run on every point below.
The carve ends in the dummy region that the lanes of a block without a team read and write (a padded row of RST doubles, two posteriors, one parity
word); the region rides in the margin the 39 KiB target leaves below a quarter of a CU's 160 KiB, so S is what it was without it."""
import os
import subprocess

import pytest

import regular_shapes as RS

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "qldpc-branched-off_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")          # csrc/Makefile's default
TARGET, CU_LDS = 39 * 1024, 160 * 1024
BB = {"bb72": (36, 72), "bb144": (72, 144), "bb288": (144, 288)}


def carve(cdeg, m, n, max_iter, S):
    """region by region, as the header comment of csrc/regular_plan.h lists them -> dict of byte offsets, `end` = dynamic LDS of the launch"""
    rst = cdeg + 1 if cdeg % 2 == 0 else cdeg
    up8 = lambda x: (x + 7) // 8 * 8
    o = {"R": 0}
    o["V"] = S * m * rst * 8
    o["E"] = o["V"] + S * n * 8
    o["L"] = up8(o["E"] + S * ((n + 3) // 4) * 4)
    o["I"] = o["L"] + S * 8
    o["A"] = up8(o["I"] + (2 * S + 2 + 4 * S) * 4)
    o["T"] = o["A"] + max(max_iter, 1) * 8
    o["D"] = o["T"] + 6 * 8 + 16
    o["end"] = o["D"] + ((rst + 2) * 8 + 4 + 15) // 16 * 16          # row, two posteriors, a 4-byte parity word; whole 16-byte units
    return o


def restated(cdeg, vdeg, m, n, max_iter, threads=RS.LB_T, force=0):
    if m <= 0 or n != 2 * m or m > threads or max_iter > 1024 or (cdeg, vdeg) not in ((6, 3), (4, 2), (8, 4)):
        return None
    S = threads // m
    if 0 < force < S:
        S = force
    while S > 1 and carve(cdeg, m, n, max_iter, S)["D"] > TARGET:
        S -= 1
    o = carve(cdeg, m, n, max_iter, S)
    return (m, S, (S * m + 63) // 64 * 64, o["end"], o["V"], o["E"], o["L"], o["I"], o["A"], o["T"], o["D"])


@pytest.fixture(scope="module")
def library_plan(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("regular_plan") / "regular_plan_main")
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-I", CSRC, os.path.join(HERE, "regular_plan_main.cpp"), "-o", exe], check=True)

    def ask(points):
        text = "".join("%d %d %d %d %d %d %d\n" % p for p in points)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(points)
        return [tuple(int(x) for x in ln.split()[1:]) if ln != "0" else None for ln in out]
    return ask


def test_carve_equals_the_restated_one(library_plan):
    points = []
    for cdeg, vdeg in ((6, 3), (4, 2), (8, 4)):
        for m in list(range(1, 80)) + [127, 128, 129, 170, 171, 255, 256, 257, 511, 512, 513]:
            for max_iter in (0, 1, 2, 50, 1024, 1025):
                for force in (0, 1, 4):
                    points.append((cdeg, vdeg, m, 2 * m, max_iter, RS.LB_T, force))
    points += [(6, 3, 36, 73, 50, RS.LB_T, 0), (6, 2, 36, 72, 50, RS.LB_T, 0), (6, 3, 0, 0, 50, RS.LB_T, 0)]
    got = library_plan(points)
    for p, g in zip(points, got):
        assert g == restated(*p), (p, g, restated(*p))
    assert sum(g is None for g in got) > 0 and sum(g is not None and g[1] > 1 for g in got) > 0


def test_dummy_region_sits_behind_the_tally_and_inside_the_allocation(library_plan):
    for name, (cdeg, vdeg, m, *_rest) in RS.TABLE.items():
        n = m * cdeg // vdeg
        (g,) = library_plan([(cdeg, vdeg, m, n, RS.MAX_ITER, RS.LB_T, 0)])
        if g is None:
            assert m > RS.LB_T, name
            continue
        ts, S, block, lds, offV, offE, offL, offI, offA, offT, offD = g
        rst = cdeg + 1 if cdeg % 2 == 0 else cdeg
        assert offD % 8 == 0 and offD >= offT + 6 * 8                             # behind the six tally words
        assert offD + (rst + 2) * 8 + 4 <= lds and lds - offD <= 96               # the row, the two posteriors and the parity word fit; under 100 bytes
        assert offD <= TARGET or S == 1
        assert 4 * lds <= CU_LDS or S == 1, name                                  # four workgroups per CU still fit
        assert (ts, S, block) == RS.plan(cdeg, m, n)[:3], name                    # the team shapes the domain tests were built for


def test_bb_codes_keep_their_teams(library_plan):
    for tag, (m, n) in BB.items():
        for max_iter in (1, 2, 50):
            (g,) = library_plan([(6, 3, m, n, max_iter, RS.LB_T, 0)])
            assert g[1] == RS.LB_T // m == RS.plan(6, m, n, max_iter)[1], (tag, max_iter, g)
            assert g[3] == RS.plan(6, m, n, max_iter)[3] + 80 <= TARGET            # 80 bytes more than the carve without the region, under 39 KiB
    (g,) = library_plan([(6, 3, 72, 144, 50, RS.LB_T, 0)])
    assert g[1] == 7 and g[10] == 37992 and g[3] == 38072                         # [[144,12,12]], S = 7: dummy region at 37 992, 38 072 bytes in all
