"""The library's own OSD-0 plan (csrc/osd_plan.h: pure arithmetic, no HIP header) against the mirror tests/osd_shapes.py keeps of it (no GPU): a
stand-alone host program (tests/osd_plan_main.cpp) is compiled once with the compiler the library is built with, run once on every point below, and
its (path, W16, block, mode, redo, refused), LDS bytes and second launch must equal osd_shapes.rule_path and the mirror's byte totals -- at the
hand-computed points of test_osd_domain_cpu.py, at every family of the table under every flag set, and on a seeded sweep of the whole range, not only
at the families the GPU tests run."""
import os
import subprocess

import numpy as np

import osd_shapes as OS

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "qldpc-branched-off_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")          # csrc/Makefile's default
ALL_FLAGS = (0,) + OS.FLAG_SETS
SWEEP = 240_000


def hand_points():
    """every (m, n, max_col_deg, flags) that test_rule_path_at_hand_computed_points asks the mirror about, recorded while that test runs, and circ144's"""
    import test_osd_domain_cpu as T
    seen, real = [], OS.rule_path
    OS.rule_path = lambda m, n, cd, flags=0: (seen.append((m, n, cd, flags)), real(m, n, cd, flags))[1]
    try:
        T.test_rule_path_at_hand_computed_points()
    finally:
        OS.rule_path = real
    assert len(seen) >= 40          # (the recording took: that test asks 48 times today)
    return seen + [(1008, 8785, 6, 0)]


def mirror_line(m, n, cd, flags):
    """what the program is to print: rule_path, the first launch's dynamic LDS from the mirror's own byte totals, and the second launch"""
    r = OS.rule_path(m, n, cd, flags)
    cd = max(cd, 1)
    small = (0 if n <= 256 else m * ((n + 63) // 64 + 1) * 8) + 11 * n + 2 * m + 16      # osd0_small_*_kernel: rows (n > 256), keys, order, pivots, solution
    lds = {"NONE": 0, "SMALL": small, "GJ": OS.gj_lds(m, n, cd), "GJG": OS.gjg_lds(m, n, cd), "REFORDER_LDS": OS.reforder_lds(m, n, cd, 1),
           "REFORDER_UG": OS.reforder_lds(m, n, cd, 2), "GLOBAL": OS.elim_lds(m, n)}[r.path]
    second = ("NONE", 0) if not r.redo else ("REFORDER_LDS", OS._wide_block(m)) if r.mode == 1 else ("REFORDER_UG", 1024) if r.mode == 2 else ("GLOBAL", 0)
    return r, "%s %d %d %d %d %d %d %s %d" % (r.path, r.w16, r.block, r.mode, r.redo, r.refused, lds, second[0], second[1])


def sweep_points():
    """m <= 31 000, n <= 66 000, column degree <= 300, the six flag sets; half of the points uniform, half crowded around the sizes where the rule
    changes (128 / 1024 / 4096 rows, 1024 / 65535 columns) so that the narrow classes are met too"""
    rng = np.random.default_rng(OS.SEED)
    h = SWEEP // 2
    m = np.concatenate([rng.integers(0, 31001, h), rng.choice([128, 1024, 4096], h) + rng.integers(-40, 41, h)])
    n = np.concatenate([rng.integers(0, 66001, h), np.where(rng.random(h) < 0.5, rng.choice([1024, 65535], h) + rng.integers(-3, 4, h), rng.integers(0, 66001, h))])
    cd = np.concatenate([rng.integers(0, 301, h), np.where(rng.random(h) < 0.5, rng.integers(0, 13, h), rng.integers(0, 301, h))])
    fl = rng.choice(ALL_FLAGS, SWEEP)
    return list(zip(m.tolist(), n.tolist(), cd.tolist(), fl.tolist()))


def test_plan_equals_the_mirror_everywhere(tmp_path):
    exe = str(tmp_path / "osd_plan_main")
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-I", CSRC, os.path.join(HERE, "osd_plan_main.cpp"), "-o", exe], check=True)
    families = [(f.m, f.n, f.max_col_deg, fl) for f in map(OS.family, OS.TABLE) for fl in ALL_FLAGS]
    points = hand_points() + families + sweep_points()
    assert len(points) >= 200_000 + len(families)
    text = "".join("%d %d %d %d\n" % p for p in points)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(points)
    seen = set()
    for p, line in zip(points, out):
        r, want = mirror_line(*p)
        assert line == want, (p, line, want)
        seen.add((r.path, r.mode, r.redo, r.refused))
    # the sweep met every outcome the rule has -- and never the one it cannot have: a free-pivot kernel with no reference-order form behind it
    assert {s[0] for s in seen} == {"NONE", "SMALL", "GJ", "GJG", "REFORDER_LDS", "REFORDER_UG", "GLOBAL"}
    assert ("NONE", 0, False, True) in seen and ("NONE", 0, False, False) in seen
    assert {("GJ", 1, True, False), ("GJG", 1, True, False), ("GJG", 2, True, False)} <= seen
    assert not [s for s in seen if s[2] and s[1] == 0]
