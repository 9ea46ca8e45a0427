#!/usr/bin/env python3
"""Post-selection on the confidence of BP + LSD, measured on one GPU: does the score predict failure, and what do the statistics cost.

  python tools/kbench_postselect.py [--rates 0.003,0.005] [--trials N] [--batch B] [--rounds R] [--out FILE]
  python tools/kbench_postselect.py --brackets-only TAG [--root TREE] [--build LIB] --out FILE      (one A/B run: appends a line to FILE)
  python tools/kbench_postselect.py --ab-verdict --out FILE                                         (reads those lines, appends the verdict)

Default mode, on circ144 ([[144,12,12]] x 12 cycles; the bundled matrices at p = 0.005, built by the GPU builder at any other p), BP + LSD with
bits_per_step 1 and max_rows 512, one seed:
  * per rate and kind: run_scores over --trials trials; from the per-trial scores the EXACT working point of every abort budget (of the thresholds that
    abort at most x of the trials, the one that aborts most; ties in the score stay together) -> abort rate, LER and binomial standard error; beside
    it the working point the device histogram gives with default_edges(kind), which can only cut at an edge; the share of "no statement" trials.
  * cost with the statistics on: two plans on the same trials, LSD alone and LSD + confidence, alternating --rounds times: the LSD brackets
    (osd_z + osd_x of phase_times) and the judge bracket (which holds the score kernel), ms per batch, median and range.
--brackets-only measures the LSD brackets of an LSD plan WITHOUT a confidence in the tree at --root (default: this one) with the library --build
(a file name in its csrc/, e.g. what tools/ab_build.sh made): run it alternately on a build of the parent commit and of this tree for the cost with
the statistics off.  --ab-verdict holds the difference of the medians against three times the larger run-to-run spread."""
import argparse
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--rates", default="0.003,0.005")
ap.add_argument("--trials", type=int, default=65536)
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--cost-trials", type=int, default=32768)
ap.add_argument("--budgets", default="0,0.01,0.05,0.1,0.2")
ap.add_argument("--out", default=None)
ap.add_argument("--seed", type=int, default=20261021)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--build", default=None)
ap.add_argument("--brackets-only", default=None, metavar="TAG")
ap.add_argument("--ab-verdict", action="store_true")
a = ap.parse_args()
ROOT = os.path.abspath(a.root)
OUT = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r30_postselect.txt")
_log = open(OUT, "a" if (a.brackets_only or a.ab_verdict) else "w")


def say(msg=""):
    print(msg, flush=True)
    _log.write(msg + "\n")
    _log.flush()


if a.ab_verdict:
    runs = {}
    for line in open(OUT):
        f = line.split()
        if len(f) == 8 and f[0] == "ab":
            runs.setdefault(f[1], []).append(float(f[7]))
    import statistics
    say("\ncost with the statistics off: LSD brackets (osd_z + osd_x, ms per batch) of an LSD plan without a confidence, alternating runs")
    for tag, v in runs.items():
        say(f"  {tag}: median {statistics.median(v):.3f}, runs {' '.join('%.3f' % x for x in v)}, spread {max(v) - min(v):.3f}")
    if len(runs) == 2:
        (ta, va), (tb, vb) = runs.items()
        diff, bar = statistics.median(vb) - statistics.median(va), 3 * max(max(va) - min(va), max(vb) - min(vb))
        say(f"  {tb} - {ta} = {diff:+.3f} ms ({100 * diff / statistics.median(va):+.2f} %); three times the larger spread = {bar:.3f} ms: "
            f"{'within' if abs(diff) <= bar else 'OUTSIDE'} the bar")
    sys.exit(0)

sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import qldpc_amd  # noqa: F401,E402
from qldpc_amd import _lib  # noqa: E402
from qldpc_amd.data import load_code, load_precomputed_matrices  # noqa: E402
from qldpc_amd.codes.bb_code import BBCodeCircuit  # noqa: E402
from qldpc_amd.noise.builder import build_decoding_matrices  # noqa: E402
from qldpc_amd.simulation import engine  # noqa: E402

if a.build:
    _lib.select_build(a.build)
T = _lib.TALLY
BITS, ROWS = 1, 512


def problem(p):
    c = load_code("bb144")
    bb = dict(ell=c["ell"], m=c["m_dim"], a_x_powers=c["a_x_powers"], a_y_powers=c["a_y_powers"], b_y_powers=c["b_y_powers"], b_x_powers=c["b_x_powers"])
    pre = load_precomputed_matrices("circ144") if abs(p - 0.005) < 1e-12 else None
    if pre is None:
        pre = build_decoding_matrices(BBCodeCircuit(c["Hx"], c["Hz"], num_cycles=12, **bb), c["Lx"], c["Lz"], p, verbose=False)
    return engine._circuit_problem(c["Hx"], c["Hz"], c["Lx"], c["Lz"], p, 12, pre, 0, bb)


def lsd_plan(prob, batch):
    plan = prob.make_plan(prob.graphs, 50, 1.0, 1.0, "dynamical", batch, 0)
    plan.use_lsd(BITS, ROWS)
    return plan


def spread(v):
    return f"{np.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"


if a.brackets_only:
    prob = problem(0.005)
    plan = lsd_plan(prob, a.batch)
    plan.run(a.seed + 1, 0, 1024); plan.read(clear=True); plan.phase_times()      # warm-up
    plan.run(a.seed, 0, a.cost_trials)
    plan.read(clear=True)
    ph, nb = plan.phase_times()
    plan.close()
    z, x = ph["osd_z"] / nb, ph["osd_x"] / nb
    say(f"ab {a.brackets_only} osd_z {z:.3f} osd_x {x:.3f} sum {z + x:.3f}")
    sys.exit(0)

from qldpc_amd.simulation.postselect import KINDS, PostSelection, default_edges  # noqa: E402

NONE = int(_lib.NO_STATEMENT)
budgets = [float(x) for x in a.budgets.split(",")]


def exact_point(score, outcome, x):
    """of the thresholds t (accept score < t) that abort at most x of the trials, the one that aborts most -> (abort rate, failures, accepted)"""
    counts = np.unique(score, return_counts=True)[1]
    cum_fail = np.concatenate([[0], np.cumsum(outcome[np.argsort(score, kind="stable")] != 0)])      # failures among the n lowest scores
    cum = np.concatenate([[0], np.cumsum(counts)])                            # accepted when the cut falls before the k-th distinct score
    k = int(np.flatnonzero(cum >= (1.0 - x) * score.size - 1e-9)[0])
    return 1.0 - cum[k] / score.size, int(cum_fail[cum[k]]), int(cum[k])


say("post-selection on the confidence of BP + LSD -- tools/kbench_postselect.py")
say(f"circ144 ([[144,12,12]] x 12 cycles), BP (50 iterations, dynamical alpha) + LSD (bits_per_step {BITS}, max_rows {ROWS}); {a.trials} trials per rate, batch {a.batch}; "
    f"ONE seed ({a.seed}); weights = quantise_weights(prior)")
for p in (float(x) for x in a.rates.split(",")):
    prob = problem(p)
    wz, wx = (_lib.quantise_weights(l) for l in prob.llrs)
    plan = lsd_plan(prob, a.batch)
    say(f"\n== p = {p}")
    for kind in KINDS:
        edges = default_edges(kind)
        plan.use_confidence(kind, edges, wz, wx)
        plan.read(clear=True)
        outcome, score = plan.run_scores(a.seed, 0, a.trials)
        tally = plan.read(clear=True)
        ps = PostSelection(plan.confidence_hist(clear=True), edges, kind)
        assert ps.trials == a.trials and int(ps.hist[:, 1:].sum()) == tally[T["total_err"]] == np.count_nonzero(outcome)
        silent = int((score == np.uint64(NONE)).sum())
        say(f"[{kind}] no statement {silent} / {a.trials} ({silent / a.trials:.5f}); score 0 (no cluster at all) {int((score == 0).sum())}; "
            f"distinct scores {np.unique(score).size}; {edges.size + 1} default bins")
        lers = []
        for x in budgets:
            ab, f, acc = exact_point(score, outcome, x)
            ler = f / acc if acc else float("nan")
            se = np.sqrt(ler * (1 - ler) / acc) if acc else float("nan")
            at = ps.at_abort_rate(x)
            lers.append(ler)
            say(f"    abort <= {x:<5g}: exact cut aborts {ab:.4f}, LER {ler:.5f} +- {se:.5f} ({f} / {acc});  default bins abort {at['abort_rate']:.4f}, "
                f"LER {at['ler']:.5f} +- {at['std_error']:.5f}")
        say(f"    LER at the largest budget / LER without post-selection = {lers[-1] / lers[0]:.3f}" + ("  (does NOT separate)" if not lers[-1] < lers[0] else ""))
    plan.close()

say(f"\n== cost with the statistics on: circ144 p = 0.005, {a.cost_trials} trials per run, batch {a.batch}, {a.rounds} alternating rounds; ms per batch, median (range)")
prob = problem(0.005)
wz, wx = (_lib.quantise_weights(l) for l in prob.llrs)
plans = {"lsd": lsd_plan(prob, a.batch), "lsd+confidence": lsd_plan(prob, a.batch)}
plans["lsd+confidence"].use_confidence("llr_2", default_edges("llr_2"), wz, wx)
ms = {n: {"lsd": [], "judge": [], "rate": []} for n in plans}
tallies = {}
for plan in plans.values():
    plan.run(a.seed + 1, 0, 1024); plan.read(clear=True); plan.phase_times()      # warm-up
for rnd in range(a.rounds):
    for name, plan in plans.items():
        t0 = time.perf_counter()
        plan.run(a.seed, 0, a.cost_trials)
        tallies[name] = plan.read(clear=True)
        dt = time.perf_counter() - t0
        ph, nb = plan.phase_times()
        ms[name]["lsd"].append((ph["osd_z"] + ph["osd_x"]) / nb)
        ms[name]["judge"].append(ph["judge"] / nb)
        ms[name]["rate"].append(a.cost_trials / dt)
assert np.array_equal(tallies["lsd"], tallies["lsd+confidence"])
for name in plans:
    say(f"[{name}] LSD brackets (osd_z + osd_x) {spread(ms[name]['lsd'])};  judge bracket {spread(ms[name]['judge'])};  {np.median(ms[name]['rate']):.4g} trials/s")
d_lsd = np.median(ms["lsd+confidence"]["lsd"]) - np.median(ms["lsd"]["lsd"])
d_judge = np.median(ms["lsd+confidence"]["judge"]) - np.median(ms["lsd"]["judge"])
say(f"    statistics on - off: LSD brackets {d_lsd:+.3f} ms ({100 * d_lsd / np.median(ms['lsd']['lsd']):+.2f} %), judge bracket {d_judge:+.3f} ms per batch of {a.batch}")
for plan in plans.values():
    plan.close()
_log.close()
