#!/usr/bin/env python3
"""Two-pass correlated decoding against independent sectors on one GPU: what the per-shot-prior kernel costs, what the links cost, what they are worth.

  python tools/kbench_correlated.py [--rates 0.003,0.005] [--trials N] [--batch B] [--no-dem] [--out FILE]

Problems: the circ144 circuit plan ([[144,12,12]] x 12 cycles; the bundled matrices at p = 0.005, built by the GPU builder at any other p) at every
rate of --rates, and the two-sector detector error model of from_decoding_matrices("circ144") as a control: its columns fire independently, so its link
table is empty by construction and (b), (c) must agree trial for trial.
Five plans per problem on the same seed and trial range:
  (a) flood      the default plan (flooding min-sum with the dynamical alpha, OSD-0): never switched, so it enqueues what the parent commit enqueues
  (b) nolinks    use_correlated(alpha, links=None): the per-shot-prior kernel in both BP brackets, nothing to raise
  (c) raise      use_correlated with links_from_circuit / links_from_dem, mode "raise"
  (d) condition  the same with mode "condition" (base = the conditional prior)
  (e) raise+cs7  (c) with OSD-CS of order 7 in the OSD stage
Printed per plan: trials/s of run(), the six phase brackets in ms per batch, BP converged per sector, Z / X / total logical errors with binomial standard
errors; then the number of trials whose verdict differs between (b) and (c), from run_outcomes on the same range, split by who was right.
(b) against (a) is what the kernel costs (another algorithm: constant alpha through the shared leg), (c) against (b) what the links cost and are worth.
Everything printed is also written to --out (default profiles/r25_correlated.txt)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import qldpc_amd  # noqa: F401,E402
from qldpc_amd import _lib  # noqa: E402
from qldpc_amd.data import load_code, load_precomputed_matrices  # noqa: E402
from qldpc_amd.codes.bb_code import BBCodeCircuit  # noqa: E402
from qldpc_amd.noise.builder import build_decoding_matrices  # noqa: E402
from qldpc_amd.simulation import correlated, engine  # noqa: E402
from qldpc_amd.simulation.dem import DetectorErrorModel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rates", default="0.003,0.005")
ap.add_argument("--trials", type=int, default=32768)
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--alpha", type=float, default=1.0)
ap.add_argument("--no-dem", action="store_true")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_correlated.txt"))
ap.add_argument("--seed", type=int, default=20261020)
a = ap.parse_args()
T = _lib.TALLY
NAMES = ("flood", "nolinks", "raise", "condition", "raise+cs7")
_log = open(a.out, "w")


def say(msg=""):
    print(msg, flush=True)
    _log.write(msg + "\n")
    _log.flush()


def rate(k, n):
    p = k / max(n, 1)
    return f"{p:.4g} +- {np.sqrt(p * (1 - p) / max(n, 1)):.2g} ({int(k)})"


def measure(make_plan, links):
    """the five plans in turn on [0, trials): tally, trials/s and phase times of run(); then the verdicts of (b) and (c)"""
    verdicts = {}
    for name in NAMES:
        plan = make_plan()
        if name == "raise+cs7":
            plan.use_osd_cs(7)
        if name != "flood":
            lk = None if name == "nolinks" else links["condition" if name == "condition" else "raise"]
            plan.use_correlated(a.alpha, lk, None if lk is None else lk.base)
        plan.run(a.seed + 1, 0, min(a.batch, 1024)); plan.read(clear=True); plan.phase_times()       # warm-up
        t0 = time.perf_counter()
        plan.run(a.seed, 0, a.trials)
        t = plan.read(clear=True)
        dt = time.perf_counter() - t0
        ph, nb = plan.phase_times()
        n = int(t[T["trials"]])
        say(f"[{name:10s}] {a.trials / dt:9.4g} trials/s;  ms per batch: " + "  ".join(f"{k} {v / max(nb, 1):.2f}" for k, v in ph.items()))
        say(f"             BP converged Z {t[T['bp_conv_z']] / n:.4f} X {t[T['bp_conv_x']] / n:.4f};  logical errors Z {rate(t[T['z_err']], n)}  "
            f"X {rate(t[T['x_err']], n)}  total {rate(t[T['total_err']], n)}")
        if name in ("nolinks", "raise"):
            verdicts[name] = plan.run_outcomes(a.seed, 0, a.trials)
            plan.read(clear=True)
        plan.close()
    b, c = verdicts["nolinks"], verdicts["raise"]
    diff = b != c
    say(f"  paired (b) against (c): {int(diff.sum())} of {a.trials} trials differ in their verdict; sector X: (b) wrong and (c) right "
        f"{int(((b & 2) > (c & 2)).sum())}, (b) right and (c) wrong {int(((b & 2) < (c & 2)).sum())}; sector Z differs in {int(((b ^ c) & 1).sum())}")


say("correlated two-sector decoding -- tools/kbench_correlated.py")
say(f"alpha {a.alpha}, batch {a.batch}, {a.trials} trials per plan, seed {a.seed}, max_iter 50, one run per plan (no repeats: read the times to two digits)")
c = load_code("bb144")
bb = dict(ell=c["ell"], m=c["m_dim"], a_x_powers=c["a_x_powers"], a_y_powers=c["a_y_powers"], b_y_powers=c["b_y_powers"], b_x_powers=c["b_x_powers"])
for p in [float(x) for x in a.rates.split(",") if x]:
    say(f"\n== circ144 circuit plan at p = {p}")
    pre = load_precomputed_matrices("circ144") if abs(p - 0.005) < 1e-12 else None
    if pre is None:
        t0 = time.perf_counter()
        pre = build_decoding_matrices(BBCodeCircuit(c["Hx"], c["Hz"], num_cycles=12, **bb), c["Lx"], c["Lz"], p, verbose=False)
        say(f"  (decoding matrices built in {time.perf_counter() - t0:.1f} s)")
    prob = engine._circuit_problem(c["Hx"], c["Hz"], c["Lx"], c["Lz"], p, 12, pre, 0, bb)
    t0 = time.perf_counter()
    sigs = (_lib.circuit_fault_signatures(prob.compiled, c["Lx"], c["Lz"], False), _lib.circuit_fault_signatures(prob.compiled, c["Lx"], c["Lz"], True))
    links = {m: correlated.links_from_circuit(prob.compiled, c["Lx"], c["Lz"], pre, p, mode=m, signatures=sigs) for m in correlated.MODES}
    lk = links["raise"]
    gz, gx = prob.graphs
    say(f"  Z {gz.m} x {gz.n}, X {gx.m} x {gx.n}; {lk.n_links} links on {int((np.diff(lk.ptr) > 0).sum())} X columns (longest run {int(np.diff(lk.ptr).max())}), "
        f"{lk.unmatched} unmatched projections; link llr {lk.llr.min():.2f} .. {lk.llr.max():.2f}, median {np.median(lk.llr):.2f}; built in {time.perf_counter() - t0:.1f} s")
    say(f"  condition: base - prior of X: median {np.median(links['condition'].base - prob.llrs[1]):.3f}, max {np.max(links['condition'].base - prob.llrs[1]):.3f}")
    measure(lambda: prob.make_plan(prob.graphs, 50, 1.0, 1.0, "dynamical", a.batch, 0), links)
if not a.no_dem:
    say("\n== the two-sector detector error model of from_decoding_matrices('circ144') (independent columns: the control)")
    dem = DetectorErrorModel.from_decoding_matrices("circ144")
    links = {m: correlated.links_from_dem(dem, mode=m) for m in correlated.MODES}
    say(f"  {dem.n_mech} mechanisms; {links['raise'].n_links} links (empty by construction), {links['raise'].unmatched} unmatched projections")
    views = [dem.decoder_view(s) for s in range(2)]
    graphs = [_lib.Graph(v.indptr, v.indices, v.shape[1]) for v in views]
    measure(lambda: dem.plan(graphs, max_iter=50, batch=a.batch), links)
_log.close()
