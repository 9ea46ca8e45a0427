#!/usr/bin/env python3
"""The fixed-weight sampler beside the Bernoulli sampler, and one stratified LER(p) sweep beside a direct run, on a shipped circuit:
    python tools/kbench_strata.py [--tag circ144] [--batch 16384] [--out profiles/r19_strata.txt]
The plans are created directly, so the sampler's p and the priors are independent.  The decoding matrices are the shipped ones (built at p = 0.005); the
probability of every column is a sum of terms proportional to p (noise/builder.py), so the priors at another p are prior_llrs(channel_probs * p / 0.005).
  1. the `sample` bracket (ms per batch) of the Bernoulli sampler at p = 0.005 and of the fixed-weight sampler at w = 17, 86, 400 on ONE plan, alternating
     --rounds times in one session; the ratio against the Bernoulli bracket of the same round and the spread.  No bar: the plan is decoder-bound.
  2. one sweep with priors at --prior-p over p_range (--p-lo, --prior-p): LER(p) with std_error, lower and upper at a few p, total trials, wall time.
  3. a direct Bernoulli run on the same plan at --prior-p, with its binomial standard error, beside the stratified estimate there.
Not measured here: hardware counters, a kernel trace, circ288."""
import argparse
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qldpc_amd  # noqa: F401,E402
from qldpc_amd import _lib  # noqa: E402
from qldpc_amd.data import load_code, load_circuit_matrices  # noqa: E402
from qldpc_amd.codes.bb_code import BBCodeCircuit  # noqa: E402
from qldpc_amd.noise.compiled import CompiledCircuit  # noqa: E402
from qldpc_amd.simulation import strata  # noqa: E402
from qldpc_amd.simulation.engine import prior_llrs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tag", default="circ144")
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--max-iter", type=int, default=50)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--bracket-batches", type=int, default=4)
ap.add_argument("--weights", default="17,86,400")
ap.add_argument("--prior-p", type=float, default=0.003)
ap.add_argument("--p-lo", type=float, default=0.001)
ap.add_argument("--report-p", default="0.001,0.0015,0.002,0.003")
ap.add_argument("--target-failures", type=int, default=100)
ap.add_argument("--max-trials-per-weight", type=int, default=262144)
ap.add_argument("--direct-trials", type=int, default=262144)
ap.add_argument("--out", default="", help="append the report to this file as well")
a = ap.parse_args()
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


say(f"== tools/kbench_strata.py --tag {a.tag} --batch {a.batch} --max-iter {a.max_iter} --prior-p {a.prior_p} --p-lo {a.p_lo}; library {os.path.basename(_lib.SO_PATH)}")
d = load_circuit_matrices(a.tag)
c = load_code(str(d["code"]))
cb = BBCodeCircuit(c["Hx"], c["Hz"], num_cycles=int(d["num_cycles"]), ell=c["ell"], m=c["m_dim"], a_x_powers=c["a_x_powers"],
                   a_y_powers=c["a_y_powers"], b_y_powers=c["b_y_powers"], b_x_powers=c["b_x_powers"])
comp = CompiledCircuit(cb.get_full_circuit(), cb.cycle * 2, cb.lin_order, cb.data_qubits, cb.Xchecks, cb.Zchecks)
gr, mk = [], []
for s in "ZX":
    n = int(d[f"Hdec{s}_shape"][1])
    gr.append(_lib.Graph(d[f"Hdec{s}_indptr"], d[f"Hdec{s}_indices"], n))
    mk.append(_lib.logical_column_masks((d[f"H{s}_logical_indptr"], d[f"H{s}_logical_indices"]), n))


def make_plan(sampler_p, prior_p):
    pr = [prior_llrs(np.asarray(d[f"channel_probs{s}"], np.float64) * (prior_p / 0.005)) for s in "ZX"]
    return _lib.CircuitPlan(comp, c["Lx"], c["Lz"], gr[0], gr[1], pr[0], pr[1], mk[0], mk[1], sampler_p, max_iter=a.max_iter, batch=a.batch)


# ---- 1. the sample bracket ---------------------------------------------------------------------------------------------------------------------------
plan = make_plan(0.005, 0.005)
N = plan.n_locs
say(f"{a.tag}: N = {N} fault locations; N p = {N * 0.005:.1f} at p = 0.005")
weights = [int(x) for x in a.weights.split(",")]
configs = [("bernoulli p=0.005", None)] + [(f"fixed w={w}", w) for w in weights]
count = a.batch * a.bracket_batches
for name, w in configs:                                                  # warm-up: allocations, first launches of both samplers
    plan.use_fixed_weight(w)
    plan.run(1, 0, min(a.batch, 256))
plan.read(clear=True)
plan.phase_times()
ms = {name: [] for name, _ in configs}
for rnd in range(a.rounds):
    for name, w in configs:
        plan.use_fixed_weight(w)
        plan.run(5, rnd * count, count)
        plan.read(clear=True)
        ph, nb = plan.phase_times()
        ms[name].append(ph["sample"] / max(nb, 1))
        say(f"round {rnd} {name:18s}: sample {ph['sample'] / nb:.3f} ms/batch of {a.batch}; whole batch {sum(ph.values()) / nb:.2f} ms "
            f"(bp_z {ph['bp_z'] / nb:.2f}, osd_z {ph['osd_z'] / nb:.2f}, bp_x {ph['bp_x'] / nb:.2f}, osd_x {ph['osd_x'] / nb:.2f})")
base = ms[configs[0][0]]
for name, w in configs:
    ratios = [x / b for x, b in zip(ms[name], base)]
    say(f"{name:18s}: sample ms/batch median {np.median(ms[name]):.3f} (min {min(ms[name]):.3f}, max {max(ms[name]):.3f}); ratio to the Bernoulli bracket of the "
        f"same round: median {np.median(ratios):.2f} (min {min(ratios):.2f}, max {max(ratios):.2f})")
plan.close()

# ---- 2. one sweep ------------------------------------------------------------------------------------------------------------------------------------
t0 = time.perf_counter()
plan = make_plan(a.prior_p, a.prior_p)
stream = _lib.Stream(0)
t_plan = time.perf_counter() - t0
t0 = time.perf_counter()
lo, hi = strata.weights_for(N, (a.p_lo, a.prior_p), 1e-9)
t_pick = time.perf_counter() - t0
ws_list = np.arange(lo, hi + 1)
say(f"sweep: priors at p = {a.prior_p}, p_range ({a.p_lo}, {a.prior_p}), coverage 1e-9 -> weights {lo}..{hi} ({ws_list.size} strata); per weight "
    f"batches of {a.batch} until {a.target_failures} failures or {a.max_trials_per_weight} trials")
t0 = time.perf_counter()
ws = strata._sweep(plan, stream, N, ws_list, a.max_trials_per_weight, a.target_failures, a.batch, 20260401)
dt = time.perf_counter() - t0
say(f"sweep: {int(ws.trials.sum())} trials, {int(ws.failures.sum())} failures, {dt:.1f} s wall ({ws.trials.sum() / dt:.0f} trials/s): the {ws_list.size} strata on "
    f"the plan as it stands; before it, creating the plan took {t_plan:.2f} s and picking the weights (weights_for, on the host) {t_pick * 1e3:.2f} ms")
say("  w: trials failures  " + "  ".join(f"{int(w)}: {int(n)} {int(k)}" for w, n, k in zip(ws.weights, ws.trials, ws.failures)))
ps = [float(x) for x in a.report_p.split(",")]
r = ws.logical_error_rate(np.array(ps))
for i, p in enumerate(ps):
    say(f"  LER({p:g}) = {r['estimate'][i]:.4e} +- {r['std_error'][i]:.2e} (z {r['estimate_z'][i]:.3e}, x {r['estimate_x'][i]:.3e}); lower {r['lower'][i]:.4e}, "
        f"upper {r['upper'][i]:.4e}; uncovered mass {1.0 - r['covered'][i]:.2e}")

# ---- 3. a direct run on the same plan ----------------------------------------------------------------------------------------------------------------
T = _lib.TALLY
t0 = time.perf_counter()
plan.run(20260402, 0, a.direct_trials, stream.ptr)
t = plan.read(stream.ptr, clear=True)
dt = time.perf_counter() - t0
direct = t[T["total_err"]] / t[T["trials"]]
se = math.sqrt(direct * (1 - direct) / t[T["trials"]])
at = ws.logical_error_rate(a.prior_p)
say(f"direct Bernoulli run at p = {a.prior_p} on the same plan: {int(t[T['trials']])} trials, {int(t[T['total_err']])} failures, {dt:.1f} s: LER {direct:.4e} +- {se:.2e}; "
    f"stratified there {float(at['estimate']):.4e} +- {float(at['std_error']):.2e}; difference {(float(at['estimate']) - direct) / math.hypot(se, float(at['std_error'])):+.2f} sigma")
plan.close()
stream.close()
say("not measured: hardware counters, a kernel trace, circ288")
if a.out:
    with open(a.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
