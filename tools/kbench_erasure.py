#!/usr/bin/env python3
"""Heralded-erasure noise on one GPU: what knowing the erasures buys, and what sampling them and building the per-shot priors costs.

  python tools/kbench_erasure.py [--p 0.003] [--rates 0.005,0.01,0.02] [--trials N] [--batch B] [--repeats R] [--out FILE]

Problem: the circ144 circuit plan ([[144,12,12]] x 12 cycles, decoding matrices built by the GPU builder at --p), BP + OSD-0, one seed.  Erasure rates
are on the CNOT class.  Plans, all on the same seed and trial range:
  flood        the default plan, no erasure noise: never switched, so it enqueues what the parent commit enqueues (its sample phase is the Bernoulli sampler)
  nolinks      use_correlated(alpha, links=None), no erasure noise: the per-shot-prior kernel at stride 0, the baseline of the aware plan's BP bracket
  aware@0      use_erasure_aware + use_erasure_noise(0.0): the same trials, syndromes and prior values as nolinks, but through the erasure sampler, the
               prior kernels and prior[batch][n] at stride n -- against nolinks, what materialising and re-reading the per-shot priors costs
  unaware@r    the default plan with use_erasure_noise({"CNOT": r}): the erasure sampler, a decoder that does not read the heralds
  aware@r      use_erasure_aware + the same noise: the erasure sampler, the two prior kernels, the per-shot-prior kernel at stride n
Printed per plan and repeat: trials/s of run() (host clock around run + read, which waits for the device), the six hipEvent phase brackets in ms per
batch, BP converged per sector and the logical errors with binomial standard errors.  Then per rate: the paired verdicts of unaware against aware, the
sample phase of aware minus unaware (= the two prior kernels: the samplers are the same launch) as a share of the sample phase and as bytes written
per second (8 (n_z + n_x) batch bytes per batch).  The repeats alternate over all plans so that drift shows as spread.
Everything printed is also written to --out (default profiles/r26_erasure.txt)."""
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
from qldpc_amd.simulation import engine  # noqa: E402
from qldpc_amd.simulation.erasure import H_INF, erasure_tables_from_circuit  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--p", type=float, default=0.003)
ap.add_argument("--rates", default="0.005,0.01,0.02")
ap.add_argument("--trials", type=int, default=65536)
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--alpha", type=float, default=1.0)
ap.add_argument("--repeats", type=int, default=2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_erasure.txt"))
ap.add_argument("--seed", type=int, default=20261020)
a = ap.parse_args()
_lib.require_device()
T = _lib.TALLY
_log = open(a.out, "w")


def say(msg=""):
    print(msg, flush=True)
    _log.write(msg + "\n")
    _log.flush()


def rate(k, n):
    p = k / max(n, 1)
    return f"{p:.4g} +- {np.sqrt(p * (1 - p) / max(n, 1)):.2g} ({int(k)})"


say("heralded-erasure noise and erasure-aware decoding -- tools/kbench_erasure.py")
say(f"circ144 at p = {a.p}, alpha {a.alpha}, batch {a.batch}, {a.trials} trials per plan and repeat, seed {a.seed}, max_iter 50, BP + OSD-0, {a.repeats} repeats")
c = load_code("bb144")
bb = dict(ell=c["ell"], m=c["m_dim"], a_x_powers=c["a_x_powers"], a_y_powers=c["a_y_powers"], b_y_powers=c["b_y_powers"], b_x_powers=c["b_x_powers"])
pre = load_precomputed_matrices("circ144") if abs(a.p - 0.005) < 1e-12 else None
if pre is None:
    t0 = time.perf_counter()
    pre = build_decoding_matrices(BBCodeCircuit(c["Hx"], c["Hz"], num_cycles=12, **bb), c["Lx"], c["Lz"], a.p, verbose=False)
    say(f"  (decoding matrices built in {time.perf_counter() - t0:.1f} s)")
prob = engine._circuit_problem(c["Hx"], c["Hz"], c["Lx"], c["Lz"], a.p, 12, pre, 0, bb)
t0 = time.perf_counter()
tables = erasure_tables_from_circuit(prob.compiled, c["Lx"], c["Lz"], pre)
gz, gx = prob.graphs
n_locs = int(np.asarray(prob.compiled.base_ops).size)
say(f"  Z {gz.m} x {gz.n}, X {gx.m} x {gx.n}; {n_locs} locations; tables built in {time.perf_counter() - t0:.1f} s")
for name, t in zip("ZX", tables):
    say(f"  tables {name}: {t.loc_col.size} contributions ({int((t.loc_h == H_INF).sum())} INF, {int((t.loc_h == 1).sum())} h = 1), longest location run "
        f"{int(np.diff(t.loc_ptr).max())}, largest c_j {int(np.diff(t.lut_ptr).max()) - 1}, lut {t.lut.size} entries, {t.unmatched} unmatched projections")
rates = [float(x) for x in a.rates.split(",") if x]
plans = [("flood", None, None), ("nolinks", None, None), ("aware@0", "aware", 0.0)] + [(f"{kind}@{r:g}", kind, r) for r in rates for kind in ("unaware", "aware")]
sample_ms, verdicts = {}, {}
for rep in range(a.repeats):
    say(f"\n== repeat {rep + 1}")
    for name, kind, r in plans:
        plan = prob.make_plan(prob.graphs, 50, 1.0, 1.0, "dynamical", a.batch, 0)
        if name == "nolinks":
            plan.use_correlated(a.alpha, None)
        if kind == "aware":
            plan.use_erasure_aware(a.alpha, tables)
        if r is not None:
            plan.use_erasure_noise({"CNOT": r})
        plan.run(a.seed + 1, 0, a.batch); plan.read(clear=True); plan.phase_times()       # warm-up: one full batch, the shape of the timed ones
        t0 = time.perf_counter()
        plan.run(a.seed, 0, a.trials)
        t = plan.read(clear=True)
        dt = time.perf_counter() - t0
        ph, nb = plan.phase_times()
        n = int(t[T["trials"]])
        sample_ms.setdefault(name, []).append(ph["sample"] / max(nb, 1))
        say(f"[{name:13s}] {a.trials / dt:9.4g} trials/s;  ms per batch: " + "  ".join(f"{k} {v / max(nb, 1):.2f}" for k, v in ph.items()))
        say(f"                BP converged Z {t[T['bp_conv_z']] / n:.4f} X {t[T['bp_conv_x']] / n:.4f};  logical errors Z {rate(t[T['z_err']], n)}  "
            f"X {rate(t[T['x_err']], n)}  total {rate(t[T['total_err']], n)}")
        if rep == 0 and kind is not None and r > 0:
            verdicts[name] = plan.run_outcomes(a.seed, 0, a.trials)
            plan.read(clear=True)
        plan.close()
say("\n== per rate (sample phase: mean over the repeats, ms per batch)")
say(f"  Bernoulli sampler (flood): {np.mean(sample_ms['flood']):.3f}; nolinks: {np.mean(sample_ms['nolinks']):.3f}; aware@0 (erasure sampler at rate 0 + the two prior "
    f"kernels): {np.mean(sample_ms['aware@0']):.3f}")
for r in rates:
    u, w = verdicts[f"unaware@{r:g}"], verdicts[f"aware@{r:g}"]
    su, sa = np.mean(sample_ms[f"unaware@{r:g}"]), np.mean(sample_ms[f"aware@{r:g}"])
    pri = sa - su
    gbs = 8.0 * (gz.n + gx.n) * a.batch / (pri * 1e-3) / 1e9 if pri > 0 else float("nan")
    say(f"  CNOT erasure rate {r:g}: unaware fails {int(np.count_nonzero(u))}, aware {int(np.count_nonzero(w))} of {a.trials}; unaware wrong and aware right "
        f"{int(((u != 0) & (w == 0)).sum())}, unaware right and aware wrong {int(((u == 0) & (w != 0)).sum())}")
    say(f"      sample phase: erasure sampler {su:.3f}, with the two prior kernels {sa:.3f}: the prior kernels take {pri:.3f} ms = {100 * pri / sa:.0f} % of it, "
        f"{gbs:.0f} GB/s of prior rows written")
_log.close()
