#!/usr/bin/env python3
"""Per-class, biased Pauli noise on one GPU: what a noise model does to the logical error rate, with priors that match it and with priors that do not.

  python tools/kbench_noise_model.py [--p 0.003] [--eta 10] [--trials N] [--batch B] [--out FILE]

Problem: the circ144 circuit plan ([[144,12,12]] x 12 cycles, decoding matrices built by the GPU builder at --p), BP + OSD-0, one seed.  Rows, all on
the same seed and trial range:
  (a) plain            the default plan: never switched, so it enqueues what the parent commit enqueues (its sample phase is circuit_sample_kernel)
  (b) uniform(p)       use_noise_model(NoiseModel.uniform(p)): the new sampler kernel drawing today's law -- must equal (a) trial for trial (asserted)
  (c) si1000 matched   use_noise_model(NoiseModel.si1000(p)) on a plan created with the model's own priors (NoiseModel.prior_llrs)
  (d) si1000 uniform   the same noise on the plan of (a): priors of the uniform model at p, the mismatched decoder
  (e) biased matched   NoiseModel.biased(p, eta) with its own priors
  (f) biased uniform   the same noise with the uniform priors
Printed per row: trials/s of run_outcomes() (host clock around run + read, which waits for the device, and copies a verdict byte per trial back), the
sample bracket and the other hipEvent phase brackets in ms per batch, BP converged per sector and the logical errors per sector and in total with
binomial standard errors.  Then (c) against (d) and (e) against (f): the trials whose verdict differs and which way they turned.
Everything printed is also written to --out (default profiles/r28_noise_model.txt)."""
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
from qldpc_amd.simulation.noise_model import NoiseModel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--p", type=float, default=0.003)
ap.add_argument("--eta", type=float, default=10.0)
ap.add_argument("--trials", type=int, default=65536)
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r28_noise_model.txt"))
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


say("per-class, biased Pauli noise models -- tools/kbench_noise_model.py")
say(f"circ144 at p = {a.p}, eta {a.eta:g}, batch {a.batch}, {a.trials} trials per row, ONE seed ({a.seed}), max_iter 50, BP + OSD-0")
c = load_code("bb144")
bb = dict(ell=c["ell"], m=c["m_dim"], a_x_powers=c["a_x_powers"], a_y_powers=c["a_y_powers"], b_y_powers=c["b_y_powers"], b_x_powers=c["b_x_powers"])
pre = load_precomputed_matrices("circ144") if abs(a.p - 0.005) < 1e-12 else None
if pre is None:
    t0 = time.perf_counter()
    pre = build_decoding_matrices(BBCodeCircuit(c["Hx"], c["Hz"], num_cycles=12, **bb), c["Lx"], c["Lz"], a.p, verbose=False)
    say(f"  (decoding matrices built in {time.perf_counter() - t0:.1f} s)")
prob = engine._circuit_problem(c["Hx"], c["Hz"], c["Lx"], c["Lz"], a.p, 12, pre, 0, bb)
gz, gx = prob.graphs
n_locs = int(np.asarray(prob.compiled.base_ops).size)
say(f"  Z {gz.m} x {gz.n}, X {gx.m} x {gx.n}; {n_locs} locations by op code 1..6: {np.bincount(np.asarray(prob.compiled.base_ops), minlength=7)[1:].tolist()}")
sigs = (_lib.circuit_fault_signatures(prob.compiled, c["Lx"], c["Lz"], False), _lib.circuit_fault_signatures(prob.compiled, c["Lx"], c["Lz"], True))
models = {"uniform": NoiseModel.uniform(a.p), "si1000": NoiseModel.si1000(a.p), "biased": NoiseModel.biased(a.p, a.eta)}
priors = {}
for name, m in models.items():
    t0 = time.perf_counter()
    pz, px, unmatched = m._channel_probs(prob.compiled, c["Lx"], c["Lz"], pre, signatures=sigs)
    priors[name] = m.prior_llrs(prob.compiled, c["Lx"], c["Lz"], pre, signatures=sigs)
    say(f"  {name:8s} {m!r}")
    say(f"           matched priors in {time.perf_counter() - t0:.1f} s: total mass Z {pz.sum():.4f} X {px.sum():.4f} (uniform matrices: "
        f"{np.sum(pre['channel_probsZ']):.4f} / {np.sum(pre['channel_probsX']):.4f}); zero-mass columns {int((pz == 0).sum())} / {int((px == 0).sum())}; unmatched {unmatched}")
assert np.array_equal(priors["uniform"][0], prob.llrs[0]) and np.array_equal(priors["uniform"][1], prob.llrs[1]), "uniform(p) does not reproduce the builder's priors"
say("  uniform(p) reproduces the builder's channel probabilities and priors bit for bit")

rows = [("(a) plain", None, None), ("(b) uniform(p)", "uniform", None), ("(c) si1000 matched", "si1000", "si1000"), ("(d) si1000 uniform", "si1000", None),
        ("(e) biased matched", "biased", "biased"), ("(f) biased uniform", "biased", None)]
verdicts = {}
say()
for name, model, prior in rows:
    plan = prob.make_plan(prob.graphs, 50, 1.0, 1.0, "dynamical", a.batch, 0, llrs=None if prior is None else priors[prior])
    if model is not None:
        plan.use_noise_model(models[model])
    plan.run(a.seed + 1, 0, a.batch); plan.read(clear=True); plan.phase_times()       # warm-up: one full batch, the shape of the timed ones
    t0 = time.perf_counter()
    verdicts[name[:3]] = plan.run_outcomes(a.seed, 0, a.trials)
    t = plan.read(clear=True)
    dt = time.perf_counter() - t0
    ph, nb = plan.phase_times()
    n = int(t[T["trials"]])
    say(f"[{name:18s}] {a.trials / dt:9.4g} trials/s;  sample {ph['sample'] / max(nb, 1):.3f} ms per batch;  " +
        "  ".join(f"{k} {v / max(nb, 1):.2f}" for k, v in ph.items() if k != "sample"))
    say(f"                     BP converged Z {t[T['bp_conv_z']] / n:.4f} X {t[T['bp_conv_x']] / n:.4f};  logical errors Z {rate(t[T['z_err']], n)}  "
        f"X {rate(t[T['x_err']], n)}  total {rate(t[T['total_err']], n)}")
    plan.close()
assert np.array_equal(verdicts["(a)"], verdicts["(b)"]), "uniform(p) on the new sampler differs from the plain plan"
say("\n(b) equals (a) trial for trial")
say("\n== matched against uniform priors on the same trials (one seed: a difference below its standard error says nothing)")
for m, u, what in (("(c)", "(d)", "si1000"), ("(e)", "(f)", f"biased eta {a.eta:g}")):
    vm, vu = verdicts[m], verdicts[u]
    say(f"  {what}: matched fails {int(np.count_nonzero(vm))}, uniform priors fail {int(np.count_nonzero(vu))} of {a.trials}; verdict differs in "
        f"{int(np.count_nonzero((vm != 0) != (vu != 0)))} trials: matching the priors turned {int(((vu != 0) & (vm == 0)).sum())} right and "
        f"{int(((vu == 0) & (vm != 0)).sum())} wrong")
_log.close()
