#!/usr/bin/env python3
"""Soft-readout noise on one GPU: what reading the confidence levels buys, and what sampling them and building the per-shot priors costs.

  python tools/kbench_soft.py [--p 0.003] [--sigmas 0.3,0.4,0.5] [--levels 8] [--trials N] [--batch B] [--repeats R] [--out FILE] [--no-resources]

Problem: the circ144 circuit plan ([[144,12,12]] x 12 cycles, decoding matrices built by the GPU builder at --p), BP + OSD-0, one seed.  The readout is
SoftReadout.gaussian(sigma, levels).  Plans, all on the same seed and trial range:
  flood          the default plan, hard measurements: never switched, so it enqueues what the parent commit enqueues
  nolinks        use_correlated(alpha, links=None), hard measurements: the per-shot-prior kernel at stride 0, the baseline of the aware plan's BP bracket
  plain@s        nolinks with use_soft_readout(sigma s): the soft sampler, the plain priors -- a decoder that does not know the readout is noisy
  marginal@s     the same with marginal_priors: the matched prior of a decoder that does not read the levels
  aware@s        use_soft_aware on the marginal plan: the soft sampler, the two prior kernels, the per-shot-prior kernel at stride n
Printed per plan and repeat: trials/s of run() (host clock around run + read, which waits for the device), the six hipEvent phase brackets in ms per
batch, BP converged per sector and the logical errors with binomial standard errors.  Then per sigma: the paired verdicts of marginal against aware,
and the sample phase of aware minus marginal (= the two prior kernels: the samplers are the same launch) as a share of the sample phase and as bytes
written per second (8 (n_z + n_x) batch bytes per batch).  The repeats alternate over all plans so that drift shows as spread.  Last, unless
--no-resources: the register, LDS and occupancy figures of the two kernels of csrc/soft.hip (hipcc -Rpass-analysis=kernel-resource-usage).
Everything printed is also written to --out (default profiles/r29_soft.txt)."""
import argparse
import os
import re
import subprocess
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
from qldpc_amd.simulation.soft import SoftReadout, marginal_priors, soft_tables_from_circuit  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--p", type=float, default=0.003)
ap.add_argument("--sigmas", default="0.3,0.4,0.5")
ap.add_argument("--levels", type=int, default=8)
ap.add_argument("--trials", type=int, default=65536)
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--alpha", type=float, default=1.0)
ap.add_argument("--repeats", type=int, default=2)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r29_soft.txt"))
ap.add_argument("--seed", type=int, default=20261021)
ap.add_argument("--no-resources", action="store_true")
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


say("soft-readout noise and soft-aware decoding -- tools/kbench_soft.py")
say(f"circ144 at p = {a.p}, alpha {a.alpha}, batch {a.batch}, {a.trials} trials per plan and repeat, seed {a.seed}, max_iter 50, BP + OSD-0, {a.repeats} repeats, "
    f"{a.levels} levels")
c = load_code("bb144")
bb = dict(ell=c["ell"], m=c["m_dim"], a_x_powers=c["a_x_powers"], a_y_powers=c["a_y_powers"], b_y_powers=c["b_y_powers"], b_x_powers=c["b_x_powers"])
pre = load_precomputed_matrices("circ144") if abs(a.p - 0.005) < 1e-12 else None
if pre is None:
    t0 = time.perf_counter()
    pre = build_decoding_matrices(BBCodeCircuit(c["Hx"], c["Hz"], num_cycles=12, **bb), c["Lx"], c["Lz"], a.p, verbose=False)
    say(f"  (decoding matrices built in {time.perf_counter() - t0:.1f} s)")
prob = engine._circuit_problem(c["Hx"], c["Hz"], c["Lx"], c["Lz"], a.p, 12, pre, 0, bb)
gz, gx = prob.graphs
sigs = (_lib.circuit_fault_signatures(prob.compiled, c["Lx"], c["Lz"], False), _lib.circuit_fault_signatures(prob.compiled, c["Lx"], c["Lz"], True))
sigmas = [float(x) for x in a.sigmas.split(",") if x]
readouts, tables, marg = {}, {}, {}
t0 = time.perf_counter()
for s in sigmas:
    readouts[s] = SoftReadout.gaussian(s, a.levels)
    tables[s] = soft_tables_from_circuit(prob.compiled, c["Lx"], c["Lz"], pre, readouts[s], signatures=sigs)
    marg[s] = marginal_priors(pre, tables[s], readouts[s])
say(f"  Z {gz.m} x {gz.n}, X {gx.m} x {gx.n}; {int(np.asarray(prob.compiled.base_ops).size)} locations, {tables[sigmas[0]][0].n_meas} measurements; "
    f"tables of {len(sigmas)} channels built in {time.perf_counter() - t0:.1f} s")
for name, t in zip("ZX", tables[sigmas[0]]):
    cnt = np.bincount(t.meas_col[t.meas_col >= 0], minlength=t.n)
    say(f"  tables {name}: {int((t.meas_col >= 0).sum())} measurements on {int((cnt > 0).sum())} columns, at most {int(cnt.max())} per column, lut {t.lut.size} "
        f"entries, {t.unmatched} unmatched projections")
for s in sigmas:
    say(f"  sigma {s:g}: qbar = {readouts[s].qbar:.5g}, q per level = " + " ".join(f"{q:.3g}" for q in readouts[s].q))
plans = [("flood", None, None), ("nolinks", None, None)] + [(f"{kind}@{s:g}", kind, s) for s in sigmas for kind in ("plain", "marginal", "aware")]
sample_ms, verdicts, ler = {}, {}, {}
for rep in range(a.repeats):
    say(f"\n== repeat {rep + 1}")
    for name, kind, s in plans:
        plan = prob.make_plan(prob.graphs, 50, 1.0, 1.0, "dynamical", a.batch, 0, llrs=marg[s] if kind in ("marginal", "aware") else None)
        if kind == "aware":
            plan.use_soft_aware(a.alpha, tables[s])
        elif name != "flood":
            plan.use_correlated(a.alpha, None)
        if s is not None:
            plan.use_soft_readout(readouts[s])
        plan.run(a.seed + 1, 0, a.batch); plan.read(clear=True); plan.phase_times()       # warm-up: one full batch, the shape of the timed ones
        t0 = time.perf_counter()
        plan.run(a.seed, 0, a.trials)
        t = plan.read(clear=True)
        dt = time.perf_counter() - t0
        ph, nb = plan.phase_times()
        n = int(t[T["trials"]])
        sample_ms.setdefault(name, []).append(ph["sample"] / max(nb, 1))
        ler[name] = (int(t[T["total_err"]]), n)
        say(f"[{name:13s}] {a.trials / dt:9.4g} trials/s;  ms per batch: " + "  ".join(f"{k} {v / max(nb, 1):.2f}" for k, v in ph.items()))
        say(f"                BP converged Z {t[T['bp_conv_z']] / n:.4f} X {t[T['bp_conv_x']] / n:.4f};  logical errors Z {rate(t[T['z_err']], n)}  "
            f"X {rate(t[T['x_err']], n)}  total {rate(t[T['total_err']], n)}")
        if rep == 0 and kind in ("marginal", "aware"):
            verdicts[name] = plan.run_outcomes(a.seed, 0, a.trials)
            plan.read(clear=True)
        plan.close()
say("\n== per sigma (sample phase: mean over the repeats, ms per batch)")
say(f"  hard measurements: Bernoulli sampler (flood) {np.mean(sample_ms['flood']):.3f}, nolinks {np.mean(sample_ms['nolinks']):.3f};  LER flood "
    f"{rate(*ler['flood'])}, nolinks {rate(*ler['nolinks'])}")
for s in sigmas:
    u, w = verdicts[f"marginal@{s:g}"], verdicts[f"aware@{s:g}"]
    su, sa = np.mean(sample_ms[f"marginal@{s:g}"]), np.mean(sample_ms[f"aware@{s:g}"])
    pri = sa - su
    gbs = 8.0 * (gz.n + gx.n) * a.batch / (pri * 1e-3) / 1e9 if pri > 0 else float("nan")
    say(f"  sigma {s:g}: LER plain {rate(*ler[f'plain@{s:g}'])}, marginal {rate(*ler[f'marginal@{s:g}'])}, aware {rate(*ler[f'aware@{s:g}'])}")
    say(f"      paired: marginal fails {int(np.count_nonzero(u))}, aware {int(np.count_nonzero(w))} of {a.trials}; marginal wrong and aware right "
        f"{int(((u != 0) & (w == 0)).sum())}, marginal right and aware wrong {int(((u == 0) & (w != 0)).sum())}")
    say(f"      sample phase: soft sampler {su:.3f}, with the two prior kernels {sa:.3f}: the prior kernels take {pri:.3f} ms = {100 * pri / sa:.0f} % of it, "
        f"{gbs:.0f} GB/s of prior rows written")
if not a.no_resources:
    say("\n== kernel resource usage (hipcc -Rpass-analysis=kernel-resource-usage, csrc/soft.hip, gfx950)")
    csrc = os.path.join(ROOT, "qldpc-branched-off_amd", "csrc")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
           "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "soft.hip"), "-o", os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True).stderr
    keep = False
    for line in text.splitlines():
        m = re.search(r"remark: (.*)\[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        if "Function Name" in m.group(1):
            keep = "soft_sample_kernel" in m.group(1) or "soft_prior_kernel" in m.group(1)
        if keep:
            say("  " + m.group(1).strip())
_log.close()
