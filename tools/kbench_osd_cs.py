#!/usr/bin/env python3
"""BP + OSD-CS against BP + OSD-0 and Relay-BP on one GPU (config-5 shape: [[144,12,12]] x 12 cycles, bundled circ144 matrices).

  python tools/kbench_osd_cs.py [--trials N] [--batch B] [--sim-trials N] [--rates 0.003,0.004,0.005] [--orders 0,7,20] [--out FILE]

Part 0: the OSD-CS kernel's resources (hipcc -Rpass-analysis=kernel-resource-usage, when hipcc is on this machine).  Part 1: one circuit
plan per OSD stage (OSD-0, OSD-CS of each order) on the same trials and seed, both sectors on one stream (exclusive hipEvent spans): ms of
the OSD phase per sector batch and trials/s of the whole plan.  Part 2: run_simulation with BP + OSD-0, BP + OSD-CS (order 7) and Relay-BP
at each error rate (the builder makes the matrices of rates that are not bundled): logical error rate with its binomial standard error.
Everything printed is also written to --out (default profiles/r06_osd_cs.txt).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import qldpc_amd  # noqa: F401,E402
from qldpc_amd import _lib  # noqa: E402
from qldpc_amd.data import load_code, load_circuit_matrices, load_precomputed_matrices  # noqa: E402
from qldpc_amd.codes.bb_code import BBCodeCircuit  # noqa: E402
from qldpc_amd.noise.compiled import CompiledCircuit  # noqa: E402
from qldpc_amd.simulation.engine import prior_llrs, run_simulation  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tag", default="circ144")
ap.add_argument("--trials", type=int, default=32768)
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--sim-trials", type=int, default=16384)
ap.add_argument("--rates", default="0.003,0.004,0.005")
ap.add_argument("--orders", default="0,7,20")
ap.add_argument("--sim-order", type=int, default=7)
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r06_osd_cs.txt"))
ap.add_argument("--seed", type=int, default=20261016)
a = ap.parse_args()
params = _lib.relay_params({}, with_clip=False)
T = _lib.TALLY
_log = open(a.out, "w")


def say(msg=""):
    print(msg, flush=True)
    _log.write(msg + "\n")
    _log.flush()


say("OSD-CS (combination sweep after OSD-0) -- tools/kbench_osd_cs.py")
src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qldpc-branched-off_amd", "csrc", "osd_cs.hip")
hipcc = "/opt/rocm/bin/hipcc"
if os.path.exists(hipcc):
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as td:
        r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-c", src, "-o",
                            os.path.join(td, "o.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    lines = [ln.split("remark:")[1].replace("[-Rpass-analysis=kernel-resource-usage]", "").strip() for ln in r.stderr.splitlines() if "remark:" in ln]
    keep, on = [], False
    for ln in lines:
        if ln.startswith("Function Name:"):
            on = "osd_cs_kernel" in ln
        if on:
            keep.append(ln)
    say("kernel resources (osd_cs_kernel, 1024 threads): " + "; ".join(keep))
say(f"Relay-BP parameters: {params}")

d = load_circuit_matrices(a.tag)
c = load_code(str(d["code"]))
bb = dict(ell=c["ell"], m=c["m_dim"], a_x_powers=c["a_x_powers"], a_y_powers=c["a_y_powers"], b_y_powers=c["b_y_powers"], b_x_powers=c["b_x_powers"])
cb = BBCodeCircuit(c["Hx"], c["Hz"], num_cycles=int(d["num_cycles"]), **bb)
comp = CompiledCircuit(cb.get_full_circuit(), cb.cycle * 2, cb.lin_order, cb.data_qubits, cb.Xchecks, cb.Zchecks)
gr, pr, mk = [], [], []
for s in "ZX":
    n = int(d[f"Hdec{s}_shape"][1])
    gr.append(_lib.Graph(d[f"Hdec{s}_indptr"], d[f"Hdec{s}_indices"], n))
    pr.append(prior_llrs(d[f"channel_probs{s}"]))
    mk.append(_lib.logical_column_masks((d[f"H{s}_logical_indptr"], d[f"H{s}_logical_indices"]), n))
say(f"{a.tag}: Z {gr[0].m} x {gr[0].n}, X {gr[1].m} x {gr[1].n}, {int(d['num_cycles'])} cycles, batch {a.batch}, {a.trials} trials, seed {a.seed}")


orders = [int(x) for x in a.orders.split(",") if x != ""]
rows = {}
for name in ["bp_osd0"] + [f"osd_cs{o}" for o in orders]:
    plan = _lib.CircuitPlan(comp, c["Lx"], c["Lz"], gr[0], gr[1], pr[0], pr[1], mk[0], mk[1], 0.005, max_iter=50, use_osd=True,
                            flags=_lib.FLAG_MC_UNFUSED, batch=a.batch)
    if name != "bp_osd0":
        plan.use_osd_cs(int(name[6:]))
    plan.run(a.seed + 1, 0, min(a.batch, 1024)); plan.read(clear=True); plan.phase_times()   # warm-up (module load, workspaces)
    t0 = time.perf_counter()
    plan.run(a.seed, 0, a.trials)
    tally = plan.read(clear=True)
    dt = time.perf_counter() - t0
    ph, nb = plan.phase_times()
    plan.close()
    trials = int(tally[T["trials"]])
    rows[name] = dict(tally=tally, dt=dt, ph={k: v / max(nb, 1) for k, v in ph.items()})
    ler = tally[T["total_err"]] / trials
    say(f"\n[{name}] {trials} trials in {dt:.3f} s = {trials / dt:.4g} trials/s; logical errors {int(tally[T['total_err']])} "
        f"(LER {ler:.4g} +- {np.sqrt(ler * (1 - ler) / trials):.2g})")
    say("  ms per batch of " + str(a.batch) + ": " + ", ".join(f"{k} {v:.3f}" for k, v in rows[name]["ph"].items()))
    say(f"  OSD calls Z {int(tally[T['osd_z']])} X {int(tally[T['osd_x']])}; unsatisfied outputs Z {int(tally[T['unsat_z']])} X {int(tally[T['unsat_x']])}")
for o in orders:
    r = rows[f"osd_cs{o}"]
    say(f"order {o}: OSD phase per sector batch Z {r['ph']['osd_z']:.3f} ms  X {r['ph']['osd_x']:.3f} ms "
        f"(OSD-0: Z {rows['bp_osd0']['ph']['osd_z']:.3f}  X {rows['bp_osd0']['ph']['osd_x']:.3f});  whole plan {r['dt'] / rows['bp_osd0']['dt']:.2f}x BP + OSD-0")

say(f"\nrun_simulation, [[144,12,12]] x {int(d['num_cycles'])} cycles, {a.sim_trials} trials per point (LER +- binomial standard error), seed {a.seed}")
for p in (float(x) for x in a.rates.split(",")):
    pre = load_precomputed_matrices(a.tag) if abs(p - 0.005) < 1e-12 and a.tag == "circ144" else None
    if pre is None:
        from qldpc_amd.noise.builder import build_decoding_matrices
        t0 = time.perf_counter()
        pre = build_decoding_matrices(cb, c["Lx"], c["Lz"], p, verbose=False)
        say(f"  (p = {p}: decoding matrices built in {time.perf_counter() - t0:.1f} s)")
    for dec in ("bp_osd", "bp_osd_cs", "relay_bp"):
        kw = dict(decoder=dec, relay_params=dict(params)) if dec == "relay_bp" else (dict(decoder=dec, osd_order=a.sim_order) if dec == "bp_osd_cs" else {})
        t0 = time.perf_counter()
        r = run_simulation(c["Hx"], c["Hz"], c["Lx"], c["Lz"], p, num_trials=a.sim_trials, num_cycles=int(d["num_cycles"]), maxIter=50,
                           precomputed_matrices=pre, base_seed=a.seed, batch=a.batch, devices=[0], **bb, **kw)
        dt = time.perf_counter() - t0
        ler, nt = r["logical_error_rate"], r["num_trials"]
        label = f"{dec}({a.sim_order})" if dec == "bp_osd_cs" else dec
        say(f"  p={p:.3f} {label:13s}: LER {ler:.4g} +- {np.sqrt(ler * (1 - ler) / nt):.2g}  ({int(r['tally'][T['total_err']])} / {nt});  "
            f"{nt / dt:.4g} trials/s (wall, incl. plan set-up)")
_log.close()
