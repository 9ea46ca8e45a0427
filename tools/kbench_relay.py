#!/usr/bin/env python3
"""Relay-BP against BP + OSD-0 on one GPU (config-5 shape: [[144,12,12]] x 12 cycles, bundled circ144 matrices, plan-sampled trials).

  python tools/kbench_relay.py [--trials N] [--batch B] [--sim-trials N] [--rates 0.003,0.004,0.005]

Part 1: one circuit plan per decoder on the same trials and seed, both sectors on one stream (exclusive hipEvent spans): ms of the
Relay-BP kernel per sector batch, legs and iterations per trial, trials/s of the whole plan.  Part 2: run_simulation with both decoders
at each error rate (the builder makes the matrices of rates that are not bundled): logical error rate with its binomial standard
error, and trials/s.  Relay-BP parameters: _lib.RELAY_DEFAULTS unless overridden with --relay t0=..,max_legs=..
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
ap.add_argument("--relay", default="", help="Relay-BP parameter overrides, e.g. t0=80,max_legs=100")
ap.add_argument("--seed", type=int, default=20261016)
a = ap.parse_args()
relay = {}
for kv in filter(None, a.relay.split(",")):
    k, v = kv.split("=")
    relay[k] = float(v) if "." in v or "e" in v else int(v)
params = _lib.relay_params(dict(relay), with_clip=False)
T = _lib.TALLY
print(f"Relay-BP parameters: {params}", flush=True)

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
print(f"{a.tag}: Z {gr[0].m} x {gr[0].n}, X {gr[1].m} x {gr[1].n}, {int(d['num_cycles'])} cycles, batch {a.batch}, {a.trials} trials, seed {a.seed}", flush=True)

rows = {}
for name in ("bp_osd0", "relay_bp"):
    plan = _lib.CircuitPlan(comp, c["Lx"], c["Lz"], gr[0], gr[1], pr[0], pr[1], mk[0], mk[1], 0.005, max_iter=50, use_osd=True,
                            flags=_lib.FLAG_MC_UNFUSED, batch=a.batch)
    if name == "relay_bp":
        plan.use_relay(**params)
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
    print(f"\n[{name}] {trials} trials in {dt:.3f} s = {trials / dt:.4g} trials/s; logical errors {int(tally[T['total_err']])} "
          f"(LER {ler:.4g} +- {np.sqrt(ler * (1 - ler) / trials):.2g})", flush=True)
    print("  ms per batch of " + str(a.batch) + ": " + ", ".join(f"{k} {v:.3f}" for k, v in rows[name]["ph"].items()), flush=True)
    print(f"  converged per trial: Z {tally[T['bp_conv_z']] / trials:.4f}  X {tally[T['bp_conv_x']] / trials:.4f};  iterations per trial: "
          f"Z {tally[T['iters_z']] / trials:.2f}  X {tally[T['iters_x']] / trials:.2f};  OSD-0 calls Z {int(tally[T['osd_z']])} X {int(tally[T['osd_x']])}", flush=True)
    if name == "relay_bp":
        print(f"  legs per trial: Z {tally[T['legs_z']] / trials:.3f}  X {tally[T['legs_x']] / trials:.3f};  unsatisfied outputs Z {int(tally[T['unsat_z']])} "
              f"X {int(tally[T['unsat_x']])};  Relay-BP kernel per sector batch (hipEvent): Z {rows[name]['ph']['bp_z']:.3f} ms  X {rows[name]['ph']['bp_x']:.3f} ms",
              flush=True)
print(f"\nwhole plan, same trials: Relay-BP {rows['relay_bp']['dt'] / rows['bp_osd0']['dt']:.2f}x the time of BP + OSD-0", flush=True)

print(f"\nrun_simulation, [[144,12,12]] x {int(d['num_cycles'])} cycles, {a.sim_trials} trials per point (LER +- binomial standard error)", flush=True)
for p in (float(x) for x in a.rates.split(",")):
    pre = load_precomputed_matrices(a.tag) if abs(p - 0.005) < 1e-12 and a.tag == "circ144" else None
    if pre is None:
        from qldpc_amd.noise.builder import build_decoding_matrices
        t0 = time.perf_counter()
        pre = build_decoding_matrices(cb, c["Lx"], c["Lz"], p, verbose=False)
        print(f"  (p = {p}: decoding matrices built in {time.perf_counter() - t0:.1f} s)", flush=True)
    for dec in ("bp_osd", "relay_bp"):
        kw = dict(decoder=dec, relay_params=dict(params)) if dec == "relay_bp" else {}
        t0 = time.perf_counter()
        r = run_simulation(c["Hx"], c["Hz"], c["Lx"], c["Lz"], p, num_trials=a.sim_trials, num_cycles=int(d["num_cycles"]), maxIter=50,
                           precomputed_matrices=pre, base_seed=a.seed, batch=a.batch, devices=[0], **bb, **kw)
        dt = time.perf_counter() - t0
        ler, nt = r["logical_error_rate"], r["num_trials"]
        extra = f"  legs/trial Z {r['mean_legs_z']:.3f} X {r['mean_legs_x']:.3f}" if dec == "relay_bp" else ""
        print(f"  p={p:.3f} {dec:8s}: LER {ler:.4g} +- {np.sqrt(ler * (1 - ler) / nt):.2g}  ({r['logical_errors'] if 'logical_errors' in r else int(r['tally'][T['total_err']])}"
              f" / {nt});  {nt / dt:.4g} trials/s (wall, incl. plan set-up){extra}", flush=True)
