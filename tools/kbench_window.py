#!/usr/bin/env python3
"""Sliding-window decoding against whole-graph BP + OSD-0 on one GPU.

  python tools/kbench_window.py [--tag circ144] [--trials N] [--batch B] [--configs 4:2,6:3,8:4] [--rates 0.005,0.003] [--long bb72:30,bb144:36]

Part 1: one circuit plan per decoder on the same trials and seed at every error rate (the builder makes the matrices of rates that are not
bundled): logical error rate with its binomial standard error, trials/s, the unsatisfied-trial rate, OSD-0 trials, the hipEvent phase
times per batch, and per sector how many windows / distinct graphs there are and how many windows take the LDS-resident workgroup decoder.
Part 2 (--long code:cycles): run_simulation of a long memory experiment, windowed (the first --configs entry) against the whole graph.
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
from qldpc_amd.noise.builder import build_decoding_matrices  # noqa: E402
from qldpc_amd.noise.compiled import CompiledCircuit  # noqa: E402
from qldpc_amd.simulation.engine import prior_llrs, run_simulation  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tag", default="circ144")
ap.add_argument("--trials", type=int, default=32768)
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--configs", default="4:2,6:3,8:4")
ap.add_argument("--rates", default="0.005,0.003")
ap.add_argument("--long", default="")
ap.add_argument("--long-trials", type=int, default=8192)
ap.add_argument("--seed", type=int, default=20261017)
a = ap.parse_args()
configs = [tuple(int(x) for x in c.split(":")) for c in filter(None, a.configs.split(","))]
T = _lib.TALLY


def bb_of(c):
    return dict(ell=c["ell"], m=c["m_dim"], a_x_powers=c["a_x_powers"], a_y_powers=c["a_y_powers"], b_y_powers=c["b_y_powers"], b_x_powers=c["b_x_powers"])


d = load_circuit_matrices(a.tag)
c = load_code(str(d["code"]))
cycles = int(d["num_cycles"])
cb = BBCodeCircuit(c["Hx"], c["Hz"], num_cycles=cycles, **bb_of(c))
comp = CompiledCircuit(cb.get_full_circuit(), cb.cycle * 2, cb.lin_order, cb.data_qubits, cb.Xchecks, cb.Zchecks)
k = np.asarray(c["Lx"]).shape[0]
for p in (float(x) for x in filter(None, a.rates.split(","))):
    if abs(p - float(d["error_rate"])) < 1e-12:
        pre = load_precomputed_matrices(a.tag)
    else:
        t0 = time.perf_counter()
        pre = build_decoding_matrices(cb, c["Lx"], c["Lz"], p, verbose=False)
        print(f"(p = {p}: decoding matrices built in {time.perf_counter() - t0:.1f} s)", flush=True)
    gr, pr, mk = [], [], []
    for s in "ZX":
        ip, ix, shape = _lib.canonical_csr(pre[f"Hdec{s}"])
        gr.append(_lib.Graph(ip, ix, shape[1]))
        pr.append(prior_llrs(np.asarray(pre[f"channel_probs{s}"], dtype=np.float64)))
        if f"H{s}_logical" in pre:
            mk.append(_lib.logical_column_masks(pre[f"H{s}_logical"], shape[1]))
        else:
            flr = int(pre[f"first_logical_row{s}"])
            mk.append(_lib.logical_column_masks(np.asarray(pre[f"H{s}_full"])[flr:flr + k], shape[1]))
    print(f"\n== {a.tag} p = {p}: Z {gr[0].m} x {gr[0].n}, X {gr[1].m} x {gr[1].n}, {cycles} cycles, batch {a.batch}, {a.trials} trials, seed {a.seed}", flush=True)
    base = None
    for cfg in [None] + configs:
        plan = _lib.CircuitPlan(comp, c["Lx"], c["Lz"], gr[0], gr[1], pr[0], pr[1], mk[0], mk[1], p, max_iter=50, use_osd=True, batch=a.batch)
        name = "whole graph"
        if cfg:
            plan.use_window(*cfg)
            name = f"window ({cfg[0]}, {cfg[1]})"
            infos = []
            for g, prior, lr in ((gr[0], pr[0], len(cb.Xchecks)), (gr[1], pr[1], len(cb.Zchecks))):
                dec = _lib.WindowDecoder(g, lr, cfg[0], cfg[1], prior)
                infos.append(dec.info())
                dec.close()
        plan.run(a.seed + 1, 0, min(a.batch, 2048)); plan.read(clear=True); plan.phase_times()     # warm-up (module load, workspaces)
        t0 = time.perf_counter()
        plan.run(a.seed, 0, a.trials)
        tally = plan.read(clear=True)
        dt = time.perf_counter() - t0
        ph, nb = plan.phase_times()
        plan.close()
        n = int(tally[T["trials"]])
        ler = tally[T["total_err"]] / n
        if base is None:
            base = dt
        print(f"[{name}] {n / dt:.4g} trials/s ({dt / base:.2f}x the whole-graph time); LER {ler:.5f} +- {np.sqrt(ler * (1 - ler) / n):.5f} "
              f"({int(tally[T['total_err']])} / {n}); unsatisfied trials Z {tally[T['unsat_z']] / n:.5f} X {tally[T['unsat_x']] / n:.5f}; "
              f"trials through OSD-0 Z {tally[T['osd_z']] / n:.4f} X {tally[T['osd_x']] / n:.4f}; iterations per trial Z {tally[T['iters_z']] / n:.1f} "
              f"X {tally[T['iters_x']] / n:.1f}", flush=True)
        print("    ms per batch: " + ", ".join(f"{kk} {v / max(nb, 1):.3f}" for kk, v in ph.items()), flush=True)
        if cfg:
            print("    windows per sector: " + "; ".join(f"{'ZX'[i]} {x['windows']} windows on {x['graphs']} graphs, largest {x['max_rows']} x {x['max_cols']}, "
                                                           f"{x['wg2_windows']} on the LDS-resident workgroup decoder (wg2)" for i, x in enumerate(infos)), flush=True)

for item in filter(None, a.long.split(",")):
    code, cyc = item.split(":")
    cyc = int(cyc)
    c = load_code(code)
    cb = BBCodeCircuit(c["Hx"], c["Hz"], num_cycles=cyc, **bb_of(c))
    t0 = time.perf_counter()
    pre = build_decoding_matrices(cb, c["Lx"], c["Lz"], 0.005, verbose=False)
    rows = _lib.canonical_csr(pre["HdecZ"])[2][0]
    print(f"\n== {code} x {cyc} cycles, p = 0.005: {rows} rows per sector (matrices built in {time.perf_counter() - t0:.1f} s), {a.long_trials} trials", flush=True)
    for cfg in (None, configs[0]):
        for rep in range(2):                                              # the second call is the measurement (module load, first allocations)
            t0 = time.perf_counter()
            r = run_simulation(c["Hx"], c["Hz"], c["Lx"], c["Lz"], 0.005, num_trials=a.long_trials, num_cycles=cyc, maxIter=50, precomputed_matrices=pre,
                               base_seed=a.seed, batch=min(a.batch, a.long_trials), devices=[0], window=cfg, **bb_of(c))
            dt = time.perf_counter() - t0
        ler, nt = r["logical_error_rate"], r["num_trials"]
        print(f"[{'whole graph' if cfg is None else f'window {cfg}'}] {nt / dt:.4g} trials/s (wall, incl. plan set-up); LER {ler:.5f} +- {np.sqrt(ler * (1 - ler) / nt):.5f}; "
              f"unsatisfied Z {r['tally'][T['unsat_z']]} X {r['tally'][T['unsat_x']]}; ms per batch: "
              + ", ".join(f"{kk} {v:.2f}" for kk, v in r.get("phase_ms_per_batch", {}).items()), flush=True)
