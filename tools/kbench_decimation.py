#!/usr/bin/env python3
"""BP with guided decimation against flooding BP + OSD-0 on one GPU (config-5 shape: [[144,12,12]] x 12 cycles, plan-sampled trials, one seed).

  python tools/kbench_decimation.py --rate 0.005 [--trials 32768] [--batch 16384] [--per-round 1,8,32] [--t-round 6,12] [--budget 100,400] [--cs-order 7]

One circuit plan per row, all on the same trials: flooding BP + OSD-0 (the unswitched plan), then for every grid point
(per_round, t_round, max_rounds with t_round * (1 + max_rounds) = budget) decimation + OSD-0 and decimation + OSD-CS(cs-order).  Per row: converged
fraction per sector, mean iterations and rounds per trial, ms of the BP bracket per sector batch (hipEvent spans), the OSD share of the decode
time, whole-plan trials/s (wall clock of run + read, after a warm-up) and the logical error rate with its binomial standard error.  The matrices
of a rate that is not bundled (0.005 is) come from the builder.  One rate per invocation, so that a driver can give every GPU step its own limit:

  timeout -k 10 900 python tools/kbench_decimation.py --rate 0.005 > profiles/r09_decimation.txt && \\
  timeout -k 10 900 python tools/kbench_decimation.py --rate 0.003 >> profiles/r09_decimation.txt
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
from qldpc_amd.simulation.engine import prior_llrs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tag", default="circ144")
ap.add_argument("--rate", type=float, default=0.005)
ap.add_argument("--trials", type=int, default=32768)
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--per-round", default="1,8,32")
ap.add_argument("--t-round", default="6,12")
ap.add_argument("--budget", default="100,400", help="t_round * (1 + max_rounds)")
ap.add_argument("--alpha", type=float, default=1.0)
ap.add_argument("--fix-llr", type=float, default=50.0)
ap.add_argument("--cs-order", type=int, default=7)
ap.add_argument("--seed", type=int, default=20261018)
a = ap.parse_args()
T = _lib.TALLY

d = load_circuit_matrices(a.tag)
c = load_code(str(d["code"]))
bb = dict(ell=c["ell"], m=c["m_dim"], a_x_powers=c["a_x_powers"], a_y_powers=c["a_y_powers"], b_y_powers=c["b_y_powers"], b_x_powers=c["b_x_powers"])
cycles = int(d["num_cycles"])
cb = BBCodeCircuit(c["Hx"], c["Hz"], num_cycles=cycles, **bb)
comp = CompiledCircuit(cb.get_full_circuit(), cb.cycle * 2, cb.lin_order, cb.data_qubits, cb.Xchecks, cb.Zchecks)
if abs(a.rate - 0.005) < 1e-12:
    M = load_precomputed_matrices(a.tag)
else:
    from qldpc_amd.noise.builder import build_decoding_matrices
    t0 = time.perf_counter()
    M = build_decoding_matrices(cb, c["Lx"], c["Lz"], a.rate, verbose=False)
    print(f"(p = {a.rate}: decoding matrices built in {time.perf_counter() - t0:.1f} s)", flush=True)
k = np.asarray(c["Lx"]).shape[0]
gr, pr, mk = [], [], []
for s in "ZX":
    ip, ix, shape = _lib.canonical_csr(M[f"Hdec{s}"])
    gr.append(_lib.Graph(ip, ix, shape[1]))
    pr.append(prior_llrs(np.asarray(M[f"channel_probs{s}"], dtype=np.float64)))
    if f"H{s}_logical" in M:
        mk.append(_lib.logical_column_masks(M[f"H{s}_logical"], shape[1]))
    else:
        flr = int(M[f"first_logical_row{s}"])
        mk.append(_lib.logical_column_masks(np.asarray(M[f"H{s}_full"])[flr:flr + k], shape[1]))
print(f"\n== {a.tag} at p = {a.rate}: Z {gr[0].m} x {gr[0].n}, X {gr[1].m} x {gr[1].n}, {cycles} cycles, batch {a.batch}, {a.trials} trials, seed {a.seed}, "
      f"alpha {a.alpha}, fix_llr {a.fix_llr}, clip_llr 20 ==", flush=True)
print("row                                   | conv Z / X     | iters Z / X     | rounds Z / X  | BP ms/batch Z / X | OSD share | trials/s  | LER +- s.e.", flush=True)


def row(name, decim=None, cs=None):
    plan = _lib.CircuitPlan(comp, c["Lx"], c["Lz"], gr[0], gr[1], pr[0], pr[1], mk[0], mk[1], a.rate, max_iter=50, use_osd=True, flags=_lib.FLAG_MC_UNFUSED,
                            batch=a.batch)
    if cs is not None:
        plan.use_osd_cs(cs)
    if decim is not None:
        plan.use_decimation(**decim)
    plan.run(a.seed + 1, 0, min(a.batch, 1024)); plan.read(clear=True); plan.phase_times()   # warm-up (module load, workspaces)
    t0 = time.perf_counter()
    plan.run(a.seed, 0, a.trials)
    t = plan.read(clear=True)
    dt = time.perf_counter() - t0
    ph, nb = plan.phase_times()
    plan.close()
    n = int(t[T["trials"]])
    ph = {key: v / max(nb, 1) for key, v in ph.items()}
    dec = ph["bp_z"] + ph["bp_x"] + ph["osd_z"] + ph["osd_x"]
    ler = t[T["total_err"]] / n
    print(f"{name:37s} | {t[T['bp_conv_z']] / n:.4f} / {t[T['bp_conv_x']] / n:.4f} | {t[T['iters_z']] / n:6.1f} / {t[T['iters_x']] / n:6.1f} | "
          f"{t[T['legs_z']] / n:5.2f} / {t[T['legs_x']] / n:5.2f} | {ph['bp_z']:7.1f} / {ph['bp_x']:7.1f} | {(ph['osd_z'] + ph['osd_x']) / max(dec, 1e-9):9.3f} | "
          f"{n / dt:9.4g} | {ler:.4f} +- {np.sqrt(ler * (1 - ler) / n):.4f}  (unsat {int(t[T['unsat_z']] + t[T['unsat_x']])})", flush=True)
    return n / dt, ler


row("flooding BP(50) + OSD-0")
for budget in (int(x) for x in a.budget.split(",")):
    for tr in (int(x) for x in a.t_round.split(",")):
        for per in (int(x) for x in a.per_round.split(",")):
            p = _lib.decim_params(dict(alpha=a.alpha, t_round=tr, max_rounds=max(budget // tr - 1, 0), per_round=per, fix_llr=a.fix_llr), with_clip=False)
            tag = f"BPGD t{tr} r{p['max_rounds']} k{per}"
            row(f"{tag} + OSD-0", p)
            row(f"{tag} + OSD-CS({a.cs_order})", p, a.cs_order)
