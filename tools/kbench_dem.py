#!/usr/bin/env python3
"""Phase split, trials/s and logical error rate of a DEM plan built from shipped decoding matrices, beside the circuit plan of the same matrices on
the same GPU:  python tools/kbench_dem.py [--tag circ144] [--trials 100000] [--batch 16384] [--out profiles/r13_dem.txt]
The two plans sample different noise (independent columns are not circuit faults), so nothing here is a bar: the sampler bracket is read against the
circuit plan's `sample` bracket and against its own `bp_z` bracket, the logical error rates side by side.
--circuit-only: the circuit plan alone; --build <file in csrc/>: another build of the same ABI (timers, an A/B build).  The circuit plan's split at the
parent commit comes from that commit's own tools/kbench_circuit.py --tag circ144 --trials 100000 (its library lacks qldpc_circuit_plan_create_dem)."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qldpc_amd  # noqa: F401,E402
from qldpc_amd import _lib  # noqa: E402
from qldpc_amd.data import load_code, load_circuit_matrices  # noqa: E402
from qldpc_amd.codes.bb_code import BBCodeCircuit  # noqa: E402
from qldpc_amd.noise.compiled import CompiledCircuit  # noqa: E402
from qldpc_amd.simulation.engine import prior_llrs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tag", default="circ144")
ap.add_argument("--trials", type=int, default=100000)
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--max-iter", type=int, default=50)
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--circuit-only", action="store_true")
ap.add_argument("--build", default="", help="a library file name in csrc/")
ap.add_argument("--out", default="", help="append the report to this file as well")
a = ap.parse_args()
if a.build:
    _lib.select_build(a.build)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


def measure(name, plan):
    T = _lib.TALLY
    plan.run(1, 0, min(a.batch, 256)); plan.read(clear=True)            # warm-up: allocations, first launches
    for rep in range(a.reps):
        plan.phase_times()
        t0 = time.perf_counter()
        plan.run(5, 0, a.trials)
        t = plan.read(clear=True)
        dt = time.perf_counter() - t0
        ph, nb = plan.phase_times()
        say(f"{name} rep {rep}: {a.trials / dt:.0f} trials/s ({dt:.2f} s, {nb} batches of <= {a.batch}); LER {t[T['total_err']] / t[0]:.5f} "
            f"(z {t[T['z_err']] / t[0]:.5f}, x {t[T['x_err']] / t[0]:.5f}); BP converged z {t[T['bp_conv_z']] / t[0]:.3f} x {t[T['bp_conv_x']] / t[0]:.3f}; "
            f"OSD calls {t[T['osd_z']]}+{t[T['osd_x']]}; unsat {t[T['unsat_z']]}+{t[T['unsat_x']]}")
        say("    phases ms/batch: " + " ".join(f"{k}={v / max(nb, 1):.3f}" for k, v in ph.items()))
    return ph, nb


say(f"== tools/kbench_dem.py --tag {a.tag} --trials {a.trials} --batch {a.batch} --max-iter {a.max_iter}; library {os.path.basename(_lib.SO_PATH)}")
d = load_circuit_matrices(a.tag)
c = load_code(str(d["code"]))
cb = BBCodeCircuit(c["Hx"], c["Hz"], num_cycles=int(d["num_cycles"]), ell=c["ell"], m=c["m_dim"], a_x_powers=c["a_x_powers"],
                   a_y_powers=c["a_y_powers"], b_y_powers=c["b_y_powers"], b_x_powers=c["b_x_powers"])
comp = CompiledCircuit(cb.get_full_circuit(), cb.cycle * 2, cb.lin_order, cb.data_qubits, cb.Xchecks, cb.Zchecks)
gr, pr, mk = [], [], []
for s in "ZX":
    n = int(d[f"Hdec{s}_shape"][1])
    gr.append(_lib.Graph(d[f"Hdec{s}_indptr"], d[f"Hdec{s}_indices"], n))
    pr.append(prior_llrs(d[f"channel_probs{s}"]))
    mk.append(_lib.logical_column_masks((d[f"H{s}_logical_indptr"], d[f"H{s}_logical_indices"]), n))
cplan = _lib.CircuitPlan(comp, c["Lx"], c["Lz"], gr[0], gr[1], pr[0], pr[1], mk[0], mk[1], 0.005, max_iter=a.max_iter, batch=a.batch)
cph, cnb = measure(f"circuit plan ({a.tag}, p = 0.005 on every op)", cplan)
cplan.close()
if not a.circuit_only:
    from qldpc_amd.simulation.dem import DetectorErrorModel
    dem = DetectorErrorModel.from_decoding_matrices(a.tag)
    dplan = dem.plan(gr, max_iter=a.max_iter, batch=a.batch)
    say(f"DEM: {dem.n_mech} mechanisms (the columns of HdecZ then HdecX, one empty column per sector left out), detectors {dem.n_det}, k {dem.k}; "
        f"sum of p {dem.prob.sum():.2f} = mean mechanisms firing per trial")
    dph, dnb = measure(f"DEM plan (from_decoding_matrices({a.tag!r}))", dplan)
    dplan.close()
    ds, cs, bz = dph["sample"] / max(dnb, 1), cph["sample"] / max(cnb, 1), dph["bp_z"] / max(dnb, 1)
    say(f"sampler bracket: DEM {ds:.3f} ms/batch vs circuit {cs:.3f} ms/batch ({ds / cs:.2f}x); DEM bp_z bracket {bz:.3f} ms/batch -> the DEM sampler "
        f"{'EXCEEDS' if ds > bz else 'is below'} the bp_z bracket")
if a.out:
    with open(a.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
