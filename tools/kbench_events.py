#!/usr/bin/env python3
"""Phase split of decode_events beside run_outcomes on the same plan and the same trials:
    python tools/kbench_events.py [--tag circ144] [--trials 65536] [--batch 16384] [--reps 3] [--out profiles/r17_events.txt]
The records are packed from the plan's own sample(), so both calls decode the same syndromes; the runs alternate (run_outcomes, decode_events, ...) and the
spread over the repetitions is printed beside the means.  What is read against what: `sample` of decode_events (copy + unpack) against `sample` of
run_outcomes (the Philox sampler); `judge` (predict) against `judge`; the BP / OSD brackets against each other.
--dev: additionally the _dev form on records that already sit on the device (no copy inside the bracket).  --build <file in csrc/>: another build."""
import argparse
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one the library then binds to)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qldpc_amd  # noqa: F401,E402
from qldpc_amd import _lib  # noqa: E402
from qldpc_amd.data import load_code, load_circuit_matrices  # noqa: E402
from qldpc_amd.codes.bb_code import BBCodeCircuit  # noqa: E402
from qldpc_amd.noise.compiled import CompiledCircuit  # noqa: E402
from qldpc_amd.simulation.engine import prior_llrs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tag", default="circ144")
ap.add_argument("--trials", type=int, default=65536)
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--max-iter", type=int, default=50)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--dev", action="store_true")
ap.add_argument("--build", default="", help="a library file name in csrc/")
ap.add_argument("--out", default="", help="append the report to this file as well")
a = ap.parse_args()
if a.build:
    _lib.select_build(a.build)
lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


say(f"== tools/kbench_events.py --tag {a.tag} --trials {a.trials} --batch {a.batch} --max-iter {a.max_iter} --reps {a.reps}; library {os.path.basename(_lib.SO_PATH)}")
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
plan = _lib.CircuitPlan(comp, c["Lx"], c["Lz"], gr[0], gr[1], pr[0], pr[1], mk[0], mk[1], 0.005, max_iter=a.max_iter, batch=a.batch)
seed, begin = 5, 0
spz, tz, spx, tx = plan.sample(seed, begin, a.trials)
records = _lib.pack_events(np.hstack([spz, spx]))                # the default layout: sector Z's rows, then sector X's
say(f"{a.trials} records of {records.shape[1]} bytes ({spz.shape[1]} + {spx.shape[1]} detectors), packed from the plan's own sample(seed {seed}, begin {begin})")
plan.run_outcomes(1, 0, min(a.batch, 256)); plan.read(clear=True)            # warm-up: allocations, first launches
plan.decode_events(records[:min(a.batch, 256)], seed, begin)
plan.phase_times()
rows = {"run_outcomes": [], "decode_events": []}
outcome = pred = None
for rep in range(a.reps):
    for name in rows:
        t0 = time.perf_counter()
        if name == "run_outcomes":
            outcome = plan.run_outcomes(seed, begin, a.trials)
            plan.read(clear=True)
        else:
            pred = plan.decode_events(records, seed, begin)
        dt = time.perf_counter() - t0
        ph, nb = plan.phase_times()
        rows[name].append([v / max(nb, 1) for v in ph.values()])
        say(f"{name} rep {rep}: {a.trials / dt:.0f} shots/s ({dt:.2f} s, {nb} batches of <= {a.batch}); phases ms/batch: "
            + " ".join(f"{k}={v / max(nb, 1):.3f}" for k, v in ph.items()))
truth = [tz, tx]
verdict = np.zeros(a.trials, np.uint8)
for s in range(2):
    bits = ((pred[s][:, None] >> np.arange(truth[s].shape[1], dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.int8)
    verdict |= (bits != truth[s]).any(axis=1).astype(np.uint8) << np.uint8(s)
say(f"verdicts of decode_events against run_outcomes: {int((verdict != outcome).sum())} of {a.trials} differ")
names = list(_lib.CIRCUIT_PHASES)
for name, r in rows.items():
    r = np.array(r)
    say(f"{name:14s} mean ms/batch: " + " ".join(f"{k}={r[:, i].mean():.3f}" for i, k in enumerate(names)) + "   spread (max - min): "
        + " ".join(f"{k}={r[:, i].max() - r[:, i].min():.3f}" for i, k in enumerate(names)))
ro, de = np.array(rows["run_outcomes"]), np.array(rows["decode_events"])
for i, k in enumerate(names):
    spread = max(ro[:, i].max() - ro[:, i].min(), de[:, i].max() - de[:, i].min())
    diff = de[:, i].mean() - ro[:, i].mean()
    what = ("copy + unpack vs the sampler" if k == "sample" else "predict vs the judge" if k == "judge" else "the same launches")
    say(f"  {k:6s} decode_events - run_outcomes = {diff:+.3f} ms/batch (spread {spread:.3f}): {'ABOVE the bar' if diff > spread else 'within the bar'}  [{what}]")
if a.dev:
    dev = torch.device("cuda", 0)
    d_rec = torch.from_numpy(records).to(dev)
    d_p0, d_p1 = torch.zeros(a.trials, dtype=torch.int64, device=dev), torch.zeros(a.trials, dtype=torch.int64, device=dev)
    d_fl = torch.zeros(a.trials, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)
    for rep in range(a.reps):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        plan.decode_events_dev(d_rec.data_ptr(), a.trials, records.shape[1], d_p0.data_ptr(), d_p1.data_ptr(), d_fl.data_ptr(), seed=seed, shot_begin=begin,
                               stream=stream.cuda_stream)
        stream.synchronize()
        dt = time.perf_counter() - t0
        ph, nb = plan.phase_times()
        say(f"decode_events_dev rep {rep}: {a.trials / dt:.0f} shots/s ({dt:.2f} s); phases ms/batch: " + " ".join(f"{k}={v / max(nb, 1):.3f}" for k, v in ph.items()))
    same = np.array_equal(d_p0.cpu().numpy().view(np.uint64), pred[0]) and np.array_equal(d_p1.cpu().numpy().view(np.uint64), pred[1]) and np.array_equal(d_fl.cpu().numpy(), pred[2])
    say(f"decode_events_dev results equal decode_events: {same}")
plan.close()
if a.out:
    with open(a.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
