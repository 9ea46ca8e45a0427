#!/usr/bin/env python3
"""BP + LSD against BP + OSD-0 on one GPU: the time of the plan's OSD stage, what the clusters did, and what the answers are worth.

  python tools/kbench_lsd.py [--shapes circ144@0.005,circ144@0.003,bb288x18@0.005] [--trials N] [--batch B] [--rounds R] [--out FILE]

Per shape (circ144: the bundled [[144,12,12]] x 12-cycle matrices at p = 0.005, built by the GPU builder at any other p; bb288x18: [[288,12,18]] x 18
cycles as in tools/kbench_big.py) three circuit plans on the same trials and seed: OSD-0 (a plan that is never switched: it enqueues what it enqueued
before LSD existed, so it is the yardstick), LSD at bits_per_step 1 and 4 (max_rows --max-rows).  The plans run in turn, --rounds times over
(alternating, so that a drift of the machine lands on all three); printed per plan: QLDPC_PHASE_OSD_Z / _X ms per batch (median and range over the
rounds), trials/s of the whole plan (median), the shots per sector that ended with flag 0 / 1 / 2, and the logical error rate.  Then, on one sampled
batch decoded by hand, the share of LSD answers that equal OSD-0's bit for bit, and the rounds / rows / columns of the flag-0 shots.
Everything printed is also written to --out (default profiles/r23_lsd.txt)."""
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

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="circ144@0.005,circ144@0.003,bb288x18@0.005")
ap.add_argument("--trials", type=int, default=32768)
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--big-trials", type=int, default=8192, help="trials of the bb288 shape")
ap.add_argument("--big-batch", type=int, default=4096)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--max-rows", type=int, default=512)
ap.add_argument("--by-hand", type=int, default=4096, help="trials of the batch decoded by hand for the share of equal answers")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_lsd.txt"))
ap.add_argument("--seed", type=int, default=20261020)
a = ap.parse_args()
T = _lib.TALLY
_log = open(a.out, "w")


def say(msg=""):
    print(msg, flush=True)
    _log.write(msg + "\n")
    _log.flush()


def problem(shape):
    name, p = shape.split("@")
    p = float(p)
    code, cycles = ("bb144", 12) if name == "circ144" else ("bb288", 18)
    c = load_code(code)
    bb = dict(ell=c["ell"], m=c["m_dim"], a_x_powers=c["a_x_powers"], a_y_powers=c["a_y_powers"], b_y_powers=c["b_y_powers"], b_x_powers=c["b_x_powers"])
    pre = load_precomputed_matrices("circ144") if name == "circ144" and abs(p - 0.005) < 1e-12 else None
    if pre is None:
        t0 = time.perf_counter()
        pre = build_decoding_matrices(BBCodeCircuit(c["Hx"], c["Hz"], num_cycles=cycles, **bb), c["Lx"], c["Lz"], p, verbose=False)
        say(f"  (decoding matrices of {shape} built in {time.perf_counter() - t0:.1f} s)")
    return p, engine._circuit_problem(c["Hx"], c["Hz"], c["Lx"], c["Lz"], p, cycles, pre, 0, bb)


def spread(v):
    return f"{np.median(v):.3f} ({min(v):.3f} .. {max(v):.3f})"


say("BP + LSD (cluster-local post-processing) against BP + OSD-0 -- tools/kbench_lsd.py")
say(f"max_rows {a.max_rows}, {a.rounds} alternating rounds per shape, seed {a.seed}; OSD-0 = a plan that is never switched (the parent's OSD stage, same kernels)")
for shape in a.shapes.split(","):
    say(f"\n== {shape}")
    p, prob = problem(shape)
    big = not shape.startswith("circ144")
    trials, batch = (a.big_trials, a.big_batch) if big else (a.trials, a.batch)
    gz, gx = prob.graphs
    say(f"Z {gz.m} x {gz.n}, X {gx.m} x {gx.n}; batch {batch}, {trials} trials per run")
    names = ["osd0", "lsd_b1", "lsd_b4"]
    plans = {}
    for name in names:
        plan = prob.make_plan(prob.graphs, 50, 1.0, 1.0, "dynamical", batch, 0)
        if name != "osd0":
            plan.use_lsd(int(name[5:]), a.max_rows)
        plan.run(a.seed + 1, 0, min(batch, 1024)); plan.read(clear=True); plan.phase_times(); plan.lsd_counts(clear=True)      # warm-up
        plans[name] = plan
    ms = {n: {"osd_z": [], "osd_x": [], "bp_z": [], "rate": []} for n in names}
    tallies, counts = {}, {}
    for rnd in range(a.rounds):
        for name in names:
            plan = plans[name]
            t0 = time.perf_counter()
            plan.run(a.seed, 0, trials)
            tallies[name] = plan.read(clear=True)
            dt = time.perf_counter() - t0
            ph, nb = plan.phase_times()
            counts[name] = plan.lsd_counts(clear=True)
            for k in ("osd_z", "osd_x", "bp_z"):
                ms[name][k].append(ph[k] / max(nb, 1))
            ms[name]["rate"].append(trials / dt)
    for name in names:
        t = tallies[name]
        ler = t[T["total_err"]] / t[T["trials"]]
        say(f"[{name}] OSD phase ms per batch: Z {spread(ms[name]['osd_z'])}  X {spread(ms[name]['osd_x'])};  BP Z {np.median(ms[name]['bp_z']):.3f};  "
            f"{np.median(ms[name]['rate']):.4g} trials/s")
        say(f"    OSD-stage shots Z {int(t[T['osd_z']])} X {int(t[T['osd_x']])}; LER {ler:.4g} +- {np.sqrt(ler * (1 - ler) / t[T['trials']]):.2g} "
            f"({int(t[T['total_err']])} / {int(t[T['trials']])}); unsatisfied Z {int(t[T['unsat_z']])} X {int(t[T['unsat_x']])}")
        if name != "osd0":
            c = counts[name]
            tot = max(int(c.sum()), 1)
            say(f"    flags 0 / 1 / 2: Z {c[0].tolist()} X {c[1].tolist()}; capped share {c[:, 1].sum() / tot:.4f}, without candidates {c[:, 2].sum() / tot:.4f}")
            say(f"    OSD stage against OSD-0: Z {np.median(ms[name]['osd_z']) / np.median(ms['osd0']['osd_z']):.2f}x  "
                f"X {np.median(ms[name]['osd_x']) / np.median(ms['osd0']['osd_x']):.2f}x")
    # one batch by hand: which answers equal OSD-0's
    count = min(a.by_hand, batch)
    sampled = plans["osd0"].sample(a.seed, 0, count)
    for plan in plans.values():
        plan.close()
    for sec, (g, prior) in enumerate(zip(prob.graphs, prob.llrs)):
        synd = sampled[2 * sec]
        det, conv, llr, _ = _lib.minsum_decode_batch(g, synd, prior, 50, "dynamical", 1.0)
        bad = np.flatnonzero(conv == 0)
        if not bad.size:
            say(f"  by hand, sector {'ZX'[sec]}: BP converged on all {count} shots")
            continue
        o0 = _lib.osd0_batch(g, synd[bad], llr[bad], det[bad])
        w0 = o0.sum(axis=1)
        for bits in (1, 4):
            sol, info = _lib.lsd_batch(g, synd[bad], llr[bad], det[bad], bits, a.max_rows)
            ok = info[:, 0] == 0
            same = (sol == o0).all(axis=1)
            line = f"  by hand, sector {'ZX'[sec]}, bits_per_step {bits}: {bad.size} unconverged of {count}; flag 0 on {int(ok.sum())}; equal to OSD-0 {int(same.sum())} ({same.mean():.4f})"
            if ok.any():
                line += (f", among flag 0 {same[ok].mean():.4f}; rounds mean {info[ok, 1].mean():.1f} max {info[ok, 1].max()}, rows mean {info[ok, 2].mean():.1f} max {info[ok, 2].max()}, "
                         f"columns mean {info[ok, 3].mean():.1f} max {info[ok, 3].max()}; weight LSD / OSD-0 {sol[ok].sum() / max(int(w0[ok].sum()), 1):.4f}")
            say(line)
_log.close()
