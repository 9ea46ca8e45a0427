#!/usr/bin/env python3
"""Flooding against layered min-sum inside the circuit plan, on one GPU and the same trials.

  python tools/kbench_layered.py [--tag circ144] [--rates 0.005,0.003] [--iters 50,12] [--trials 32768] [--batch 16384] [--osd-cs N] [--out FILE] [--append]

Part 0: the kernel's resources (hipcc -Rpass-analysis=kernel-resource-usage, when hipcc is on this machine) and what the decoder reports for both
sectors (layers, LDS, form).  Part 1: per error rate and maxIter one plan per schedule on the same seed: converged fraction per sector, mean
iterations over all shots and over the converged ones, ms of the BP bracket per sector batch, the share of the OSD brackets in the plan's
device time, whole-plan trials/s, and the logical error rate with its binomial standard error.  Matrices of rates that are not bundled come from
the builder.  Everything printed is also written to --out (default profiles/r08_layered.txt).  Run one --tag per process, each under its own timeout.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import qldpc_amd  # noqa: F401,E402
from qldpc_amd import _lib  # noqa: E402
from qldpc_amd.data import load_code, load_circuit_matrices  # noqa: E402
from qldpc_amd.codes.bb_code import BBCodeCircuit  # noqa: E402
from qldpc_amd.noise.compiled import CompiledCircuit  # noqa: E402
from qldpc_amd.noise.builder import build_decoding_matrices  # noqa: E402
from qldpc_amd.simulation.engine import prior_llrs  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--tag", default="circ144")
ap.add_argument("--rates", default="0.005,0.003")
ap.add_argument("--iters", default="50,12")
ap.add_argument("--trials", type=int, default=32768)
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--osd-cs", type=int, default=-1, help="run OSD-CS of this order in the OSD stage instead of OSD-0")
ap.add_argument("--flags", type=lambda x: int(x, 0), default=0, help="QLDPC_FLAG_LAYERED_* form selectors for the layered plans")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_layered.txt"))
ap.add_argument("--append", action="store_true")
ap.add_argument("--seed", type=int, default=20261017)
a = ap.parse_args()
T = _lib.TALLY
_log = open(a.out, "a" if a.append else "w")


def say(msg=""):
    print(msg, flush=True)
    _log.write(msg + "\n")
    _log.flush()


if not a.append:
    say("Layered against flooding min-sum in the circuit plan -- tools/kbench_layered.py")
    src = os.path.join(ROOT, "qldpc-branched-off_amd", "csrc", "minsum_layered.hip")
    hipcc = "/opt/rocm/bin/hipcc"
    if os.path.exists(hipcc):
        import subprocess
        import tempfile
        with tempfile.TemporaryDirectory() as td:
            r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-c", src, "-o",
                                os.path.join(td, "o.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
        cur = None
        for ln in r.stderr.splitlines():
            if "remark:" not in ln:
                continue
            ln = ln.split("remark:")[1].replace("[-Rpass-analysis=kernel-resource-usage]", "").strip()
            if ln.startswith("Function Name:"):
                cur = ln.split("minsum_layered_kernelILb")[1][:7] if "minsum_layered_kernel" in ln else None
                if cur:
                    say(f"kernel resources, minsum_layered_kernel<VG={cur[0]}, IDXL={cur[4]}>:")
            elif cur and ln.split(":")[0] in ("VGPRs", "SGPRs Spill", "VGPRs Spill", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]"):
                say("    " + ln)

d = load_circuit_matrices(a.tag)
c = load_code(str(d["code"]))
cycles = int(d["num_cycles"])
bb = dict(ell=c["ell"], m=c["m_dim"], a_x_powers=c["a_x_powers"], a_y_powers=c["a_y_powers"], b_y_powers=c["b_y_powers"], b_x_powers=c["b_x_powers"])
cb = BBCodeCircuit(c["Hx"], c["Hz"], num_cycles=cycles, **bb)
comp = CompiledCircuit(cb.get_full_circuit(), cb.cycle * 2, cb.lin_order, cb.data_qubits, cb.Xchecks, cb.Zchecks)
gr, mk = [], []
for s in "ZX":
    n = int(d[f"Hdec{s}_shape"][1])
    gr.append(_lib.Graph(d[f"Hdec{s}_indptr"], d[f"Hdec{s}_indices"], n))
    mk.append(_lib.logical_column_masks((d[f"H{s}_logical_indptr"], d[f"H{s}_logical_indices"]), n))
say(f"\n{a.tag}: Z {gr[0].m} x {gr[0].n}, X {gr[1].m} x {gr[1].n}, {cycles} cycles, batch {a.batch}, {a.trials} trials per plan, seed {a.seed}, "
    f"OSD stage {'OSD-CS(' + str(a.osd_cs) + ')' if a.osd_cs >= 0 else 'OSD-0'}")

for p in (float(x) for x in a.rates.split(",")):
    if abs(p - float(d["error_rate"])) < 1e-12:
        probs = [np.asarray(d[f"channel_probs{s}"], np.float64) for s in "ZX"]
    else:                                                  # the matrices keep their structure; the channel probabilities are those of this rate
        M = build_decoding_matrices(cb, c["Lx"], c["Lz"], p, verbose=False)
        for s, g in zip("ZX", gr):
            ip, ix, shape = _lib.canonical_csr(M[f"Hdec{s}"])
            assert shape == (g.m, g.n) and np.array_equal(ip, g.indptr) and np.array_equal(ix, g.indices), "the builder's matrix differs from the bundled one"
        probs = [np.asarray(M[f"channel_probs{s}"], np.float64) for s in "ZX"]
    pr = [prior_llrs(x) for x in probs]
    for it in (int(x) for x in a.iters.split(",")):
        rows = {}
        for schedule in ("flooding", "layered"):
            plan = _lib.CircuitPlan(comp, c["Lx"], c["Lz"], gr[0], gr[1], pr[0], pr[1], mk[0], mk[1], p, max_iter=it, use_osd=True,
                                    flags=a.flags if schedule == "layered" else 0, batch=a.batch)
            if a.osd_cs >= 0:
                plan.use_osd_cs(a.osd_cs)
            if schedule == "layered":
                plan.use_layered()
                if p == float(a.rates.split(",")[0]) and it == int(a.iters.split(",")[0]):
                    for s, g, q in zip("ZX", gr, pr):
                        dec = _lib.LayeredDecoder(g, q, max_iter=it, flags=a.flags)
                        say(f"  layered decoder, sector {s}: {dec.info()}")
                        dec.close()
            plan.run(a.seed + 1, 0, min(a.batch, 1024)); plan.read(clear=True); plan.phase_times()       # warm-up (module load, workspaces)
            t0 = time.perf_counter()
            plan.run(a.seed, 0, a.trials)
            tally = plan.read(clear=True)
            dt = time.perf_counter() - t0
            ph, nb = plan.phase_times()
            plan.close()
            n = int(tally[T["trials"]])
            ph = {k: v / max(nb, 1) for k, v in ph.items()}
            ler = tally[T["total_err"]] / n
            conv = [int(tally[T["bp_conv_" + s]]) for s in "zx"]
            its = [int(tally[T["iters_" + s]]) for s in "zx"]
            mean_conv = [(its[i] - (n - conv[i]) * it) / max(conv[i], 1) for i in range(2)]
            rows[schedule] = dict(dt=dt, ler=ler, conv=conv, ph=ph)
            say(f"  p={p:.3f} maxIter={it:2d} {schedule:8s}: converged Z {conv[0] / n:.4f} X {conv[1] / n:.4f}; mean iterations all shots Z {its[0] / n:.2f} X {its[1] / n:.2f}, "
                f"converged shots Z {mean_conv[0]:.2f} X {mean_conv[1]:.2f}")
            say(f"      BP bracket per sector batch of {a.batch}: Z {ph['bp_z']:.3f} ms X {ph['bp_x']:.3f} ms; OSD Z {ph['osd_z']:.3f} X {ph['osd_x']:.3f} ms "
                f"(OSD share of the device time {(ph['osd_z'] + ph['osd_x']) / max(sum(ph.values()), 1e-9):.3f}); plan {n / dt:.4g} trials/s; "
                f"LER {ler:.4g} +- {np.sqrt(ler * (1 - ler) / n):.2g} ({int(tally[T['total_err']])} / {n})")
        f, l = rows["flooding"], rows["layered"]
        say(f"      layered / flooding: trials/s x{f['dt'] / l['dt']:.2f}; BP bracket x{(l['ph']['bp_z'] + l['ph']['bp_x']) / (f['ph']['bp_z'] + f['ph']['bp_x']):.2f}; "
            f"unconverged Z {1 - l['conv'][0] / a.trials:.4f} vs {1 - f['conv'][0] / a.trials:.4f}, X {1 - l['conv'][1] / a.trials:.4f} vs {1 - f['conv'][1] / a.trials:.4f}; "
            f"LER {l['ler']:.4g} vs {f['ler']:.4g}")
_log.close()
