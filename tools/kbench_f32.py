#!/usr/bin/env python3
"""f64 against f32 min-sum inside the circuit plan, on one GPU and the same trials.

  python tools/kbench_f32.py [--tag circ144] [--rates 0.005,0.003] [--iters 50] [--trials 32768] [--batch 16384] [--compare 4096] [--out FILE] [--append]

Part 0: the kernel's resources (hipcc -Rpass-analysis=kernel-resource-usage, when hipcc is on this machine) and what the f32 decoder reports for both
sectors (LDS, threads, resident workgroups per CU, form).  Part 1: per error rate one plan per precision on the same seed: converged fraction per
sector, mean iterations, ms of the BP bracket per sector batch, the share of the OSD brackets in the plan's device time, whole-plan trials/s and the
logical error rate; then the ratio of the BP brackets beside the structural expectation (about 2x: 2-cycle instead of 4-cycle issue and >= 2
workgroups per CU) and the statistical criterion |LER32 - LER64| <= 3 sqrt(2 LER64 (1 - LER64) / N), also applied to the converged fractions.
Part 2: the first --compare trials through both decode calls: the share whose BP outcome (conv, final_iter, err) is the same in f32 and f64.
The f64 rows run the f64 kernels of this tree, which the f32 decoder does not touch.  Matrices of rates that are not bundled come from the builder.
Everything printed is also written to --out (default profiles/r11_f32.txt).  Run one --tag per process, each under its own timeout.
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
ap.add_argument("--iters", type=int, default=50)
ap.add_argument("--trials", type=int, default=32768)
ap.add_argument("--batch", type=int, default=16384)
ap.add_argument("--compare", type=int, default=4096, help="trials of part 2 (per-shot comparison of the two decode calls)")
ap.add_argument("--flags", type=lambda x: int(x, 0), default=0, help="QLDPC_FLAG_F32_* form selectors for the f32 plans")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_f32.txt"))
ap.add_argument("--append", action="store_true")
ap.add_argument("--seed", type=int, default=20261018)
a = ap.parse_args()
T = _lib.TALLY
_log = open(a.out, "a" if a.append else "w")


def say(msg=""):
    print(msg, flush=True)
    _log.write(msg + "\n")
    _log.flush()


if not a.append:
    say("f32 against f64 min-sum in the circuit plan -- tools/kbench_f32.py")
    src = os.path.join(ROOT, "qldpc-branched-off_amd", "csrc", "minsum_f32.hip")
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
                cur = ln.split("minsum_f32_kernelILi")[1].split("EEE")[0] if "minsum_f32_kernel" in ln else None
                if cur:
                    say(f"kernel resources, minsum_f32_kernel<BLOCK={cur.split('ELb')[0]}, CLEAN={cur.split('ELb')[1]}>:")
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
say(f"\n{a.tag}: Z {gr[0].m} x {gr[0].n}, X {gr[1].m} x {gr[1].n}, {cycles} cycles, maxIter {a.iters}, batch {a.batch}, {a.trials} trials per plan, seed {a.seed}")

first = True
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
    if first:
        for s, g, q in zip("ZX", gr, pr):
            dec = _lib.Minsum32Decoder(g, q, max_iter=a.iters, flags=a.flags)
            say(f"  f32 decoder, sector {s}: {dec.info()}")
            dec.close()
        first = False
    rows = {}
    for precision in ("f64", "f32"):
        plan = _lib.CircuitPlan(comp, c["Lx"], c["Lz"], gr[0], gr[1], pr[0], pr[1], mk[0], mk[1], p, max_iter=a.iters, use_osd=True,
                                flags=a.flags if precision == "f32" else 0, batch=a.batch)
        if precision == "f32":
            plan.use_f32()
        plan.run(a.seed + 1, 0, min(a.batch, 1024)); plan.read(clear=True); plan.phase_times()       # warm-up (module load, workspaces)
        t0 = time.perf_counter()
        plan.run(a.seed, 0, a.trials)
        tally = plan.read(clear=True)
        dt = time.perf_counter() - t0
        ph, nb = plan.phase_times()
        n = int(tally[T["trials"]])
        ph = {k: v / max(nb, 1) for k, v in ph.items()}
        ler = tally[T["total_err"]] / n
        conv = [int(tally[T["bp_conv_" + s]]) / n for s in "zx"]
        its = [int(tally[T["iters_" + s]]) / n for s in "zx"]
        rows[precision] = dict(dt=dt, ler=ler, conv=conv, ph=ph, n=n)
        say(f"  p={p:.3f} {precision}: converged Z {conv[0]:.4f} X {conv[1]:.4f}; mean iterations Z {its[0]:.2f} X {its[1]:.2f}; BP bracket per sector batch of "
            f"{a.batch}: Z {ph['bp_z']:.3f} ms X {ph['bp_x']:.3f} ms; OSD share of the device time {(ph['osd_z'] + ph['osd_x']) / max(sum(ph.values()), 1e-9):.3f}; "
            f"plan {n / dt:.4g} trials/s; LER {ler:.4g} +- {np.sqrt(ler * (1 - ler) / n):.2g} ({int(tally[T['total_err']])} / {n})")
        if precision == "f32" and a.compare > 0:
            cnt = min(a.compare, a.trials)
            spz, _, spx, _ = plan.sample(a.seed, 0, cnt)
            for s, g, q, synd in zip("ZX", gr, pr, (spz, spx)):
                e64, c64, _, i64 = _lib.minsum_decode_batch(g, synd, q, a.iters, "dynamical", 1.0, want_llr=False)
                dec = _lib.Minsum32Decoder(g, q, max_iter=a.iters, flags=a.flags)
                e32, c32, _, i32 = dec.decode(synd)
                dec.close()
                same = (c64 == c32) & (i64 == i32) & (e64 == e32).all(axis=1)
                both = (c64 == 1) & (c32 == 1)
                say(f"      sector {s}, first {cnt} trials: BP outcome (conv, final_iter, err) equal in {same.mean():.4f}; among the shots converged in both "
                    f"{same[both].mean() if both.any() else float('nan'):.4f}; converged in one only {int((c64 != c32).sum())}")
        plan.close()
    f, g32 = rows["f64"], rows["f32"]
    n = f["n"]
    ratio = (f["ph"]["bp_z"] + f["ph"]["bp_x"]) / max(g32["ph"]["bp_z"] + g32["ph"]["bp_x"], 1e-9)
    bound = lambda x: 3.0 * np.sqrt(2.0 * x * (1.0 - x) / n)                  # noqa: E731  three sigma of a difference of two independent estimates
    say(f"      f64 / f32: BP bracket x{ratio:.2f} (structural expectation about x2; below x1.3 see DESIGN 4.9), trials/s x{f['dt'] / g32['dt']:.2f}")
    say(f"      criterion |LER32 - LER64| = {abs(g32['ler'] - f['ler']):.4g} <= {bound(f['ler']):.4g}: {'equivalent' if abs(g32['ler'] - f['ler']) <= bound(f['ler']) else 'NOT equivalent'}; "
        + "; ".join(f"converged {s} |{g32['conv'][i]:.4f} - {f['conv'][i]:.4f}| <= {bound(f['conv'][i]):.4g}: "
                    f"{'yes' if abs(g32['conv'][i] - f['conv'][i]) <= bound(f['conv'][i]) else 'NO'}" for i, s in enumerate("ZX")))
_log.close()
