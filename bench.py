#!/usr/bin/env python3
"""Benchmark of the hot path on MI355X: decoded shots/sec, [[144,12,12]] code capacity, p = 0.005, 50 BP iterations
(BASELINE.json); with --full also the circuit-level trial pipeline (BASELINE config 5) in the same run.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]

A plain run times the headline leg alone (`value` below) and prints its JSON line; `--full` adds every other leg, the CPU
baselines and the checks against the oracle (`--p-sweep`, `--circuit`, `--legs`, `--no-cpu-baseline` shape what it adds).
`--dump-outputs DIR` writes what the headline leg's plan returned after its last timed step -- the int64[16] tally of the
timed steps, all ranks summed -- as DIR/tally.npy (float64); with the same arguments the shots are the same in every run.

One process per GPU.  `--gpus N` with WORLD_SIZE unset starts the N ranks itself (children, before anything touches the
GPU); under `torch.distributed.run` it reads RANK / LOCAL_RANK / WORLD_SIZE.  Shots are sharded by global shot index
(Philox streams keyed by it: tallies do not depend on N), there is no data-path collective, and ONE all-reduce of the
int64[16] tally (RCCL through torch.distributed "nccl") closes each timed region -- what replaces the reference's
pool.imap + Python tally loop (src/simulation/engine.py:433-457).

A "step" of the headline leg = one batch of `--batch` synthetic shots through the device-resident pipeline
(Philox sample -> GF(2) syndrome -> min-sum decode -> OSD-0 on failures -> logical compare -> tally); nothing crosses PCIe
inside the timed region.  Legs (all with max_iter = 50, identical tallies):
  * `value`: FIXED-WORK mode -- every shot executes all 50 iterations, outputs frozen at its first converged iteration:
    the accounting the 1e7 shots/s / 346,973 B/shot north-star target was derived in;
  * `reference_semantics`: the reference's per-shot early exit (kernels.py:361-364), ~1.03 iterations/shot here;
  * `circuit_level`: BASELINE config 5, [[144,12,12]] x (12 + 2) cycles at p = 0.005, one step = one batch of 16,384 trials,
    a trial = sample + decode Z + OSD-0 + decode X + OSD-0 + logical comparison (engine.py:68-122), with a hipEvent split.
`roofline` names the BINDING resource of the dominant kernel.  The messages of this decoder live in registers / LDS, so
HBM is not it (measured traffic is ~0.04 % of the streaming model's bytes): the bound is f64 VALU issue.  achieved = VALU
wave-instructions per second (instruction count from the committed PMC pass of the same kernel, time from hipEvents on
the launch stream in this run), peak = 1024 SIMDs x (shader clock measured in this run) / 4 cycles per wave-instruction.
`efficiency` sets the algorithmic floor of the reference's loop nest (f64 lane-operations, counted in DESIGN.md 5.1)
against the lane-slots actually issued.  The SURVEY 8d streaming-model bytes stay in `hbm_model` for reference.
`cpu_baseline` = the C oracle (a port of the reference loop nest, early-exit semantics) on the host cores over a bounded
sample of the same trial stream (rank 0 only, after the timed regions; the other ranks of an N > 1 run wait at the next barrier); a reported baseline, not the target.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

SEED = 20260206
HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec (MI355X_MICROARCH.md: 8.0 TB/s spec, ~6.3 TB/s achievable)
SIMDS = 256 * 4                # MI355X: 256 CUs x 4 SIMDs; one f64 / 32-bit VALU wave64 instruction issues per 4 cycles per SIMD
LABELS = {"bb72": "[[72,12,6]]", "bb144": "[[144,12,12]]", "bb288": "[[288,12,18]]", "bb90": "[[90,8,10]]", "bb108": "[[108,8,10]]",
          "steane": "[[7,1,3]]"}


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=1 << 20, help="shots per step per GPU (BASELINE config 2 is quoted at 4096)")
    ap.add_argument("--min-launch", type=int, default=0, help="launch granule of the code-capacity plan (0 = --batch taken literally; qldpc_cc_plan_create)")
    ap.add_argument("--code", default="bb144", help="bb72 = BASELINE config 2, bb144 = config 3 (headline), bb288 = config 4")
    ap.add_argument("--p", type=float, default=0.005)
    ap.add_argument("--p-sweep", default="", help="(--full) comma-separated error rates (BASELINE config 4: --code bb288 --p-sweep 0.004,0.005,0.006): the headline leg "
                                                  "once per point, one tally and one all-reduce per point, every point in the JSON line; `value` is the rate over all points")
    ap.add_argument("--max-iter", type=int, default=50)
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) leave out the CPU baselines and the oracle checks")
    ap.add_argument("--cpu-seconds", type=float, default=10.0, help="CPU work per baseline (each of the two legs)")
    ap.add_argument("--kernel", choices=["auto", "resident", "stream"], default="auto")
    ap.add_argument("--legs", choices=["both", "fixed"], default="both",
                    help="(--full) 'fixed' runs only the headline fixed-work leg (every launch in a rocprofv3 --stats summary is then the timed kernel)")
    ap.add_argument("--circuit", default=None, help="(--full) circuit-level leg: decoding matrices tag (circ72 / circ144 / circ288, default circ144) or 'none'")
    ap.add_argument("--circuit-batch", type=int, default=16384, help="trials per step per GPU")
    ap.add_argument("--circuit-steps", type=int, default=4)
    ap.add_argument("--circuit-warmup", type=int, default=1)
    ap.add_argument("--circuit-flags", type=lambda x: int(x, 0), default=0)
    ap.add_argument("--no-code-capacity", action="store_true", help="(--full) run only the circuit-level leg (profiling)")
    ap.add_argument("--full", action="store_true", help="every leg, CPU baseline and oracle check besides the headline leg")
    ap.add_argument("--dump-outputs", metavar="DIR", default="", help="write the headline leg's tally of the timed steps to DIR/tally.npy (float64)")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.full:
        args.circuit = "circ144" if args.circuit is None else args.circuit
    else:
        extra = [f for f, on in (("--p-sweep", bool(args.p_sweep)), ("--no-code-capacity", args.no_code_capacity),
                                 ("--circuit " + str(args.circuit), args.circuit not in (None, "none"))) if on]
        if extra:
            ap.error(f"{', '.join(extra)} measures beyond the headline leg: add --full")
        args.legs, args.circuit, args.no_cpu_baseline = "fixed", "none", True      # the plain run: the headline leg alone
    return args


def dump_outputs(path, arrays):
    """--dump-outputs: one DIR/<name>.npy (float64) per array the timed path returned."""
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), np.asarray(a, np.float64))


# --------------------------------------------------------------------------------------------------------------------------------
# launcher: `python bench.py --gpus N` starts its own N ranks (the reference's one-call launch, engine.py:433-435)
# --------------------------------------------------------------------------------------------------------------------------------
def launch_ranks(args):
    """Parent of an N-rank run.  Touches no GPU API: the ranks are fresh child processes with RANK / LOCAL_RANK / WORLD_SIZE /
    MASTER_* set; rank 0's JSON line passes through on stdout.  Returns the worst exit code."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    try:
        pending = list(procs)
        while pending:
            for p in list(pending):
                r = p.poll()
                if r is None:
                    continue
                pending.remove(p)
                if r != 0:
                    rc = rc or r
                    for q in pending:          # a rank failed: the others would wait in a collective forever
                        q.terminate()
            time.sleep(0.05)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    return rc


# --------------------------------------------------------------------------------------------------------------------------------
# PMC figures measured separately with rocprofv3 (tools/pmc_passes.sh -> tools/pmc_summarise.py -> profiles/pmc.json)
# --------------------------------------------------------------------------------------------------------------------------------
def source_digest(files):
    h = hashlib.sha256()
    for f in files:
        with open(os.path.join(ROOT, "qldpc-branched-off_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def pmc_entry(key):
    """The committed PMC record for `key`, or None when there is none or when the kernel's source changed since it was taken
    (a stale count is refused, not reported)."""
    try:
        with open(os.path.join(ROOT, "profiles", "pmc.json")) as fh:
            e = json.load(fh)["entries"][key]
        if e["source_digest"] != source_digest(e["sources"]):
            return None
        return e
    except (OSError, ValueError, KeyError):
        return None


def isa_entry(key):
    """The committed static instruction mix of the kernel behind PMC record `key` (tools/isa_mix.py --record -> profiles/isa_mix.json), or None
    when the kernel's sources changed since it was taken."""
    try:
        with open(os.path.join(ROOT, "profiles", "isa_mix.json")) as fh:
            e = json.load(fh)["entries"][key]
        if e["source_digest"] != source_digest(e["sources"]):
            return None
        return e
    except (OSError, ValueError, KeyError):
        return None


def issue_roofline(entry, mix, units_per_launch, ms_per_launch, clock_mhz, floor_cycles_per_unit, unit_name):
    """Binding-resource object: VALU instruction ISSUE of the 1024 SIMDs, in SIMD issue-cycles.

    A wave64 VALU instruction holds its SIMD's issue port for 2 cycles (add / sub / logic / shift-right / move, f32 add and mul) or 4 (every
    f64 or 64-bit instruction, every compare and v_cndmask, every three-operand integer instruction, v_mul_lo / hi, lane moves) -- measured
    per mnemonic on the box by tools/microbench/issue_rate.hip (profiles/r03_issue_rate.txt).  peak = 1024 SIMDs x shader clock (measured in
    this run) issue-cycles per second.
      achieved / frac : the ALGORITHMIC issue-cycles of the reference loop nest (every operation of kernels.py:282-359 priced
                        at the cheapest instruction that can do it) per second, over the kernel time of THIS run (hipEvents on the launch stream)
      issued_frac     : the issue-cycles the kernel actually spends = SQ_INSTS_VALU per unit (committed PMC pass of the same kernel) x
                        mean cycles per VALU instruction of its steady-state loop (committed static mix, tools/isa_mix.py)
    """
    if not entry or ms_per_launch <= 0:
        return None
    clock = clock_mhz if clock_mhz and clock_mhz > 0 else None
    peak = SIMDS * (clock or 2400.0) * 1e6                        # SIMD issue-cycles per second
    secs = ms_per_launch * 1e-3
    per_unit = entry["SQ_INSTS_VALU"] / entry["units_per_launch"]
    out = {"bound": "valu_issue", "unit": "G SIMD issue-cycles/s", "peak": round(peak / 1e9, 2), "achieved": None, "frac": None,
           "clock_mhz": round(clock, 1) if clock else None,
           "clock_source": "in-kernel s_memtime / s_memrealtime, median over workgroups, this run" if clock else "ASSUMED 2400 MHz (no probe)",
           "kernel": entry["kernel"], "kernel_ms_per_launch": round(ms_per_launch, 4),
           "valu_wave_insts_per_" + unit_name: round(per_unit, 2), "pmc_source": entry.get("source", "profiles/pmc.json"),
           "issue_rates_source": "profiles/r03_issue_rate.txt"}
    if floor_cycles_per_unit:
        ach = floor_cycles_per_unit * units_per_launch / secs
        out["achieved"] = round(ach / 1e9, 2)
        out["frac"] = round(ach / peak, 4)
        out["algorithmic_issue_cycles_per_" + unit_name] = round(floor_cycles_per_unit, 2)
    if mix:
        cpi = mix["valu_issue_cycles"] / max(mix["valu_instructions"], 1)
        issued = per_unit * cpi * units_per_launch / secs
        tot = max(mix["valu_instructions"], 1)
        out["issued_frac"] = round(issued / peak, 4)
        out["issue_cycles_per_" + unit_name] = round(per_unit * cpi, 2)
        out["issue_cycles_by_class"] = {c.replace("valu_", "") + "_cycle": round(per_unit * k / tot * int(c.split("_")[1]), 2)
                                        for c, k in sorted(mix["mix"].items()) if c.startswith("valu_")}
        out["mix_scope"] = mix["scope"]
        out["code_object"] = {k: mix["code_object"].get(k) for k in ("vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size")}
        if floor_cycles_per_unit:
            out["efficiency"] = round(floor_cycles_per_unit / (per_unit * cpi), 4)          # algorithmic / issued issue-cycles
    for k in ("SQ_WAIT_ANY_frac", "SQ_INSTS_LDS", "SQ_INSTS_SALU", "lds_bank_conflict_frac", "valu_types"):
        if k in entry:
            out[k] = entry[k]
    if entry.get("SQ_LDS_IDX_ACTIVE"):        # LDS-array cycles (PMC, incl. bank conflicts) per CU-cycle of this run: the second resource of these kernels
        out["lds_busy_frac"] = round(entry["SQ_LDS_IDX_ACTIVE"] * (units_per_launch / entry["units_per_launch"]) / (256.0 * (clock or 2400.0) * 1e6 * secs), 4)
    tr = entry.get("hbm_bytes_per_launch")
    out["traffic"] = tr
    if tr is not None:
        scale = units_per_launch / entry["units_per_launch"]
        gbs = tr * scale / secs / 1e9
        out["hbm"] = {"achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(gbs / HBM_PEAK_GBS, 5),
                      "note": "measured HBM bytes (PMC 2*FETCH_SIZE + WRITE_SIZE, separate passes, KB units) / kernel time: HBM is not the bound"}
    return out


# issue cycles (per wave64 instruction and SIMD) of the cheapest instruction for each kind of operation (profiles/r03_issue_rate.txt)
CYC_F64, CYC_CMP, CYC_SEL, CYC_LOGIC, CYC_BFI = 4, 4, 4, 2, 4


def floor_regular_cycles(m, n, cdeg, vdeg):
    """Algorithmic floor of one shot-iteration of the reference loop nest (src/decoding/kernels.py:282-359) on a (cdeg, vdeg)-regular graph, in
    SIMD issue-cycles (lane-operations x cycles of the cheapest instruction / 64 lanes); itemised in DESIGN.md 5.1.  Per edge: q = clip(v - r)
    sub, min, max (3 f64); sign of q folded into a running XOR of high words (1 logic); outgoing message: compare |q| with min1 (1 cmp), select
    a double (2 selects), apply the sign (1 bit-field insert); parity of the hard decisions (1 logic).  Per check: min1 / min2 network
    (14 f64 for degree 6) and two multiplications by alpha.  Per variable: vdeg + 1 additions."""
    per_edge = 3 * CYC_F64 + CYC_LOGIC + CYC_CMP + 2 * CYC_SEL + CYC_BFI + CYC_LOGIC
    two_smallest = {6: 14, 4: 8, 8: 20}[cdeg] * CYC_F64
    per_check = cdeg * per_edge + two_smallest + 2 * CYC_F64
    per_var = (vdeg + 1) * CYC_F64
    return (m * per_check + n * per_var) / 64.0


def floor_first_iteration_cycles(n):
    """Floor of the first-iteration kernel per shot: the Philox4x32-10 stream fixed by mc_common.h -- ceil(n / 4) calls per shot, 10 rounds of two
    32 x 32 -> 64 multiplications (v_mad_u64_u32 / v_mul_hi+lo: 4 cycles each way) and two three-input XORs (2 x 2 cycles), then four threshold
    compares per call; the bit-sliced decode itself is < 15 % on top and not counted."""
    calls = (n + 3) // 4
    return calls * (10 * (2 * 4 + 4 * CYC_LOGIC) + 4 * CYC_CMP) / 64.0


# --------------------------------------------------------------------------------------------------------------------------------
def worker(args):
    import torch
    import torch.distributed as dist
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    from qldpc_amd.data import load_code

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    _lib.require_device()                      # fail loudly: no CPU fallback for the product path
    backend = os.environ.get("QLDPC_BENCH_BACKEND", "nccl")      # "gloo" = rehearsal of the N > 1 path with ranks sharing a GPU
    ndev = torch.cuda.device_count()
    if backend == "nccl" and ndev < world:
        raise SystemExit(f"--gpus {world} but only {ndev} GPU(s) visible (set QLDPC_BENCH_BACKEND=gloo to rehearse with ranks sharing a card)")
    if backend != "nccl":
        local_rank = local_rank % ndev
    torch.cuda.set_device(local_rank)
    rccl_ranks = 1
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
        rccl_ranks = dist.get_world_size()
    coll_dev = "cuda" if backend == "nccl" else "cpu"
    stream = torch.cuda.current_stream().cuda_stream
    T = _lib.TALLY

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def reduce_tally(tally):
        """the one collective of the path; also returns the sum of the per-rank trial counts seen by every rank (a cross-check)"""
        tt = torch.from_numpy(np.ascontiguousarray(tally, np.int64).copy()).to(coll_dev)
        if world > 1:
            dist.all_reduce(tt)
        return tt.cpu().numpy()

    def max_over_ranks(x):
        td = torch.tensor([x], dtype=torch.float64, device=coll_dev)
        if world > 1:
            dist.all_reduce(td, op=dist.ReduceOp.MAX)
        return float(td.item())

    def every_rank(x):
        """[x of rank 0, x of rank 1, ...] on every rank (attribution of a scaling loss: which rank was slow)"""
        if world == 1:
            return [float(x)]
        parts = [torch.zeros(1, dtype=torch.float64, device=coll_dev) for _ in range(world)]
        dist.all_gather(parts, torch.tensor([x], dtype=torch.float64, device=coll_dev))
        return [float(t.item()) for t in parts]

    out = {}
    # ============================================================ code capacity (BASELINE configs 2-4; headline = config 3) ============
    if not args.no_code_capacity:
        code = load_code(args.code)
        label = LABELS.get(args.code, args.code)
        m, n, nnz = code["m"], code["n"], int(code["Hx_indptr"][-1])
        graph = _lib.Graph(code["Hx_indptr"], code["Hx_indices"], n, device=local_rank)
        kflag = {"auto": 0, "resident": _lib.FLAG_KERNEL_RESIDENT, "stream": _lib.FLAG_KERNEL_STREAM}[args.kernel]
        B, K, W = args.batch, args.steps, args.warmup
        b_io = m + n + 8 * n + 5

        leg_extra = {}

        def run_leg(flags, p=None, tag="fixed"):
            p = args.p if p is None else p
            plan = _lib.CodeCapacityPlan(graph, code["Lx"], p, max_iter=args.max_iter, use_osd=True, flags=flags | kflag | _lib.FLAG_CLOCK_PROBE,
                                         batch=B, min_launch=args.min_launch)

            def shot0(step):          # disjoint global shot ranges: step-major, then rank
                return (step * world + rank) * B
            for w in range(W):
                plan.run(SEED + 1, shot0(w), B, stream)
            plan.read(stream, clear=True)
            plan.kernel_time()
            barrier()
            t0 = time.perf_counter()
            for k in range(K):
                plan.run(SEED, shot0(k), B, stream)
            tally = plan.read(stream)             # synchronises the stream
            t_local = time.perf_counter() - t0    # this rank's own time to finish its K steps
            t1 = time.perf_counter()
            total = reduce_tally(tally)           # the one collective of the path (replaces engine.py:450-457)
            t_coll = time.perf_counter() - t1     # includes waiting for the slowest rank
            barrier()
            dt = time.perf_counter() - t0
            leg_extra[tag] = {"per_rank_ms_per_step": [round(x / K * 1e3, 4) for x in every_rank(t_local)],
                              "tally_allreduce_ms": [round(x * 1e3, 4) for x in every_rank(t_coll)]}
            ms_first = plan.first_iteration_time()
            ms_k, launches = plan.kernel_time()
            try:
                clock = plan.clock(stream)
            except _lib.QldpcError:
                clock = 0.0                       # unfused pipeline (irregular graph / forced streaming kernel): no probe
            plan.close()
            return max_over_ranks(dt), total, tally, ms_k, launches, clock, ms_first

        sweep = [float(x) for x in args.p_sweep.split(",") if x] if args.p_sweep else []
        sweep_points = []
        for ps in sweep:                          # BASELINE config 4: one tally and one all-reduce per error rate
            dt_p, tot_p, _, ms_p, nl_p, _, _ = run_leg(_lib.FLAG_FIXED_ITERS, p=ps, tag=f"p={ps:g}")
            sweep_points.append({"p": ps, "value": round(world * K * B / dt_p, 1), "unit": "shots/s", "ms_per_step": round(dt_p / K * 1e3, 4),
                                 "kernel_ms_per_launch": round(ms_p / max(nl_p, 1), 4), "logical_error_rate": round(float(tot_p[T["total_err"]]) / max(1, int(tot_p[T["trials"]])), 8),
                                 "tally": {k: int(tot_p[v]) for k, v in T.items() if k.endswith("_z") or k in ("trials", "total_err")}, **leg_extra[f"p={ps:g}"]})
        dt_fixed, tally_fixed, local_fixed, ms_fixed, nl_fixed, clk_fixed, _ = run_leg(_lib.FLAG_FIXED_ITERS)
        if rank == 0 and args.dump_outputs:
            dump_outputs(args.dump_outputs, {"tally": tally_fixed})       # the plan's running tally after the last timed step
        if args.legs == "fixed":
            dt_ref, tally_ref, ms_ref, nl_ref, clk_ref, ms_first = dt_fixed, tally_fixed, ms_fixed, nl_fixed, clk_fixed, 0.0
        else:
            dt_ref, tally_ref, _, ms_ref, nl_ref, clk_ref, ms_first = run_leg(0, tag="reference_semantics")
            # the timed leg keeps three batches in flight on the plan's own streams, so its per-kernel event spans overlap; the kernel times the roofline
            # prices are taken from a few more batches with the kernels of a batch one after the other (outside the timed region)
            _lib.set_option("mc_tail_overlap", 2)
            try:
                K_saved = K
                K = min(K, 4)
                _, _, _, ms_ref, nl_ref, clk_ref, ms_first = run_leg(0, tag="reference_semantics_exclusive")
            finally:
                K = K_saved
                _lib.set_option("mc_tail_overlap", 1)
        if not np.array_equal(tally_fixed, tally_ref):
            raise SystemExit(f"fixed-work and early-exit legs disagree: {tally_fixed.tolist()} vs {tally_ref.tolist()}")
        shots_total = world * K * B
        if int(tally_fixed[T["trials"]]) != shots_total:
            raise SystemExit(f"tally counts {int(tally_fixed[T['trials']])} shots, expected {shots_total} = {world} ranks x {K} steps x {B}")
        value = shots_total / dt_fixed
        mean_iters = tally_ref[T["iters_z"]] / max(1, tally_ref[T["trials"]])
        bytes_fixed = args.max_iter * 16 * nnz + b_io
        bytes_ref = mean_iters * 16 * nnz + b_io
        regular = {(72, 36): (6, 3), (144, 72): (6, 3), (288, 144): (6, 3), (90, 45): (6, 3), (108, 54): (6, 3)}.get((n, m))
        floor = floor_regular_cycles(m, n, *regular) if regular and args.kernel == "auto" else None

        def hbm_model(bytes_per_shot, ms, launches):
            if launches <= 0 or ms <= 0:
                return None
            ach = bytes_per_shot * B / (ms / launches * 1e-3) / 1e9
            return {"achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "ratio": round(ach / HBM_PEAK_GBS, 4),
                    "algorithmic_bytes_per_shot": round(float(bytes_per_shot), 1),
                    "note": "SURVEY 8d streaming message-passing MODEL bytes / kernel time (the accounting the 1e7 shots/s = 43 % target was "
                            "stated in); the messages are register / LDS resident, so this is not HBM traffic and not a roofline fraction"}

        pm_fixed = pmc_entry(f"cc_{args.code}_fixed") if args.kernel == "auto" else None
        pm_ref = pmc_entry(f"cc_{args.code}_early_exit") if args.kernel == "auto" else None
        mix_fixed = isa_entry(f"cc_{args.code}_fixed") if args.kernel == "auto" else None
        mix_ref = isa_entry(f"cc_{args.code}_early_exit") if args.kernel == "auto" else None
        roof_fixed = issue_roofline(pm_fixed, mix_fixed, B * args.max_iter, ms_fixed / max(nl_fixed, 1), clk_fixed, floor, "shot_iteration")
        if roof_fixed:
            roof_fixed["hbm_model"] = hbm_model(bytes_fixed, ms_fixed, nl_fixed)
        # reference semantics: the dominant kernel is the bit-sliced first iteration (every shot); the full decoder only sees the few shots it lists
        ms_ref_kernel = (ms_first if ms_first > 0 else ms_ref) / max(nl_ref, 1)
        roof_ref = issue_roofline(pm_ref if ms_first > 0 else None, mix_ref, B, ms_ref_kernel, clk_ref, floor_first_iteration_cycles(n), "shot")
        if roof_ref:
            roof_ref["decode_ms_per_launch"] = {"first_iteration_kernel": round(ms_first / max(nl_ref, 1), 4),
                                                "full_decoder_on_listed_shots": round((ms_ref - ms_first) / max(nl_ref, 1), 4)}
            roof_ref["hbm_model"] = hbm_model(bytes_ref, ms_ref, nl_ref)
        out.update({
            "metric": f"decoded shots/sec, {label} p={args.p:g} {args.max_iter} BP iters",
            "value": round(value, 1), "unit": "shots/s", "n_gpus": world, "rccl_ranks": rccl_ranks, "collective_backend": backend if world > 1 else None,
            "steps": K, "warmup": W,
            "ms_per_step": round(dt_fixed / K * 1e3, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": f"{label} Hx {m}x{n} nnz={nnz} code-capacity p={args.p} max_iter={args.max_iter} "
                                   f"dynamic alpha, OSD-0 on BP failures, batch={B} shots/step/GPU, fixed-work mode (all {args.max_iter} "
                                   "iterations executed per shot, outputs frozen at convergence)",
                       "code": args.code, "batch": B, "min_launch": args.min_launch, "mode": "fixed_iters", "kernel": args.kernel, "seed": SEED},
            "roofline": roof_fixed if roof_fixed else {"bound": "valu_issue", "achieved": None, "peak": None, "unit": "G wave-instructions/s", "frac": None,
                                                        "traffic": None, "kernel_ms_per_launch": round(ms_fixed / max(nl_fixed, 1), 4),
                                                        "clock_mhz": round(clk_fixed, 1) if clk_fixed else None,
                                                        "hbm_model": hbm_model(bytes_fixed, ms_fixed, nl_fixed),
                                                        "note": "no current PMC record for this kernel in profiles/pmc.json (none taken, or the kernel source "
                                                                "changed since): instruction counts are not guessed"},
            "reference_semantics": {"value": round(shots_total / dt_ref, 1), "unit": "shots/s", "ms_per_step": round(dt_ref / K * 1e3, 4),
                                    "mean_iterations": round(float(mean_iters), 4),
                                    "roofline": roof_ref if roof_ref else {"kernel_ms_per_launch": round(ms_ref / max(nl_ref, 1), 4),
                                                                           "clock_mhz": round(clk_ref, 1) if clk_ref else None,
                                                                           "hbm_model": hbm_model(bytes_ref, ms_ref, nl_ref)}},
            "tally": {k: int(tally_ref[v]) for k, v in T.items() if k.endswith("_z") or k in ("trials", "total_err")},
            "per_rank": leg_extra.get("fixed"),
        })
        if "reference_semantics" in leg_extra and "reference_semantics" in out:
            out["reference_semantics"]["per_rank"] = leg_extra["reference_semantics"]
        if sweep_points:
            tot_shots = sum(world * K * B for _ in sweep_points)
            tot_time = sum(pt["ms_per_step"] * K / 1e3 for pt in sweep_points)
            out["p_sweep"] = {"points": sweep_points, "value": round(tot_shots / tot_time, 1), "unit": "shots/s",
                              "note": "BASELINE config 4 shape: fixed-work leg per error rate, one tally + one all-reduce per point"}
        if args.legs == "fixed":
            del out["reference_semantics"]

        if rank == 0 and not args.no_cpu_baseline:          # rank 0 alone, after the timed regions (the other ranks wait at the next barrier)
            from oracle import oracle as orc          # the checker / CPU baseline, never the product path
            cores = orc.num_threads()
            probe = 200000        # includes thread start-up; large enough that the rate estimate is meaningful
            orc.cc_sample_decode_tally(code["Hx_indptr"], code["Hx_indices"], n, code["Lx"], args.p, SEED, 0, 20000, max_iter=args.max_iter, threads=0)
            t0 = time.perf_counter()
            orc.cc_sample_decode_tally(code["Hx_indptr"], code["Hx_indices"], n, code["Lx"], args.p, SEED, 0, probe, max_iter=args.max_iter, threads=0)
            rate = probe / (time.perf_counter() - t0)
            sample = int(min(max(K * B, 1), max(probe, rate * args.cpu_seconds)))
            t0 = time.perf_counter()
            t_cpu = orc.cc_sample_decode_tally(code["Hx_indptr"], code["Hx_indices"], n, code["Lx"], args.p, SEED, 0, sample,
                                               max_iter=args.max_iter, threads=0)
            dt_cpu = time.perf_counter() - t0
            # same Philox streams: the GPU tally over the same first `sample` shots must be identical
            t_gpu = _lib.cc_sample_decode_tally(graph, code["Lx"], args.p, SEED, 0, sample, max_iter=args.max_iter, flags=kflag)
            if not np.array_equal(t_cpu, t_gpu):
                raise SystemExit(f"GPU tally != oracle tally on the CPU sample: {t_gpu.tolist()} vs {t_cpu.tolist()}")
            # one host thread on a smaller sample (SURVEY 8d asks for both figures)
            one = int(max(20000, min(sample, rate / max(cores, 1) * 3.0)))
            t0 = time.perf_counter()
            orc.cc_sample_decode_tally(code["Hx_indptr"], code["Hx_indices"], n, code["Lx"], args.p, SEED, 0, one, max_iter=args.max_iter, threads=1)
            dt_one = time.perf_counter() - t0
            out["cpu_baseline"] = {"value": round(sample / dt_cpu, 1), "unit": "shots/s", "cores": cores, "kind": "port",
                                   "sample": f"first {sample} shots of the same Philox stream (seed {SEED}), reference early-exit semantics, "
                                             f"OpenMP over shots on {cores} threads; tally identical to the GPU's",
                                   "single_thread": {"value": round(one / dt_one, 1), "unit": "shots/s", "sample": f"first {one} shots, 1 thread"}}
            # LLR check of the north-star contract on a prefix: decode the syndromes of the first 4096 shots on both sides
            E = np.stack([orc.cc_sample_errors(SEED, i, n, args.p) for i in range(4096)]).astype(np.int8)
            synd = np.stack([orc.syndrome_check(code["Hx_indptr"], code["Hx_indices"], e) for e in E])
            prior = np.full(n, np.log((1.0 - args.p) / args.p))
            g_err, g_conv, g_llr, g_it = _lib.minsum_decode_batch(graph, synd, prior, args.max_iter, "dynamical", 1.0, flags=kflag)
            c_err, c_conv, c_llr, c_it = orc.minsum_decode_batch(code["Hx_indptr"], code["Hx_indices"], n, synd, prior, max_iter=args.max_iter, threads=0)
            diff = float(np.max(np.abs(g_llr - c_llr))) if g_llr.size else 0.0
            if diff > 1e-5 or not (np.array_equal(g_err, c_err) and np.array_equal(g_it, c_it)):
                raise SystemExit(f"LLR check failed: max |llr_gpu - llr_cpu| = {diff}")
            out["llr_check"] = {"shots": 4096, "max_abs_diff": diff, "tolerance": 1e-5, "hard_decisions_and_iterations_identical": True}

    # ============================================================ circuit level (BASELINE config 5) =====================================
    if args.circuit != "none":
        out["circuit_level"] = circuit_leg(args, _lib, rank, world, local_rank, stream, barrier, reduce_tally, max_over_ranks)
        if args.no_code_capacity:
            cl = out["circuit_level"]
            out.update({"metric": cl["metric"], "value": cl["value"], "unit": cl["unit"], "n_gpus": world, "rccl_ranks": rccl_ranks, "steps": cl["steps"],
                        "warmup": cl["warmup"], "ms_per_step": cl["ms_per_step"], "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
                        "dtype": "f64", "data": "synthetic", "config": cl["config"]})
    if rank == 0:
        print(json.dumps(scalars_first(out)), flush=True)
    if world > 1:
        dist.destroy_process_group()


def scalars_first(out):
    """The JSON line with every headline number as a TOP-LEVEL SCALAR ahead of the nested objects, so that a record that keeps only scalars
    (or only the head of the line) still shows config 5, the reference-semantics rate and the roofline fractions."""
    flat = {}
    rf = out.get("roofline") or {}
    flat["roofline_frac"] = rf.get("frac")
    flat["roofline_issued_frac"] = rf.get("issued_frac")
    flat["kernel_ms_per_launch"] = rf.get("kernel_ms_per_launch")
    rs = out.get("reference_semantics") or {}
    flat["ref_semantics_shots_per_s"] = rs.get("value")
    flat["ref_semantics_ms_per_step"] = rs.get("ms_per_step")
    cb = out.get("cpu_baseline") or {}
    flat["cpu_baseline_shots_per_s"] = cb.get("value")
    flat["cpu_baseline_cores"] = cb.get("cores")
    lc = out.get("llr_check") or {}
    flat["llr_max_abs_diff"] = lc.get("max_abs_diff")
    cl = out.get("circuit_level") or {}
    if cl:
        ph = cl.get("phases_ms_per_step") or {}
        flat["circuit_trials_per_s"] = cl.get("value")
        flat["circuit_ms_per_step"] = cl.get("ms_per_step")
        for k in ("sample", "bp_z", "osd_z", "bp_x", "osd_x", "judge"):
            flat[f"circuit_{k}_ms"] = ph.get(k)
        flat["circuit_logical_error_rate"] = cl.get("logical_error_rate")
        cr = cl.get("roofline") or {}
        flat["circuit_bp_frac"] = (cr.get("bp") or {}).get("frac")
        flat["circuit_osd_frac"] = (cr.get("osd") or {}).get("frac")
        flat["circuit_cpu_baseline_trials_per_s"] = (cl.get("cpu_baseline") or {}).get("value")
    for pt in (out.get("p_sweep") or {}).get("points", []):
        tag = f"{pt['p']:g}".replace(".", "p")
        flat[f"p_sweep_{tag}_shots_per_s"] = pt["value"]
        flat[f"p_sweep_{tag}_logical_error_rate"] = pt["logical_error_rate"]
    if out.get("p_sweep"):
        flat["p_sweep_shots_per_s"] = out["p_sweep"]["value"]
    line = {k: v for k, v in out.items() if not isinstance(v, (dict, list))}
    line.update({k: v for k, v in flat.items() if v is not None})
    line.update({k: v for k, v in out.items() if isinstance(v, (dict, list))})
    return line


def circuit_leg(args, _lib, rank, world, local_rank, stream, barrier, reduce_tally, max_over_ranks):
    """BASELINE config 5: per-trial pipeline of src/simulation/engine.py:68-122 on the cached decoding matrices of the reference's own
    [[144,12,12]] x 12-cycle experiment (matrix_cache/matrices_d63ef327adf94be6.npz re-packed as CSR), p = 0.005, max_iter 50, OSD-0."""
    from qldpc_amd.data import load_code, load_circuit_matrices
    from qldpc_amd.codes.bb_code import BBCodeCircuit
    from qldpc_amd.noise.compiled import CompiledCircuit
    from qldpc_amd.simulation.engine import prior_llrs
    T = _lib.TALLY
    d = load_circuit_matrices(args.circuit)
    c = load_code(str(d["code"]))
    cycles = int(d["num_cycles"])
    cb = BBCodeCircuit(c["Hx"], c["Hz"], num_cycles=cycles, ell=c["ell"], m=c["m_dim"], a_x_powers=c["a_x_powers"],
                       a_y_powers=c["a_y_powers"], b_y_powers=c["b_y_powers"], b_x_powers=c["b_x_powers"])
    comp = CompiledCircuit(cb.get_full_circuit(), cb.cycle * 2, cb.lin_order, cb.data_qubits, cb.Xchecks, cb.Zchecks)
    gr, pr, mk, dims = [], [], [], []
    for s in "ZX":
        n = int(d[f"Hdec{s}_shape"][1])
        gr.append(_lib.Graph(d[f"Hdec{s}_indptr"], d[f"Hdec{s}_indices"], n, device=local_rank))
        pr.append(prior_llrs(d[f"channel_probs{s}"]))
        mk.append(_lib.logical_column_masks((d[f"H{s}_logical_indptr"], d[f"H{s}_logical_indices"]), n))
        dims.append((int(d[f"Hdec{s}_shape"][0]), n, int(d[f"Hdec{s}_indptr"][-1])))
    B, K, W = args.circuit_batch, args.circuit_steps, args.circuit_warmup
    p = 0.005
    flags = args.circuit_flags | _lib.FLAG_CLOCK_PROBE
    plan = _lib.CircuitPlan(comp, c["Lx"], c["Lz"], gr[0], gr[1], pr[0], pr[1], mk[0], mk[1], p, max_iter=args.max_iter, use_osd=True, flags=flags, batch=B)

    def trial0(step):
        return (step * world + rank) * B
    for w in range(W):
        plan.run(SEED + 1, trial0(w), B, stream)
    plan.read(stream, clear=True)
    plan.phase_times()
    barrier()
    t0 = time.perf_counter()
    for k in range(K):
        plan.run(SEED, trial0(k), B, stream)
    tally = plan.read(stream)
    total = reduce_tally(tally)
    barrier()
    dt = max_over_ranks(time.perf_counter() - t0)
    phases, nb = plan.phase_times()        # both sectors run on the caller's stream: the hipEvent spans are exclusive and sum to the step
    if rank == 0 and args.dump_outputs and args.no_code_capacity:          # this leg is the headline
        dump_outputs(args.dump_outputs, {"tally": total})
    solo_tally = tally
    clk_bp, clk_osd = plan.clock(stream)
    trials = world * K * B
    if int(total[T["trials"]]) != trials:
        raise SystemExit(f"circuit tally counts {int(total[T['trials']])} trials, expected {trials}")
    label = LABELS.get(str(d["code"]), str(d["code"]))
    mean_it = (total[T["iters_z"]] + total[T["iters_x"]]) / max(1, 2 * trials)
    model_bytes = sum(mean_it * 16 * nnz + m + 9 * n + 5 for (m, n, nnz) in dims)
    res = {
        "metric": f"decoded trials/sec, {label} circuit-level noise, {cycles}+2 cycles, p={p:g}, {args.max_iter} BP iters, OSD-0",
        "value": round(trials / dt, 1), "unit": "trials/s", "steps": K, "warmup": W, "ms_per_step": round(dt / K * 1e3, 3),
        "config": {"workload": f"{label} x {cycles} noisy + 2 noiseless cycles, HdecZ {dims[0][0]}x{dims[0][1]} nnz={dims[0][2]}, HdecX {dims[1][0]}x{dims[1][1]} "
                               f"nnz={dims[1][2]}, p={p}, max_iter={args.max_iter}, dynamic alpha, one trial = sample + decode Z + OSD-0 + decode X + OSD-0 + "
                               f"logical comparison (reference early-exit semantics), batch={B} trials/step/GPU",
                   "matrices": args.circuit, "batch": B, "seed": SEED, "flags": args.circuit_flags},
        "phases_ms_per_step": {k: round(v / max(nb, 1), 3) for k, v in phases.items()},
        "phases_note": "hipEvent spans of the timed steps, mean per step (one stream: exclusive times that sum to the step)",
        "logical_error_rate": round(float(total[T["total_err"]]) / trials, 4),
        "bp_converged": {"z": round(float(total[T["bp_conv_z"]]) / trials, 4), "x": round(float(total[T["bp_conv_x"]]) / trials, 4)},
        "mean_iterations": round(float(mean_it), 2),
        "tally": {k: int(total[v]) for k, v in T.items()},
        "clock_mhz": {"bp": round(clk_bp, 1), "osd": round(clk_osd, 1)},
        "hbm_model": {"bytes_per_trial": round(float(model_bytes), 1), "achieved": round(model_bytes * trials / dt / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                      "ratio": round(model_bytes * trials / dt / 1e9 / HBM_PEAK_GBS / world, 4),
                      "note": "SURVEY 8d streaming MODEL bytes (16 nnz per executed iteration + I/O, both sectors) x trials/s per GPU; the decoder keeps its state "
                              "in LDS, so this is the model the north-star 40 % was stated in, not measured traffic"},
    }
    # binding-resource objects of the two dominant kernels, from the committed PMC records (refused when the kernel source changed)
    it_sum = float(solo_tally[T["iters_z"]] + solo_tally[T["iters_x"]])
    pm_bp, pm_osd = pmc_entry(f"{args.circuit}_bp"), pmc_entry(f"{args.circuit}_osd")
    bp_ms = (phases["bp_z"] + phases["bp_x"]) / max(2 * nb, 1)
    osd_ms = (phases["osd_z"] + phases["osd_x"]) / max(2 * nb, 1)
    osd_shots = float(solo_tally[T["osd_z"]] + solo_tally[T["osd_x"]])
    res["roofline"] = {
        "bp": issue_roofline(pm_bp, isa_entry(f"{args.circuit}_bp"), it_sum / max(2 * nb, 1), bp_ms, clk_bp,
                             pm_bp.get("floor_issue_cycles_per_unit") if pm_bp else None, "decode_iteration"),
        "osd": issue_roofline(pm_osd, isa_entry(f"{args.circuit}_osd"), osd_shots / max(2 * nb, 1), osd_ms, clk_osd,
                              pm_osd.get("floor_issue_cycles_per_unit") if pm_osd else None, "osd_shot"),
        "note": "per launch of one sector, from the exclusive (one-stream) batch",
    }
    if rank == 0 and not args.no_cpu_baseline:
        from oracle import oracle as orc            # CPU checker, timed beside the GPU path (never part of it)
        circ = orc.make_circuit(comp, c["Lx"], c["Lz"])
        secs = [orc.make_sector(d[f"Hdec{s}_indptr"], d[f"Hdec{s}_indices"], int(d[f"Hdec{s}_shape"][1]), orc.prior_llrs(d[f"channel_probs{s}"]),
                                d[f"H{s}_logical_indptr"], d[f"H{s}_logical_indices"]) for s in "ZX"]
        cores = orc.num_threads()
        probe = max(64, 2 * cores)
        t0 = time.perf_counter()
        orc.circuit_sample_decode_tally(circ, secs[0], secs[1], p, SEED, 0, probe, max_iter=args.max_iter, use_osd=True, threads=0)
        rate = probe / (time.perf_counter() - t0)
        sample = int(min(K * B, max(probe, rate * args.cpu_seconds)))
        t0 = time.perf_counter()
        ref = orc.circuit_sample_decode_tally(circ, secs[0], secs[1], p, SEED, 0, sample, max_iter=args.max_iter, use_osd=True, threads=0)
        dt_cpu = time.perf_counter() - t0
        chk = _lib.CircuitPlan(comp, c["Lx"], c["Lz"], gr[0], gr[1], pr[0], pr[1], mk[0], mk[1], p, max_iter=args.max_iter, use_osd=True,
                               flags=args.circuit_flags, batch=B)
        chk.run(SEED, 0, sample)
        got = chk.read()
        chk.close()
        if not np.array_equal(got, ref):
            raise SystemExit(f"circuit level: GPU tally != oracle tally on the CPU sample: {got.tolist()} vs {ref.tolist()}")
        res["cpu_baseline"] = {"value": round(sample / dt_cpu, 1), "unit": "trials/s", "cores": cores, "kind": "port",
                               "sample": f"first {sample} trials of the same Philox stream (seed {SEED}): C port of the reference per-trial loop "
                                         f"(literal circuit simulation, min-sum with early exit, packed Gauss-Jordan OSD-0), OpenMP over trials on {cores} "
                                         "threads; tally identical to the GPU's"}
    plan.close()
    return res


def main():
    args = parse_args()
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(launch_ranks(args))       # nothing above this line has touched the GPU
    worker(args)


if __name__ == "__main__":
    main()
