#!/usr/bin/env python3
"""Generate the golden vectors under tests/golden/ by running the REFERENCE'S OWN SOURCE.

Container-only tool.  /root/reference does not exist on the GPU box and nothing in the
test-suite, smoke() or bench.py imports this file.  It executes the reference's Python
functions (src/decoding/*, src/noise/*, src/codes/*) under CPython with
tools/refshim/numba (identity ``@njit``; numba itself is not installable here), i.e. the
strict IEEE-754 reading of the reference source.  Every fixture stores its inputs
explicitly (graphs, syndromes, priors, random arrays) together with the outputs the
reference produced, so the other side never re-derives anything from a NumPy seed.

Usage (from anywhere):  python3 tests/golden/make_golden.py [--only NAME]

Also re-packs the reference's *data files* (codes/*.npz, two matrix_cache/*.npz) into
compact CSR/bit form under qldpc-branched-off_amd/data/ (data, not source).
"""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.join(REPO, "tools", "refshim"))
sys.path.insert(0, REF)

from scipy.sparse import csr_matrix  # noqa: E402

from src.decoding import kernels as K  # noqa: E402
from src.decoding.sparse import performMinSum_Symmetric_Sparse  # noqa: E402
from src.decoding.dense import performMinSum_Symmetric, performBeliefPropagationFast  # noqa: E402
from src.decoding import osd as OSD  # noqa: E402
from src.codes.bb_code import BBCodeCircuit  # noqa: E402
from src.noise.compiled import CompiledCircuit  # noqa: E402
from src.noise import kernels as NK  # noqa: E402
from src.noise.simulation import run_trial_fast  # noqa: E402
from src.decoding import alpha as ALPHA  # noqa: E402
from src.decoding import scopt as SCOPT  # noqa: E402

DATA = os.path.join(REPO, "qldpc-branched-off_amd", "data")
CODES = {
    "bb72": "codes/[[72, 12, 6]].npz",
    "bb144": "codes/[[144, 12, 12]].npz",
    "bb288": "codes/[[288, 12, 18]].npz",
    "bb90": "codes/[[90, 8, 10]].npz",
    "bb108": "codes/[[108, 8, 10]].npz",
}
CACHE = {
    "circ72": ("matrix_cache/matrices_61d7ee9cf7e4c9ee.npz", "bb72", 6, 0.005),
    "circ144": ("matrix_cache/matrices_d63ef327adf94be6.npz", "bb144", 12, 0.005),
    # the reference's cached decoding matrices of its other experiments (main.py: num_cycles = distance), builder parity only
    "circ90": ("matrix_cache/matrices_982970e639ed188c.npz", "bb90", 10, 0.005),
    "circ108": ("matrix_cache/matrices_a7240995d9aa0955.npz", "bb108", 10, 0.005),
    "circ288": ("matrix_cache/matrices_6c6f54237b5d8525.npz", "bb288", 18, 0.005),
}


def save(name, **arrs):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrs)
    print(f"  wrote {name}.npz  {os.path.getsize(path) / 1024:.1f} KiB")


def save_fixed(name, **arrs):
    """save() with fixed zip member times, so that a rerun of the generator writes byte-identical files (np.savez stamps the current time)."""
    import io
    import zipfile
    path = os.path.join(HERE, name + ".npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k, v in arrs.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())
    print(f"  wrote {name}.npz  {os.path.getsize(path) / 1024:.1f} KiB")


def csr_of(H):
    c = csr_matrix(np.asarray(H))
    c.sort_indices()
    return c


def load_code(tag):
    d = np.load(os.path.join(REF, CODES[tag]))
    return {k: d[k] for k in d.files}


# --------------------------------------------------------------------------- data re-pack
def pack_data():
    os.makedirs(DATA, exist_ok=True)
    out = {}
    st = np.load(os.path.join(REF, "codes/steane.npz"))
    out["steane_Hx"] = st["Hx"].astype(np.uint8)
    out["steane_Hz"] = st["Hz"].astype(np.uint8)
    for tag in CODES:
        d = load_code(tag)
        for k in ("Hx", "Hz", "Lx", "Lz"):
            out[f"{tag}_{k}"] = d[k].astype(np.uint8)
        out[f"{tag}_params"] = np.array([int(d["ell"]), int(d["m"]), int(d["distance"])], dtype=np.int64)
        for k in ("a_x_powers", "a_y_powers", "b_y_powers", "b_x_powers"):
            out[f"{tag}_{k}"] = d[k].astype(np.int64)
    np.savez_compressed(os.path.join(DATA, "codes.npz"), **out)
    print("  wrote data/codes.npz")
    for tag, (path, code, cycles, p) in CACHE.items():
        d = np.load(os.path.join(REF, path))
        o = {"num_cycles": np.int64(cycles), "error_rate": np.float64(p),
             "k": np.int64(d["k"][0]), "code": np.array(code)}
        for s in ("Z", "X"):
            Hd = csr_of(d[f"Hdec{s}"])
            flr = int(d[f"first_logical_row{s}"][0])
            k = int(d["k"][0])
            Hl = csr_of(d[f"H{s}_full"][flr:flr + k])
            o[f"Hdec{s}_shape"] = np.array(Hd.shape, dtype=np.int64)
            o[f"Hdec{s}_indptr"] = Hd.indptr.astype(np.int32)
            o[f"Hdec{s}_indices"] = Hd.indices.astype(np.int32)
            o[f"H{s}_logical_indptr"] = Hl.indptr.astype(np.int32)
            o[f"H{s}_logical_indices"] = Hl.indices.astype(np.int32)
            o[f"channel_probs{s}"] = d[f"channel_probs{s}"].astype(np.float64)
        np.savez_compressed(os.path.join(DATA, f"{tag}_p005.npz"), **o)
        print(f"  wrote data/{tag}_p005.npz")


# --------------------------------------------------------------------------- a1 / a2
def run_sparse(Hc, synd, prior, **kw):
    e, c, v, it = performMinSum_Symmetric_Sparse(Hc, synd, prior, **kw)
    return np.asarray(e, np.int8), bool(c), np.asarray(v, np.float64), int(it)


def batch_sparse(Hc, synds, prior, **kw):
    E, C, V, I = [], [], [], []
    for s in synds:
        e, c, v, it = run_sparse(Hc, s, prior, **kw)
        E.append(e); C.append(c); V.append(v); I.append(it)
    return (np.array(E, np.int8), np.array(C, np.uint8), np.array(V, np.float64), np.array(I, np.int32))


def gen_steane():
    H = np.load(os.path.join(REF, "codes/steane.npz"))["Hx"]
    Hc = csr_of(H)
    prior = np.full(7, np.log((1 - 0.01) / 0.01))
    synds = np.array([[(s >> b) & 1 for b in range(3)] for s in range(8)], dtype=np.int8)
    out = dict(indptr=Hc.indptr.astype(np.int32), indices=Hc.indices.astype(np.int32),
               m=np.int64(3), n=np.int64(7), prior=prior, syndromes=synds, max_iter=np.int64(10))
    modes = {
        "dyn": dict(alpha=1.0, alpha_mode="dynamical"),
        "const": dict(alpha=0.8, alpha_mode="alvarado"),
        "seq": dict(alpha=np.array([0.5, 0.7, 0.9]), alpha_mode="alvarado-autoregressive"),
        "none0": dict(alpha=0, alpha_mode=None),      # None + alpha==0 -> dynamic
        "none1": dict(alpha=0.9, alpha_mode=None),    # None + alpha!=0 -> constant
    }
    for tag, kw in modes.items():
        E, C, V, I = batch_sparse(Hc, synds, prior, maxIter=10, **kw)
        out[f"{tag}_err"], out[f"{tag}_conv"], out[f"{tag}_llr"], out[f"{tag}_iter"] = E, C, V, I
    out["seq_alpha"] = np.array([0.5, 0.7, 0.9])
    # non-uniform prior incl. a negative and a zero entry
    prior2 = np.array([2.0, -0.5, 0.0, 3.25, 1.0, 4.0, 0.125])
    E, C, V, I = batch_sparse(Hc, synds, prior2, maxIter=10, alpha=1.0, alpha_mode="dynamical")
    out["prior2"] = prior2
    out["p2_err"], out["p2_conv"], out["p2_llr"], out["p2_iter"] = E, C, V, I
    save("steane_minsum", **out)


def gen_bb(tag, nsyn, rng):
    d = load_code(tag)
    out = {}
    for hname in ("Hx", "Hz"):
        H = d[hname]
        Hc = csr_of(H)
        m, n = H.shape
        out[f"{hname}_indptr"] = Hc.indptr.astype(np.int32)
        out[f"{hname}_indices"] = Hc.indices.astype(np.int32)
        out[f"{hname}_shape"] = np.array([m, n], np.int64)
        for p in (0.005, 0.03, 0.08):
            ptag = f"{hname}_p{int(round(p * 1000)):03d}"
            errs = (rng.random((nsyn, n)) < p).astype(np.int8)
            synds = (errs @ H.T % 2).astype(np.int8)          # law of alpha.py:127-128
            prior = np.full(n, np.log((1 - p) / p))
            out[f"{ptag}_errors"] = errs
            out[f"{ptag}_syndromes"] = synds
            out[f"{ptag}_prior"] = prior
            for mi in (1, 5, 50):
                E, C, V, I = batch_sparse(Hc, synds, prior, maxIter=mi, alpha=1.0, alpha_mode="dynamical")
                k = f"{ptag}_dyn_it{mi}"
                out[k + "_err"], out[k + "_conv"], out[k + "_llr"], out[k + "_iter"] = E, C, V, I
            if hname == "Hx":
                variants = {
                    "const": dict(alpha=0.8, alpha_mode="alvarado"),
                    "seq": dict(alpha=np.array([0.6, 0.7, 0.8, 0.9, 0.95]), alpha_mode="alvarado-autoregressive"),
                    "damp": dict(alpha=1.0, alpha_mode="dynamical", damping=0.7),
                    "clip5": dict(alpha=1.0, alpha_mode="dynamical", clip_llr=5.0),
                    "dampclip": dict(alpha=0.9, alpha_mode="alvarado", damping=0.5, clip_llr=6.0),
                }
                for vtag, kw in variants.items():
                    E, C, V, I = batch_sparse(Hc, synds, prior, maxIter=30, **kw)
                    k = f"{ptag}_{vtag}"
                    out[k + "_err"], out[k + "_conv"], out[k + "_llr"], out[k + "_iter"] = E, C, V, I
    out["seq_alpha"] = np.array([0.6, 0.7, 0.8, 0.9, 0.95])
    save(f"{tag}_minsum", **out)


# --------------------------------------------------------------------------- a3 a4 a5 a6
def gen_core():
    rng = np.random.default_rng(20260301)
    d = load_code("bb72")
    H = d["Hx"]
    Hc = csr_of(H)
    m, n = H.shape
    nnz = Hc.nnz
    out = dict(indptr=Hc.indptr.astype(np.int32), indices=Hc.indices.astype(np.int32), shape=np.array([m, n], np.int64))
    Q = rng.normal(0, 4, size=(6, nnz))
    Q[1, :10] = 0.0                       # exact zeros (sign convention val>=0 -> +1)
    Q[2, 5] = -0.0                        # negative zero counts as >= 0
    Q[3, 7:9] = Q[3, 6]                   # duplicated magnitude inside one row (tie -> first wins)
    Q[4, 0:6] = np.array([1.5, -1.5, 1.5, 2.0, -1.5, 9.0])
    Q[5, 3] = np.inf
    ssign = np.where(rng.random((6, m)) < 0.3, -1.0, 1.0)
    alphas = np.array([1.0, 0.5, 0.75, 0.8, 0.9375, 0.3])
    Rf, Rs, Rd = [], [], []
    Hd = H.astype(np.float64)
    mask = Hd != 0
    for t in range(6):
        r, s = K.minsum_core_sparse(Hc.data.astype(np.int8), Hc.indices.astype(np.int32), Hc.indptr.astype(np.int32),
                                    Q[t].copy(), ssign[t].copy(), float(alphas[t]), m, n)
        Rf.append(r); Rs.append(s)
        Qd = np.zeros((m, n)); Qd[mask] = Q[t]          # row-major fill == CSR order
        Rd.append(K.minsum_core(Hd, Qd, ssign[t].reshape(-1, 1).copy(), mask, float(alphas[t])))
    out.update(Q=Q, syndrome_sign=ssign, alphas=alphas, R_flat=np.array(Rf), R_sum=np.array(Rs), R_dense=np.array(Rd))
    # a5: bp_core single pass + driver runs
    Qb = rng.normal(0, 2, size=(3, nnz))
    Qb[1, :4] = 0.0
    Qb[2, :6] = np.array([40.0, -38.0, 1e-20, 3.0, -2.0, 0.5])
    Rb = []
    for t in range(3):
        Qd = np.zeros((m, n)); Qd[mask] = Qb[t]
        Rb.append(K.bp_core(Hd, Qd, ssign[t].reshape(-1, 1).copy(), mask, 0.9999999))
    out.update(bp_Q=Qb, bp_R_dense=np.array(Rb))
    p = 0.03
    errs = (rng.random((24, n)) < p).astype(np.int8)
    synds = (errs @ H.T % 2).astype(np.int8)
    prior = np.full(n, np.log((1 - p) / p))
    E, C, V, I = [], [], [], []
    for s in synds:
        e, c, v, it = performBeliefPropagationFast(Hd, s, prior, maxIter=12)
        E.append(np.asarray(e, np.int8)); C.append(bool(c)); V.append(v); I.append(int(it))
    out.update(bpdrv_syndromes=synds, bpdrv_prior=prior, bpdrv_err=np.array(E, np.int8),
               bpdrv_conv=np.array(C, np.uint8), bpdrv_llr=np.array(V), bpdrv_iter=np.array(I, np.int32))
    # a4 driver: dense entry point incl. alpha_estimation
    E, C, V, I = [], [], [], []
    for s in synds:
        e, c, v, it = performMinSum_Symmetric(Hd, s, prior, maxIter=12)
        E.append(np.asarray(e, np.int8)); C.append(bool(c)); V.append(v); I.append(int(it))
    out.update(dense_err=np.array(E, np.int8), dense_conv=np.array(C, np.uint8), dense_llr=np.array(V),
               dense_iter=np.array(I, np.int32))
    e, c, v, it = performMinSum_Symmetric(Hd, synds[3], prior, maxIter=12, alpha_estimation=True)
    out.update(alphaest_R=np.asarray(v, np.float64), alphaest_iter=np.int64(it), alphaest_conv=np.uint8(c))
    # a6 syndrome_check
    cand = (rng.random((8, n)) < 0.2).astype(np.int8)
    sc = np.array([K.syndrome_check(Hc.data.astype(np.int8), Hc.indices.astype(np.int32), Hc.indptr.astype(np.int32), c_, m)
                   for c_ in cand], np.int8)
    out.update(sc_candidates=cand, sc_syndromes=sc)
    save("core_passes", **out)


# --------------------------------------------------------------------------- a7 a8
def gen_gf2():
    rng = np.random.default_rng(77)
    out = {}
    cases = {
        "r20x70": (rng.random((20, 70)) < 0.3),
        "r64x64": (rng.random((64, 64)) < 0.5),
        "r65x129": (rng.random((65, 129)) < 0.2),
        "r70x20": (rng.random((70, 20)) < 0.4),
        "r33x64": (rng.random((33, 64)) < 0.1),
        "zeros": np.zeros((5, 9), bool),
        "ident": np.eye(12, 17, dtype=bool),
    }
    A = (rng.random((30, 90)) < 0.3)
    A[10:20] = A[0:10] ^ A[20:30]               # rank deficient
    cases["rankdef"] = A
    for tag, A in cases.items():
        A = A.astype(np.int64)
        b = (rng.random(A.shape[0]) < 0.5).astype(np.int64)
        Aw, bw = A.copy(), b.copy()
        Ar, br, pr, pc = K.gf2_elimination(Aw, bw)
        Aw2, bw2 = A.copy(), b.copy()
        Ap, bp, pr2, pc2 = K.gf2_elimination_packed(Aw2, bw2)
        assert np.array_equal(br, bp) and np.array_equal(pr, pr2) and np.array_equal(pc, pc2)
        out[f"{tag}_A"] = A.astype(np.uint8); out[f"{tag}_b"] = b.astype(np.uint8)
        out[f"{tag}_A_red"] = np.asarray(Ar).astype(np.uint8); out[f"{tag}_b_red"] = np.asarray(br).astype(np.uint8)
        out[f"{tag}_A_packed_red"] = np.asarray(Ap, dtype=np.uint64)
        out[f"{tag}_pivot_rows"] = np.asarray(pr, np.int64); out[f"{tag}_pivot_cols"] = np.asarray(pc, np.int64)
    out["cases"] = np.array(list(cases.keys()))
    save("gf2_elimination", **out)


def gen_bb256():
    """SURVEY 8c asked for >= 256 sampled syndromes per (code, p) point: Hx of the three headline codes at p = 0.005 / 0.02 / 0.05, full
    decoder defaults (maxIter 50, dynamic alpha).  Bit arrays are stored packed, the posteriors in full."""
    rng = np.random.default_rng(20260901)
    out = {}
    for tag in ("bb72", "bb144", "bb288"):
        d = load_code(tag)
        H = d["Hx"]
        Hc = csr_of(H)
        m, n = H.shape
        out[f"{tag}_shape"] = np.array([m, n], np.int64)
        for p in (0.005, 0.02, 0.05):
            ptag = f"{tag}_p{int(round(p * 1000)):03d}"
            errs = (rng.random((256, n)) < p).astype(np.int8)
            synds = (errs @ H.T % 2).astype(np.int8)
            prior = np.full(n, np.log((1 - p) / p))
            E, C, V, I = batch_sparse(Hc, synds, prior, maxIter=50, alpha=1.0, alpha_mode="dynamical")
            out[f"{ptag}_errors"] = np.packbits(errs.astype(np.uint8), axis=1, bitorder="little")
            out[f"{ptag}_hard"] = np.packbits(E.astype(np.uint8), axis=1, bitorder="little")
            out[f"{ptag}_conv"], out[f"{ptag}_llr"], out[f"{ptag}_iter"] = C, V, I
            print(f"    {ptag}: converged {int(C.sum())}/256, mean iterations {float(I.mean() + 1):.2f}")
    save("bb_256", **out)


def gen_gf2_big():
    """The production-size elimination SURVEY 8c asked for: HdecZ of the [[144,12,12]] x 12-cycle experiment (1008 x 8785) with its
    columns in the |llr| order of a non-converged golden decode, through gf2_elimination_packed (kernels.py:48-106), in place.
    Inputs are reproducible from shipped data: H = data/circ144_p005.npz, the column order and right-hand side stored here."""
    g = np.load(os.path.join(HERE, "circ144_decode.npz"))
    path, code, cycles, p = CACHE["circ144"]
    M = np.load(os.path.join(REF, path))
    H = np.asarray(M["HdecZ"]).astype(np.int64)
    case = int(g["Z_osd_cases"][0])
    order = np.asarray(g["Z_osd_ordering"][0], np.int64)
    hard = np.asarray(g["Z_err"][case], np.int64)
    synd = np.asarray(g["Z_syndromes"][case], np.int64)
    b = (synd + H @ hard) % 2                                       # osd.py:8-9
    A = H[:, order].astype(np.int64)                                # osd.py:13-15
    t0 = time.time()
    Ap, br, pr, pc = K.gf2_elimination_packed(A, b.copy())
    print(f"    1008 x 8785 elimination in pure Python: {time.time() - t0:.0f}s, rank {len(pr)}")
    save("gf2_big", ordering=order.astype(np.int32), b=b.astype(np.uint8), A_packed_red=np.asarray(Ap, np.uint64), b_red=np.asarray(br).astype(np.uint8),
         pivot_rows=np.asarray(pr, np.int64), pivot_cols=np.asarray(pc, np.int64), case=np.int64(case))


# --------------------------------------------------------------------------- circuit level
def build_circuit(tag):
    path, code, cycles, p = CACHE[tag]
    d = load_code(code)
    bb = {k: d[k] for k in ("ell", "m", "a_x_powers", "a_y_powers", "b_y_powers", "b_x_powers")}
    bb["ell"] = int(bb["ell"]); bb["m"] = int(bb["m"])
    cb = BBCodeCircuit(d["Hx"], d["Hz"], num_cycles=cycles, **bb)
    comp = CompiledCircuit(base_circuit=cb.get_full_circuit(), noiseless_suffix=cb.cycle * 2,
                           lin_order=cb.lin_order, data_qubits=cb.data_qubits, Xchecks=cb.Xchecks, Zchecks=cb.Zchecks)
    return d, cb, comp


def gen_noise(tag, ndraw):
    """a10-a13: op arrays + explicit randoms -> noisy circuit, histories, sparse syndromes, logicals."""
    path, code, cycles, _ = CACHE[tag]
    d, cb, comp = build_circuit(tag)
    Lx, Lz = d["Lx"], d["Lz"]
    out = dict(
        base_ops=comp.base_ops, base_q1=comp.base_q1, base_q2=comp.base_q2,
        suffix_ops=comp.suffix_ops, suffix_q1=comp.suffix_q1, suffix_q2=comp.suffix_q2,
        total_qubits=np.int64(comp.total_qubits), num_error_locs=np.int64(comp.num_error_locs),
        max_circuit_size=np.int64(comp.max_circuit_size),
        x_syn_positions=comp.x_syn_positions, x_syn_ptrs=comp.x_syn_ptrs,
        z_syn_positions=comp.z_syn_positions, z_syn_ptrs=comp.z_syn_ptrs,
        x_check_indices=comp.x_check_indices, x_check_ptrs=comp.x_check_ptrs,
        z_check_indices=comp.z_check_indices, z_check_ptrs=comp.z_check_ptrs,
        data_qubit_indices=comp.data_qubit_indices,
        max_syndromes_x=np.int64(comp.max_syndromes_x), max_syndromes_z=np.int64(comp.max_syndromes_z),
        num_x_checks=np.int64(comp.num_x_checks), num_z_checks=np.int64(comp.num_z_checks),
        Lx=Lx.astype(np.uint8), Lz=Lz.astype(np.uint8), num_cycles=np.int64(cycles),
    )
    n_locs = comp.num_error_locs
    ps = [0.005] * (ndraw // 2) + [0.05] * (ndraw - ndraw // 2)
    rv, rp, rt = [], [], []
    nlen, nops, nq1, nq2 = [], [], [], []
    hz, sz, hx, sx = [], [], [], []
    spz, tz, spx, tx = [], [], [], []
    cnt = []
    for t, p in enumerate(ps):
        np.random.seed(9000 + t)
        # same draw order as noise/simulation.py:43-45
        a = np.random.random(n_locs)
        b = np.random.randint(0, 3, n_locs, dtype=np.int32)
        c = np.random.randint(0, 15, n_locs, dtype=np.int32)
        rv.append(a); rp.append(b); rt.append(c)
        L = NK.generate_noisy_circuit_jit(comp.base_ops, comp.base_q1, comp.base_q2, p, a, b, c,
                                          comp.out_ops, comp.out_q1, comp.out_q2)
        nlen.append(L)
        pad = comp.max_circuit_size
        o = np.zeros(pad, np.int32); o[:L] = comp.out_ops[:L]; nops.append(o)
        o = np.zeros(pad, np.int32); o[:L] = comp.out_q1[:L]; nq1.append(o)
        o = np.zeros(pad, np.int32); o[:L] = comp.out_q2[:L]; nq2.append(o)
        full_ops = np.concatenate([comp.out_ops[:L], comp.suffix_ops]).astype(np.int32)
        full_q1 = np.concatenate([comp.out_q1[:L], comp.suffix_q1]).astype(np.int32)
        full_q2 = np.concatenate([comp.out_q2[:L], comp.suffix_q2]).astype(np.int32)
        h, s, nc, ne = NK.simulate_circuit_Z_jit(full_ops, full_q1, full_q2, comp.total_qubits,
                                                 comp.x_check_indices, comp.x_check_ptrs, comp.max_syndromes_x)
        hz.append(h.copy()); sz.append(s.copy()); cz = (nc, ne)
        h2, s2, nc2, ne2 = NK.simulate_circuit_X_jit(full_ops, full_q1, full_q2, comp.total_qubits,
                                                     comp.z_check_indices, comp.z_check_ptrs, comp.max_syndromes_z)
        hx.append(h2.copy()); sx.append(s2.copy())
        cnt.append([cz[0], cz[1], nc2, ne2])
        # the composed trial, re-seeded so run_trial_fast draws the very same arrays
        np.random.seed(9000 + t)
        a_, b_, c_, d_ = run_trial_fast(comp, p, Lx, Lz)
        spz.append(np.asarray(a_, np.int8)); tz.append(np.asarray(b_, np.int8))
        spx.append(np.asarray(c_, np.int8)); tx.append(np.asarray(d_, np.int8))
        # cross-check pieces against the composed call
        assert np.array_equal(NK.sparsify_syndrome_jit(h, nc, comp.x_syn_positions, comp.x_syn_ptrs, comp.num_x_checks), a_)
        assert np.array_equal((Lx @ NK.extract_data_state_jit(s, comp.data_qubit_indices)) % 2, b_)
    out.update(error_rates=np.array(ps), random_vals=np.array(rv), random_paulis=np.array(rp, np.int32),
               random_two_qubit=np.array(rt, np.int32), noisy_len=np.array(nlen, np.int64),
               noisy_ops=np.array(nops, np.int32), noisy_q1=np.array(nq1, np.int32), noisy_q2=np.array(nq2, np.int32),
               hist_z=np.array(hz, np.int8), state_z=np.array(sz, np.int8), hist_x=np.array(hx, np.int8),
               state_x=np.array(sx, np.int8), counts=np.array(cnt, np.int64),
               sparse_z=np.array(spz, np.int8), true_z=np.array(tz, np.int8),
               sparse_x=np.array(spx, np.int8), true_x=np.array(tx, np.int8))
    save(f"{tag}_noise", **out)
    return out


def prior_llrs(probs):
    with np.errstate(divide="ignore", invalid="ignore"):        # engine.py:210-212
        return np.clip(np.nan_to_num(np.log((1 - probs) / probs)), -50, 50)


def gen_circuit_decode(tag, noise, ndec, n_osd, max_iter, extra=0):
    """a1 on the circuit-level graphs + a9 OSD-0 (and the np.argsort order it used) + a15 priors.
    `extra` more syndrome pairs come from further run_trial_fast draws at p = 0.005 (seeds 9500 + t; only the syndromes are kept)."""
    path, code, cycles, _ = CACHE[tag]
    m = np.load(os.path.join(REF, path))
    out = {}
    sel = [i for i in range(len(noise["error_rates"])) if noise["error_rates"][i] == 0.005][:ndec]
    more = {"sparse_z": [], "sparse_x": []}
    if extra:
        d, cb, comp = build_circuit(tag)
        for t in range(extra):
            np.random.seed(9500 + t)
            a_, b_, c_, d_ = run_trial_fast(comp, 0.005, d["Lx"], d["Lz"])
            more["sparse_z"].append(np.asarray(a_, np.int8)); more["sparse_x"].append(np.asarray(c_, np.int8))
    for s, spk in (("Z", "sparse_z"), ("X", "sparse_x")):
        Hd = m[f"Hdec{s}"]
        Hc = csr_of(Hd)
        llr = prior_llrs(m[f"channel_probs{s}"])
        out[f"llrs_{s}"] = llr
        synds = noise[spk][sel]
        if extra:
            synds = np.concatenate([synds, np.array(more[spk], np.int8)])
        t0 = time.time()
        E, C, V, I = batch_sparse(Hc, synds, llr, maxIter=max_iter, alpha=1.0, alpha_mode="dynamical")
        print(f"    {tag} {s}: {len(synds)} decodes in {time.time() - t0:.1f}s conv={C.tolist()} iters={I.tolist()}")
        out[f"{s}_syndromes"] = synds.astype(np.int8)
        out[f"{s}_err"], out[f"{s}_conv"], out[f"{s}_llr"], out[f"{s}_iter"] = E, C, V, I
        # OSD-0 on the first n_osd non-converged decodes (reference call: engine.py:96-97, osd.py:5-29)
        fails = [i for i in range(len(synds)) if not C[i]][:n_osd]
        Hf = np.asarray(Hd, dtype=np.float64)
        sols, orders = [], []
        real_argsort = np.argsort
        for i in fails:
            cap = {}

            def spy(a, *aa, **kk):
                r = real_argsort(a, *aa, **kk)
                cap.setdefault("o", r.copy())
                return r
            OSD.np.argsort = spy          # observe (not alter) the ordering osd.py:12 computes
            try:
                t0 = time.time()
                sol = performOSD = OSD.performOSD_enhanced(Hf, synds[i], V[i], E[i], order=0)
            finally:
                OSD.np.argsort = real_argsort
            print(f"      OSD-0 {tag} {s} case {i}: {time.time() - t0:.1f}s")
            sols.append(np.asarray(sol, np.int64)); orders.append(cap["o"].astype(np.int64))
        out[f"{s}_osd_cases"] = np.array(fails, np.int64)
        out[f"{s}_osd_solution"] = np.array(sols, np.int64).reshape(len(fails), -1)
        out[f"{s}_osd_ordering"] = np.array(orders, np.int64).reshape(len(fails), -1)
    out["max_iter"] = np.int64(max_iter)
    out["noise_rows"] = np.array(sel, np.int64)
    save(f"{tag}_decode", **out)


class RecordingRng:
    """Wraps a numpy Generator and keeps every `random(n)` draw, so the fixture can store the error patterns the reference used."""

    def __init__(self, seed):
        self.gen = np.random.default_rng(seed)
        self.draws = []

    def random(self, n):
        r = self.gen.random(n)
        self.draws.append(r.copy())
        return r


def spy_histograms(module, fn, *args, **kw):
    """Run fn and also return the (hist, edges) pairs np.histogram produced inside it (observed, not altered)."""
    real = np.histogram
    seen = []

    def spy(a, *aa, **kk):
        r = real(a, *aa, **kk)
        seen.append((np.asarray(r[0]).copy(), np.asarray(r[1]).copy()))
        return r
    module.np.histogram = spy
    try:
        out = fn(*args, **kw)
    finally:
        module.np.histogram = real
    return out, seen


def gen_estimators():
    """f4: estimate_alpha_alvarado / _autoregressive (alpha.py) and estimate_scopt_beta (scopt.py) with recorded draws."""
    out = {}
    names = []
    c = load_code("bb72")
    Hbb = np.asarray(c["Hx"], dtype=np.int64)
    n_bb = Hbb.shape[1]
    q = np.random.default_rng(5).uniform(0.01, 0.12, n_bb)
    priors_bb = {"uni": np.full(n_bb, np.log((1 - 0.05) / 0.05)), "mix": np.log((1 - q) / q)}
    m72 = np.load(os.path.join(REF, CACHE["circ72"][0]))
    Hc72 = np.asarray(m72["HdecZ"], dtype=np.int64)
    graphs = {"bb72": (Hbb, 0.05), "circ72": (Hc72, 0.005)}
    priors = {"bb72_uni": priors_bb["uni"], "bb72_mix": priors_bb["mix"], "circ72_chan": prior_llrs(m72["channel_probsZ"])}

    def record(name, gname, pname, kind, rng, result, hists, **params):
        H, p = graphs[gname]
        draws = np.array(rng.draws)
        names.append(name)
        out[f"{name}__graph"] = np.array(gname)
        out[f"{name}__prior"] = np.array(pname)
        out[f"{name}__kind"] = np.array(kind)
        out[f"{name}__p"] = np.float64(p)
        out[f"{name}__errors"] = np.packbits(draws < p, axis=1)                 # [calls * trials][ceil(n/8)]
        for k, v in params.items():
            out[f"{name}__{k}"] = np.asarray(v)
        for k, v in result.items():
            out[f"{name}__out_{k}"] = np.asarray(v, dtype=np.float64)
        out[f"{name}__hist"] = np.array([h for h, _ in hists], dtype=np.float64)   # [2 * fits][bins] density histograms (class 0, class 1, ...)
        out[f"{name}__edges"] = np.array([e for _, e in hists][::2], dtype=np.float64)
        print(f"    {name}: {result}")

    for gname, pname, trials, bins, seed in (("bb72", "bb72_uni", 300, 50, 11), ("bb72", "bb72_mix", 300, 40, 12), ("circ72", "circ72_chan", 24, 50, 13)):
        H, p = graphs[gname]
        rng = RecordingRng(seed)
        t0 = time.time()
        (a, r2), hists = spy_histograms(ALPHA, ALPHA.estimate_alpha_alvarado, csr_matrix(H), p, trials=trials, bins=bins, rng=rng, llrs=priors[pname])
        record(f"alv_{pname}", gname, pname, "alvarado", rng, {"alpha": a, "r2": r2}, hists, trials=trials, bins=bins)
        print(f"      {time.time() - t0:.1f}s")
    for gname, pname, trials, bins, iters, damping, clip, seed in (("bb72", "bb72_mix", 150, 50, 4, 1.0, 20.0, 21), ("bb72", "bb72_uni", 150, 30, 3, 0.7, 6.0, 22),
                                                                   ("circ72", "circ72_chan", 12, 50, 2, 1.0, 20.0, 23)):
        H, p = graphs[gname]
        rng = RecordingRng(seed)
        t0 = time.time()
        (av, rv), hists = spy_histograms(ALPHA, ALPHA.estimate_alpha_alvarado_autoregressive, csr_matrix(H), p, maxIter=iters, trials=trials, bins=bins,
                                         damping=damping, clip_llr=clip, rng=rng, llrs=priors[pname])
        record(f"auto_{pname}", gname, pname, "autoregressive", rng, {"alpha": av, "r2": rv}, hists, trials=trials, bins=bins, iters=iters, damping=damping, clip=clip)
        print(f"      {time.time() - t0:.1f}s")
    for tag, gname, pname, trials, bins, iters, mode, alpha, damping, clip, seed in (
            ("dyn", "bb72", "bb72_mix", 150, 50, 20, "dynamical", 1.0, 1.0, 20.0, 31),
            ("alv", "bb72", "bb72_uni", 150, 50, 12, "alvarado", 0.8, 0.8, 8.0, 32),
            ("seq", "bb72", "bb72_mix", 150, 25, 9, "alvarado-autoregressive", np.array([0.7, 0.8, 0.9]), 1.0, 20.0, 33),
            ("dyn", "circ72", "circ72_chan", 10, 50, 8, "dynamical", 1.0, 1.0, 20.0, 34)):
        H, p = graphs[gname]
        rng = RecordingRng(seed)
        t0 = time.time()
        (b, r2), hists = spy_histograms(SCOPT, SCOPT.estimate_scopt_beta, csr_matrix(H), p, trials=trials, bins=bins, alpha=alpha, alpha_mode=mode,
                                        maxIter=iters, damping=damping, clip_llr=clip, rng=rng, llrs=priors[pname])
        record(f"scopt_{tag}_{pname}", gname, pname, "scopt", rng, {"beta": b, "r2": r2}, hists, trials=trials, bins=bins, iters=iters, alpha_mode=mode,
               alpha=alpha, damping=damping, clip=clip)
        print(f"      {time.time() - t0:.1f}s")
    out["cases"] = np.array(names)
    for k, v in priors.items():
        out[f"prior__{k}"] = v
    save("estimators", **out)


def gen_osdw():
    """f1: performOSD_enhanced with order > 0 on syndromes OSD-0 cannot satisfy (the only case in which osd.py:31-75 runs)."""
    rng = np.random.default_rng(606)
    c = load_code("bb72")
    mats = {"bb72x": np.asarray(c["Hx"], dtype=np.int64),
            "dup": np.array([[1, 1, 0, 1, 0, 0, 1], [0, 1, 1, 0, 1, 0, 0], [1, 1, 0, 1, 0, 0, 1], [1, 0, 1, 1, 1, 0, 1], [0, 0, 0, 1, 1, 1, 0]], dtype=np.int64)}
    out = {}
    names = []
    real_argsort = np.argsort
    for t, (mm, nn, dens) in enumerate(((6, 10, 0.35), (8, 14, 0.3), (5, 9, 0.4), (10, 16, 0.25))):
        Hs = (rng.random((mm, nn)) < dens).astype(np.int64)
        Hs[mm // 2] = Hs[0] ^ Hs[1]                   # a dependent row: random syndromes are mostly inconsistent
        mats[f"rnd{t}"] = Hs
    plan = [("bb72x", o, mc) for o in (1, 2, 3) for mc in (None, 7)] + [("bb72x", 2, 40), ("dup", 1, None), ("dup", 2, None), ("dup", 3, 4),
                                                                         ("dup", 5, None), ("bb72x", 2, "consistent")]
    plan += [(f"rnd{t}", o, mc) for t in range(4) for o, mc in ((1, None), (2, None), (2, 9), (3, None), (4, 25), (2, None), (3, None), (1, None))]
    for k, (tag, order, mc) in enumerate(plan):
        H = mats[tag]
        m, n = H.shape
        want_change = tag.startswith("rnd") and k % 2 == 0       # half of the small cases must end on a swept candidate
        for attempt in range(2000):
            llr = rng.normal(0, 3, n)
            hard = (rng.random(n) < 0.1).astype(np.int64)
            if mc == "consistent":
                synd = (H @ (rng.random(n) < 0.1).astype(np.int64)) % 2
            else:
                synd = (rng.random(m) < 0.5).astype(np.int64)
            seen = []

            def spy(a, *aa, **kk):
                r = real_argsort(a, *aa, **kk)
                seen.append(r.copy())
                return r
            OSD.np.argsort = spy
            try:
                sol = OSD.performOSD_enhanced(H.astype(np.float64), synd, llr, hard, order=order, max_combinations=None if mc == "consistent" else mc)
                sol0 = OSD.performOSD_enhanced(H.astype(np.float64), synd, llr, hard, order=0)
            finally:
                OSD.np.argsort = real_argsort
            if not want_change or not np.array_equal(np.asarray(sol) % 2, np.asarray(sol0) % 2):
                break
        else:
            raise SystemExit(f"no draw of case {k} changes the answer")
        if mc == "consistent":
            mc = None
        sol = np.asarray(sol, dtype=np.int64) % 2
        swept = len(seen) >= 3                      # ordering, second sort (only when the sweep runs), ordering of the order-0 call
        if swept:
            assert np.array_equal(seen[1], np.arange(len(seen[1]))), "second argsort is not the identity: tie in the fixture"
        name = f"case{k}"
        names.append(name)
        out[f"{name}__graph"] = np.array(tag)
        out[f"{name}__order"] = np.int64(order)
        out[f"{name}__maxc"] = np.int64(mc or 0)
        out[f"{name}__syndrome"] = synd.astype(np.int8)
        out[f"{name}__llr"] = llr
        out[f"{name}__hard"] = hard.astype(np.int8)
        out[f"{name}__ordering"] = seen[0].astype(np.int32)
        out[f"{name}__solution"] = sol.astype(np.int8)
        out[f"{name}__swept"] = np.int64(swept)
        out[f"{name}__differs_from_osd0"] = np.int64(not np.array_equal(sol, np.asarray(sol0) % 2))
        print(f"    {name}: {tag} order={order} maxc={mc} swept={swept} differs={out[f'{name}__differs_from_osd0']}")
    for tag, H in mats.items():
        out[f"graph__{tag}"] = H.astype(np.int8)
    ndiff = sum(int(out[f"{nm}__differs_from_osd0"]) for nm in names)
    print(f"    {ndiff} of {len(names)} cases end on a swept candidate instead of the OSD-0 solution")
    assert ndiff >= 6
    out["cases"] = np.array(names)
    save("osdw", **out)


# --------------------------------------------------------------------------- whole circuit-level trials
# The decoder settings of the trial fixtures.  Alpha values are fixed inputs (the reference's estimators are too slow in pure
# Python, and _run_single_trial_fast takes alpha as given).  Config B is main.py's operating point; its X sequence is
# shorter than maxIter, so iterations 7..19 reuse its last value (dense.py:62, kernels.py minsum_decoder_full_autoregressive).
TRIAL_CONFIGS = {
    "A": dict(max_iter=50, osd_order=0, alpha_mode="dynamical", alpha_z=1.0, alpha_x=1.0),
    "B": dict(max_iter=20, osd_order=2, alpha_mode="alvarado-autoregressive",
              alpha_z=np.round(np.linspace(0.62, 0.95, 20), 6),
              alpha_x=np.array([0.58, 0.66, 0.72, 0.78, 0.82, 0.86, 0.88])),
    "C": dict(max_iter=30, osd_order=0, alpha_mode="alvarado", alpha_z=0.75, alpha_x=0.85),
}
# (tag) -> list of (config, [(error_rate, base_seed, trials, want_z_only, want_x_only, want_osd)])
TRIAL_PLAN = {
    "circ72": [(c, [(0.005, 7200, 12, 1, 1, 4), (0.01, 7201, 12, 3, 3, 2)]) for c in "ABC"],
    "circ144": [(c, [(0.005, 14400, 8, 2, 2, 2)]) for c in "AB"],
    "circ288": [("B", [(0.005, 28800, 2, 0, 0, 0)])],
}


def _oracle():
    sys.path.insert(0, REPO)
    from oracle import oracle as orc
    orc.build()
    return orc


def _trial_shared_data(tag, cfg, error_rate, base_seed):
    """shared_data of engine.py:391-419 for precomputed matrices (load_matrices) and fixed alpha values."""
    from src.utils.caching import load_matrices
    path, code, cycles, _ = CACHE[tag]
    key = os.path.basename(path)[len("matrices_"):-len(".npz")]
    matrices = load_matrices(os.path.join(REF, "matrix_cache"), key)
    d, cb, comp = build_circuit(tag)
    Lx, Lz = d["Lx"], d["Lz"]
    with np.errstate(divide='ignore', invalid='ignore'):                      # engine.py:210-212
        llrs_z = np.clip(np.nan_to_num(np.log((1 - matrices['channel_probsZ']) / matrices['channel_probsZ'])), -50, 50)
        llrs_x = np.clip(np.nan_to_num(np.log((1 - matrices['channel_probsX']) / matrices['channel_probsX'])), -50, 50)
    use_sparse = matrices['HdecZ'].shape[1] > 5000                            # engine.py:214
    sd = {
        'error_rate': error_rate, 'Lx': Lx, 'Lz': Lz,
        'HdecZ': np.asarray(matrices['HdecZ'], dtype=np.float64, order='C'),
        'HdecX': np.asarray(matrices['HdecX'], dtype=np.float64, order='C'), 'llrs_z': llrs_z, 'llrs_x': llrs_x,
        'HZ_logical': np.ascontiguousarray(matrices['HZ_full'][matrices['first_logical_rowZ']:matrices['first_logical_rowZ'] + Lx.shape[0]]),
        'HX_logical': np.ascontiguousarray(matrices['HX_full'][matrices['first_logical_rowX']:matrices['first_logical_rowX'] + Lx.shape[0]]),
        'alpha_mode': cfg["alpha_mode"], 'alpha_z': cfg["alpha_z"], 'alpha_x': cfg["alpha_x"],
        'maxIter': cfg["max_iter"], 'osd_order': cfg["osd_order"],
        'base_seed': base_seed, 'use_sparse': use_sparse,
        'HdecZ_csr': csr_matrix(matrices['HdecZ']) if use_sparse else None,
        'HdecX_csr': csr_matrix(matrices['HdecX']) if use_sparse else None,
        'compiled_circuit': comp,
    }
    return sd


def _screen_trials(orc, sd, base_seed, count):
    """Seed selection only (nothing of it is stored): the oracle's verdicts for trials base_seed + 0 .. count-1, so the fixture can
    pick trials that exercise the hard cases.  Returns int arrays (z_err, x_err, osd_z, osd_x)."""
    comp = sd["compiled_circuit"]
    fx = {k: getattr(comp, k) for k in ("base_ops", "base_q1", "base_q2", "suffix_ops", "suffix_q1", "suffix_q2", "total_qubits",
                                        "max_circuit_size", "max_syndromes_x", "max_syndromes_z", "x_syn_positions", "x_syn_ptrs",
                                        "z_syn_positions", "z_syn_ptrs", "num_x_checks", "num_z_checks", "data_qubit_indices")}
    fx["Lx"], fx["Lz"] = sd["Lx"], sd["Lz"]
    n_locs = comp.num_error_locs
    SZ, TZ, SX, TX = [], [], [], []
    for i in range(count):
        np.random.seed(base_seed + i)
        rv = np.random.random(n_locs)
        rp = np.random.randint(0, 3, n_locs, dtype=np.int32)
        rt = np.random.randint(0, 15, n_locs, dtype=np.int32)
        a, b, c, e = orc.run_trial(fx, sd["error_rate"], rv, rp, rt)
        SZ.append(a); TZ.append(b); SX.append(c); TX.append(e)
    res = []
    for s, S, T, al in (("Z", SZ, TZ, sd["alpha_z"]), ("X", SX, TX, sd["alpha_x"])):
        Hc = csr_of(sd[f"Hdec{s}"])
        ip, ix, n = Hc.indptr.astype(np.int32), Hc.indices.astype(np.int32), Hc.shape[1]
        E, C, V, _ = orc.minsum_decode_batch(ip, ix, n, np.array(S), sd[f"llrs_{s.lower()}"], max_iter=sd["maxIter"], alpha=al,
                                             alpha_mode=sd["alpha_mode"], threads=0)
        Lg = sd[f"H{s}_logical"].astype(np.int64)
        err = np.zeros(count, np.int64)
        for i in range(count):
            det = E[i] if C[i] else orc.osd0(ip, ix, n, S[i], V[i], E[i])
            err[i] = not np.array_equal((Lg @ det.astype(np.int64)) % 2, T[i])
        res += [err, 1 - C.astype(np.int64)]
    return res[0], res[2], res[1], res[3]


def _pick_trials(screen, total, want_z, want_x, want_osd):
    z, x, oz, ox = screen
    picked = []
    for cond, k in ((z & ~x & 1, want_z), (x & ~z & 1, want_x), ((oz | ox) & ~(z | x) & 1, want_osd)):
        picked += [int(i) for i in np.flatnonzero(cond) if i not in picked][:k]
    picked += [i for i in range(len(z)) if i not in picked][:total - len(picked)]
    return sorted(picked[:total])


def _packbits(a):
    return np.packbits(np.asarray(a, np.uint8) % 2, axis=-1, bitorder="little")


def gen_trials(tag, screen_count=None, posteriors_per_sector=2):
    """Whole circuit-level trials by the reference's own _run_single_trial_fast (engine.py:68-122), imported, not re-composed.

    engine.py imports rich and multiprocessing; both import here, no stub is needed.  The decoder and OSD calls the trial makes
    are observed (not altered) by wrapping the names engine.py imported: each BP call's hard decision, success flag, final
    iteration and (for a few decodes) posteriors; each OSD call's np.argsort order (osd.py:12) and solution.  Every OSD call is
    then repeated with np.argsort forced to kind="stable" -- the device's tie rule -- and that solution and the verdict it leads to
    are stored too.  One file per (tag, config): {tag}_trials_{config}.npz."""
    import src.simulation.engine as ENG
    orc = _oracle()
    real = {k: getattr(ENG, k) for k in ("performMinSum_Symmetric", "performMinSum_Symmetric_Sparse", "performOSD_enhanced")}
    real_argsort = np.argsort
    for cname, groups in TRIAL_PLAN[tag]:
        cfg = TRIAL_CONFIGS[cname]
        t_start = time.time()
        rows = []                      # one dict per trial
        for error_rate, base_seed, total, wz, wx, wo in groups:
            sd = _trial_shared_data(tag, cfg, error_rate, base_seed)
            scount = (screen_count or (400 if tag == "circ72" else 1500)) if wz or wx or wo else total
            t0 = time.time()
            scr = _screen_trials(orc, sd, base_seed, scount)
            idxs = _pick_trials(scr, total, wz, wx, wo)
            print(f"    {tag} {cname} p={error_rate}: screened {scount} trials in {time.time() - t0:.0f}s "
                  f"(z-only {int((scr[0] & ~scr[1] & 1).sum())}, x-only {int((scr[1] & ~scr[0] & 1).sum())}) -> {idxs}")
            for idx in idxs:
                calls = []

                def bp_spy(name):
                    def f(*a, **k):
                        r = real[name](*a, **k)
                        calls.append(("bp", np.asarray(r[0], np.int8).copy(), bool(r[1]), np.asarray(r[2], np.float64).copy(), int(r[3])))
                        return r
                    return f

                def osd_spy(H, syndrome, llr, hard, order=0, max_combinations=None):
                    seen = []

                    def spy(a, *aa, **kk):
                        r = real_argsort(a, *aa, **kk)
                        if seen:               # the order-w sweep's second sort (osd.py:40) must be tie free, else the fixture is ambiguous
                            assert np.array_equal(r, real_argsort(a, kind="stable"))
                        seen.append(r.copy())
                        return r

                    def stable(a, *aa, **kk):
                        kk["kind"] = "stable"
                        return real_argsort(a, *aa, **kk)
                    ENG.np.argsort = spy
                    try:
                        sol = real["performOSD_enhanced"](H, syndrome, llr, hard, order=order, max_combinations=max_combinations)
                    finally:
                        ENG.np.argsort = real_argsort
                    ENG.np.argsort = stable
                    try:
                        sol_st = real["performOSD_enhanced"](H, syndrome, llr, hard, order=order, max_combinations=max_combinations)
                    finally:
                        ENG.np.argsort = real_argsort
                    calls.append(("osd", seen[0].copy(), np.asarray(sol, np.int64) % 2, np.asarray(sol_st, np.int64) % 2, len(seen) > 1))
                    return sol

                ENG.performMinSum_Symmetric = bp_spy("performMinSum_Symmetric")
                ENG.performMinSum_Symmetric_Sparse = bp_spy("performMinSum_Symmetric_Sparse")
                ENG.performOSD_enhanced = osd_spy
                try:
                    t0 = time.time()
                    verdict = ENG._run_single_trial_fast(idx, sd)
                finally:
                    for k, v in real.items():
                        setattr(ENG, k, v)
                np.random.seed(base_seed + idx)          # the same draws once more, for the stored syndromes / logicals
                spz, tz, spx, tx = run_trial_fast(sd["compiled_circuit"], error_rate, sd["Lx"], sd["Lz"])
                row = dict(error_rate=error_rate, base_seed=base_seed, trial=idx, verdict=np.array(verdict, np.uint8),
                           use_sparse=sd["use_sparse"], Z_syndrome=np.asarray(spz, np.int8), X_syndrome=np.asarray(spx, np.int8),
                           Z_true=np.asarray(tz, np.int8), X_true=np.asarray(tx, np.int8))
                it = iter(calls)
                for s in "ZX":
                    bp = next(it)
                    assert bp[0] == "bp"
                    row[f"{s}_hard"], row[f"{s}_succ"], row[f"{s}_post"], row[f"{s}_iter"] = bp[1], bp[2], bp[3], bp[4]
                    det = bp[1].astype(np.int64)
                    row[f"{s}_osd"] = None
                    if not bp[2]:
                        o = next(it)
                        assert o[0] == "osd"
                        row[f"{s}_osd"] = dict(ordering=o[1], solution=o[2], stable=o[3], swept=o[4])
                        det = o[2]
                    row[f"{s}_det"] = det
                    Lg = sd[f"H{s}_logical"]
                    stable_det = row[f"{s}_osd"]["stable"] if row[f"{s}_osd"] else det
                    row[f"{s}_err_stable"] = not np.array_equal((Lg @ stable_det) % 2, row[f"{s}_true"])
                    assert (not np.array_equal((Lg @ det) % 2, row[f"{s}_true"])) == bool(verdict["ZX".index(s)])
                assert next(it, None) is None
                row["verdict_stable"] = np.array([row["Z_err_stable"], row["X_err_stable"], row["Z_err_stable"] or row["X_err_stable"]], np.uint8)
                print(f"      trial {base_seed}+{idx}: {time.time() - t0:.1f}s verdict={tuple(int(v) for v in verdict)} "
                      f"succ=({row['Z_succ']},{row['X_succ']}) iters=({row['Z_iter']},{row['X_iter']})")
                rows.append(row)
        save_fixed(f"{tag}_trials_{cname}", **_pack_trials(cfg, rows, posteriors_per_sector))
        print(f"    {tag} {cname}: {len(rows)} trials in {time.time() - t_start:.0f}s")


def _pack_trials(cfg, rows, per_sector):
    out = dict(max_iter=np.int64(cfg["max_iter"]), osd_order=np.int64(cfg["osd_order"]), alpha_mode=np.array(cfg["alpha_mode"]),
               alpha_Z=np.asarray(cfg["alpha_z"], np.float64), alpha_X=np.asarray(cfg["alpha_x"], np.float64),
               use_sparse=np.uint8(rows[0]["use_sparse"]),
               error_rate=np.array([r["error_rate"] for r in rows]), base_seed=np.array([r["base_seed"] for r in rows], np.int64),
               trial=np.array([r["trial"] for r in rows], np.int64), verdict=np.array([r["verdict"] for r in rows]),
               verdict_stable=np.array([r["verdict_stable"] for r in rows]))
    for s in "ZX":
        out[f"{s}_syndrome"] = _packbits([r[f"{s}_syndrome"] for r in rows])
        out[f"{s}_true"] = np.array([r[f"{s}_true"] for r in rows], np.uint8)
        out[f"{s}_hard"] = _packbits([r[f"{s}_hard"] for r in rows])
        out[f"{s}_succ"] = np.array([r[f"{s}_succ"] for r in rows], np.uint8)
        out[f"{s}_iter"] = np.array([r[f"{s}_iter"] for r in rows], np.int32)
        out[f"{s}_det"] = _packbits([r[f"{s}_det"] for r in rows])
        osd = [t for t, r in enumerate(rows) if r[f"{s}_osd"] is not None]
        n = rows[0][f"{s}_hard"].size
        assert n < 2 ** 15
        out[f"{s}_osd_trials"] = np.array(osd, np.int64)
        out[f"{s}_osd_ordering"] = np.array([rows[t][f"{s}_osd"]["ordering"] for t in osd], np.int16).reshape(len(osd), n)
        out[f"{s}_osd_swept"] = np.array([rows[t][f"{s}_osd"]["swept"] for t in osd], np.uint8)
        out[f"{s}_osd_stable"] = _packbits([rows[t][f"{s}_osd"]["stable"] for t in osd]).reshape(len(osd), -1)
        out[f"{s}_osd_tie_changes_solution"] = np.array([not np.array_equal(rows[t][f"{s}_osd"]["stable"], rows[t][f"{s}_osd"]["solution"])
                                                         for t in osd], np.uint8)
        # posteriors of a few decodes: OSD'd ones first (all maxIter iterations, so the whole alpha sequence is used), and for X one
        # with +-inf entries if the OSD'd ones have none
        post = osd[:per_sector]
        if s == "X" and not any(np.isinf(rows[t]["X_post"]).any() for t in post):
            post += [t for t, r in enumerate(rows) if np.isinf(r["X_post"]).any() and t not in post][:1]
        out[f"{s}_post_trials"] = np.array(post, np.int64)
        out[f"{s}_post"] = np.array([rows[t][f"{s}_post"] for t in post], np.float64).reshape(len(post), n)
    out["tie_changes_verdict"] = np.array([not np.array_equal(r["verdict"], r["verdict_stable"]) for r in rows], np.uint8)
    return out


# --------------------------------------------------------------------------- graph shapes beyond the BB matrices
def gen_wg_shapes():
    """Six small families of tests/graph_shapes.py (rows of degree 40 and 57, column degrees 0 .. 8, two degree-1 checks on one column, odd nnz,
    eleven 64-column chunks) through the reference's own decoder: 8 syndromes each, max_iter = 12.  The fixture stores the graph, prior and
    syndromes the generator returned and the reference's (error, converged, values, final_iter)."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import graph_shapes as GS
    out, names = {}, []
    for c in GS.families():
        if not c.golden:
            continue
        names.append(c.name)
        pn = next(iter(c.priors))
        prior = c.priors[pn]
        S = GS.syndromes(c, 8)
        Hc = csr_matrix((np.ones(c.nnz, np.int8), c.indices, c.indptr), shape=(c.m, c.n))
        E, C, V, I = batch_sparse(Hc, S, prior, maxIter=12, alpha_mode="dynamical")
        for k, v in (("indptr", c.indptr), ("indices", c.indices), ("n", np.int64(c.n)), ("prior_name", np.array(pn)), ("prior", prior), ("syndromes", S),
                     ("max_iter", np.int64(12)), ("err", E), ("conv", C), ("llr", V), ("iter", I)):
            out[f"{c.name}__{k}"] = v
        print(f"  {c.name}: {c.m} x {c.n}, nnz {c.nnz}, converged {int(C.sum())}/8, NaN {bool(np.isnan(V).any())}")
    out["families"] = np.array(names)
    save_fixed("wg_shapes", **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None)
    ap.add_argument("--trial-tags", default=",".join(TRIAL_PLAN), help="circuits of --only trials")
    a = ap.parse_args()
    todo = a.only.split(",") if a.only else ["data", "steane", "bb", "core", "gf2", "circ72", "circ144", "estimators", "osdw", "bb256", "gf2big", "wgshapes", "trials"]
    t0 = time.time()
    if "data" in todo:
        print("[data]"); pack_data()
    if "steane" in todo:
        print("[steane]"); gen_steane()
    if "bb" in todo:
        rng = np.random.default_rng(20260206)
        for tag, nsyn in (("bb72", 64), ("bb144", 64), ("bb288", 32)):
            print(f"[{tag}]"); gen_bb(tag, nsyn, rng)
    if "core" in todo:
        print("[core]"); gen_core()
    if "gf2" in todo:
        print("[gf2]"); gen_gf2()
    if "circ72" in todo:
        print("[circ72]"); nz = gen_noise("circ72", 8); gen_circuit_decode("circ72", nz, 4, 3, 50)
    if "circ144" in todo:
        # SURVEY 8c counts at production size: 8 draws per error rate, 16 syndromes and 8 reference OSD-0 solutions per sector
        print("[circ144]"); nz = gen_noise("circ144", 16); gen_circuit_decode("circ144", nz, 8, 8, 50, extra=8)
    if "estimators" in todo:
        print("[estimators]"); gen_estimators()
    if "osdw" in todo:
        print("[osdw]"); gen_osdw()
    if "bb256" in todo:
        print("[bb256]"); gen_bb256()
    if "gf2big" in todo:
        print("[gf2big]"); gen_gf2_big()
    if "wgshapes" in todo:
        print("[wgshapes]"); gen_wg_shapes()
    if "trials" in todo:
        for tag in a.trial_tags.split(","):
            print(f"[trials {tag}]"); gen_trials(tag)
    print(f"done in {time.time() - t0:.0f}s")


if __name__ == "__main__":
    main()
