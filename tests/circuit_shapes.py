"""Small syndrome-extraction circuits at the sizes where the circuit-plan samplers index differently than on the bundled BB plans, and a model of
the per-location fault signatures that shares nothing with the library.

The bundled circ72 plan has n_locs = 4320 (a multiple of 4 and of 32), 288 detectors in both sectors (9 whole words each, an even word count),
k = 12 and a base circuit that ends in a preparation.  SHAPES holds five circuits off every one of those multiples; test_circuit_shapes_cpu.py pins
their edges and the model, test_circuit_shapes_gpu.py compares the kernels on them.

The frame law, from the header of csrc/circuit.hip and noise/kernels.py: a Z frame moves target -> control through a CNOT, is cleared by PrepX and
read by MeasX; an X frame moves control -> target, is cleared by PrepZ and read by MeasZ.  A fault flips the frame BEFORE a measurement and AFTER a
preparation or CNOT (an IDLE does nothing, so either).  Detector s is raw measurement s XOR the previous raw measurement of the same check; the
logical bits are L @ (frame of the data qubits) at the end of base circuit + suffix.  Plain module (no pytest hooks)."""
import functools
from types import SimpleNamespace

import numpy as np

OP_CNOT, OP_PREP_X, OP_PREP_Z, OP_MEAS_X, OP_MEAS_Z, OP_IDLE = 1, 2, 3, 4, 5, 6
# component masks of csrc/sampler_common.h: bit0 = X on slot 0, bit1 = X on slot 1, bit2 = Z on slot 0, bit3 = Z on slot 1
CNOT_COMP = (1, 5, 4, 2, 10, 8, 3, 15, 12, 11, 7, 13, 14, 9, 6)
IDLE_COMP = (1, 5, 4)


# ---------------------------------------------------------------------------------------- GF(2) helpers for the logical operators
def _row_reduce(M):
    """-> (reduced rows without the zero ones, pivot columns) over GF(2)"""
    M = (np.array(M, np.uint8) & 1).reshape(-1, np.asarray(M).shape[-1])
    rows, piv = [], []
    for r in M:
        r = r.copy()
        for q, c in zip(rows, piv):
            if r[c]:
                r ^= q
        if r.any():
            c = int(np.flatnonzero(r)[0])
            for i in range(len(rows)):
                if rows[i][c]:
                    rows[i] = rows[i] ^ r
            rows.append(r)
            piv.append(c)
    return rows, piv


def _nullspace(H):
    H = np.asarray(H, np.uint8) & 1
    n = H.shape[1]
    rows, piv = _row_reduce(H)
    out = []
    for f in (c for c in range(n) if c not in piv):
        v = np.zeros(n, np.uint8)
        v[f] = 1
        for r, c in zip(rows, piv):
            v[c] = r[f]
        out.append(v)
    return out


def css_logicals(Hx, Hz):
    """(Lx, Lz): representatives of ker Hz / row space Hx and of ker Hx / row space Hz, uint8[k, n]"""
    out = []
    for checks, stabs in ((Hz, Hx), (Hx, Hz)):
        rows, piv = _row_reduce(stabs)
        keep = []
        for v in _nullspace(checks):
            r = v.copy()
            for q, c in zip(rows, piv):
                if r[c]:
                    r ^= q
            if r.any():
                c = int(np.flatnonzero(r)[0])
                for i in range(len(rows)):
                    if rows[i][c]:
                        rows[i] = rows[i] ^ r
                rows.append(r)
                piv.append(c)
                keep.append(v)
        out.append(np.array(keep, np.uint8).reshape(len(keep), np.asarray(Hx).shape[1]))
    assert out[0].shape == out[1].shape
    return out[0], out[1]


# ---------------------------------------------------------------------------------------- the circuit builder
class CSSCircuit:
    """Serial syndrome extraction of any CSS code, with the attributes CompiledCircuit and build_decoding_matrices read.  One cycle: PrepX of the X
    ancillas; check by check the CNOTs ancilla -> data of every X check, then data -> ancilla of every Z check; `idle` IDLEs on the data qubits in
    turn; MeasZ of the Z ancillas; MeasX of the X ancillas; PrepZ of the Z ancillas.  prep_z_first moves the PrepZ to the start of the cycle, so
    that the base circuit ends in MeasX.  The noiseless suffix is two more cycles, as for the BB circuits."""

    def __init__(self, Hx, Hz, num_cycles, idle=0, prep_z_first=False):
        Hx, Hz = np.asarray(Hx, np.uint8) & 1, np.asarray(Hz, np.uint8) & 1
        assert Hx.shape[1] == Hz.shape[1] and not ((Hx.astype(int) @ Hz.T.astype(int)) & 1).any()
        self.Hx, self.Hz, self.num_cycles, self.n = Hx, Hz, int(num_cycles), Hx.shape[1]
        self.Xchecks = [("Xcheck", i) for i in range(Hx.shape[0])]
        self.Zchecks = [("Zcheck", i) for i in range(Hz.shape[0])]
        self.data_qubits = [("data", j) for j in range(self.n)]
        self.lin_order = {q: i for i, q in enumerate(self.Xchecks + self.data_qubits + self.Zchecks)}
        prep_z = [("PrepZ", q) for q in self.Zchecks]
        ops = list(prep_z) if prep_z_first else []
        ops += [("PrepX", q) for q in self.Xchecks]
        for i, c in enumerate(self.Xchecks):
            ops += [("CNOT", c, ("data", int(j))) for j in np.flatnonzero(Hx[i])]
        for i, c in enumerate(self.Zchecks):
            ops += [("CNOT", ("data", int(j)), c) for j in np.flatnonzero(Hz[i])]
        ops += [("IDLE", ("data", j % self.n)) for j in range(idle)]
        ops += [("MeasZ", q) for q in self.Zchecks] + [("MeasX", q) for q in self.Xchecks]
        if not prep_z_first:
            ops += prep_z
        self.cycle = ops

    def get_full_circuit(self):
        return self.cycle * self.num_cycles


def _repetition(n, closed=False):
    H = np.zeros((n if closed else n - 1, n), np.uint8)
    for i in range(H.shape[0]):
        H[i, i] = H[i, (i + 1) % n] = 1
    return H


def _hgp(H1, H2):
    """hypergraph product: Hx = [H1 (x) I | I (x) H2^T], Hz = [I (x) H2 | H1^T (x) I]"""
    (r1, n1), (r2, n2) = H1.shape, H2.shape
    I = lambda m: np.eye(m, dtype=np.uint8)      # noqa: E731
    return np.hstack([np.kron(H1, I(n2)), np.kron(I(r1), H2.T)]), np.hstack([np.kron(I(n1), H2), np.kron(H1.T, I(r2))])


_C422 = np.ones((1, 4), np.uint8)
_HAMMING = np.array([[1, 0, 1, 0, 1, 0, 1], [0, 1, 1, 0, 0, 1, 1], [0, 0, 0, 1, 1, 1, 1]], np.uint8)
_SHOR_X = np.array([[1, 1, 1, 1, 1, 1, 0, 0, 0], [0, 0, 0, 1, 1, 1, 1, 1, 1]], np.uint8)
_SHOR_Z = np.array([[1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 1, 1, 0, 0, 0, 0, 0, 0], [0, 0, 0, 1, 1, 0, 0, 0, 0], [0, 0, 0, 0, 1, 1, 0, 0, 0],
                    [0, 0, 0, 0, 0, 0, 1, 1, 0], [0, 0, 0, 0, 0, 0, 0, 1, 1]], np.uint8)

# name -> (Hx, Hz, cycles, idles per cycle, PrepZ first).  What each must keep is asserted by test_circuit_shapes_cpu.py::test_the_table_keeps_its_edges.
SHAPES = {
    "c422": lambda: (_C422, _C422, 1, 1, True),                                            # 13 locations, 3 detectors per sector, ends in MeasX
    "steane": lambda: (_HAMMING, _HAMMING, 3, 1, False),                                   # k = 1, 111 locations, 18 measurements
    "shor": lambda: (_SHOR_X, _SHOR_Z, 4, 1, False),                                       # 12 and 36 detectors: 1 + 2 words
    "k64": lambda: (np.kron(np.eye(32, dtype=np.uint8), _C422),) * 2 + (1, 3, False),      # 32 copies of [[4,2,2]]: k = 64
    "hgp": lambda: _hgp(_repetition(3), _repetition(4)) + (33, 1, False),                  # 8 and 9 checks, 35 rounds: 280 and 315 detectors
}


@functools.lru_cache(maxsize=None)
def shape(name):
    """-> namespace(name, cb, compiled, Lx, Lz, k, n_locs, nsx, nsz, n_meas): the circuit of SHAPES[name], compiled by the package's host code"""
    import qldpc_amd  # noqa: F401
    from qldpc_amd.noise.compiled import CompiledCircuit
    Hx, Hz, cycles, idle, first = SHAPES[name]()
    cb = CSSCircuit(Hx, Hz, cycles, idle, first)
    Lx, Lz = css_logicals(Hx, Hz)
    comp = CompiledCircuit(base_circuit=cb.get_full_circuit(), noiseless_suffix=cb.cycle * 2, lin_order=cb.lin_order, data_qubits=cb.data_qubits,
                           Xchecks=cb.Xchecks, Zchecks=cb.Zchecks)
    ops = np.asarray(comp.base_ops)
    return SimpleNamespace(name=name, cb=cb, compiled=comp, Lx=Lx, Lz=Lz, k=Lx.shape[0], n_locs=int(ops.size), nsx=int(comp.x_syn_ptrs[-1]),
                           nsz=int(comp.z_syn_ptrs[-1]), n_meas=int(np.isin(ops, (OP_MEAS_X, OP_MEAS_Z)).sum()))


# ---------------------------------------------------------------------------------------- the signature model
def signatures_model(compiled, Lx, Lz, sector_is_x):
    """(ptr int32[2 N + 1], idx uint16[...], logmask uint64[2 N]) in the layout of _lib.circuit_fault_signatures: entry 2 * location + slot holds the
    detectors (ascending) and logical bits that one flip of the sector's kind on the gate's first qubit (slot 0) or on a CNOT's target (slot 1)
    turns; slot 1 of every other gate is empty.  One frame per entry, all walked through base circuit + suffix at once."""
    base = np.asarray(compiled.base_ops, np.int64)
    ops = np.concatenate([base, np.asarray(compiled.suffix_ops, np.int64)])
    q1 = np.concatenate([compiled.base_q1, compiled.suffix_q1]).astype(np.int64)
    q2 = np.concatenate([compiled.base_q2, compiled.suffix_q2]).astype(np.int64)
    N = base.size
    prep, meas = (OP_PREP_Z, OP_MEAS_Z) if sector_is_x else (OP_PREP_X, OP_MEAS_X)
    pos, ptrs = ((compiled.z_syn_positions, compiled.z_syn_ptrs) if sector_is_x else (compiled.x_syn_positions, compiled.x_syn_ptrs))
    L = np.asarray(Lz if sector_is_x else Lx, np.int64)
    frame = np.zeros((int(compiled.total_qubits), 2 * N), np.uint8)
    raw = []
    for i in range(ops.size):
        op, a, c = int(ops[i]), int(q1[i]), int(q2[i])
        after = op in (OP_PREP_X, OP_PREP_Z, OP_CNOT)
        if i < N and not after:
            frame[a, 2 * i] ^= 1
        if op == OP_CNOT:
            if sector_is_x:
                frame[c] ^= frame[a]
            else:
                frame[a] ^= frame[c]
        elif op == prep:
            frame[a] = 0
        elif op == meas:
            raw.append(frame[a].copy())
        if i < N and after:
            frame[a, 2 * i] ^= 1
            if op == OP_CNOT:
                frame[c, 2 * i + 1] ^= 1
    raw = np.array(raw, np.uint8).reshape(len(raw), 2 * N)
    assert raw.shape[0] == int(ptrs[-1])                                    # every measurement of this kind belongs to a check
    det = raw.copy()
    for k in range(len(ptrs) - 1):
        mine = np.asarray(pos[ptrs[k]:ptrs[k + 1]], np.int64)
        det[mine[1:]] ^= raw[mine[:-1]]
    logical = (L @ frame[np.asarray(compiled.data_qubit_indices, np.int64)].astype(np.int64)) & 1          # [k, 2 N]
    entry, d = np.nonzero(det.T)                                            # entry-major, detectors ascending inside an entry
    ptr = np.zeros(2 * N + 1, np.int32)
    np.cumsum(np.bincount(entry, minlength=2 * N), out=ptr[1:])
    logmask = np.zeros(2 * N, np.uint64)
    for r in range(L.shape[0]):
        logmask |= logical[r].astype(np.uint64) << np.uint64(r)
    return ptr, d.astype(np.uint16), logmask


@functools.lru_cache(maxsize=None)
def model_signatures(name):
    """(signatures of sector Z, of sector X) of a shape, from the model, once"""
    S = shape(name)
    return tuple(signatures_model(S.compiled, S.Lx, S.Lz, x) for x in (False, True))


def xor_of_signatures(S, sigs, faults):
    """(sparse_z, true_z, sparse_x, true_x) int8: the XOR of the signatures of the components of `faults` = [(location, Pauli choice)]"""
    ty = np.asarray(S.compiled.base_ops)
    out = [np.zeros(S.nsx, np.int8), np.zeros(S.k, np.int8), np.zeros(S.nsz, np.int8), np.zeros(S.k, np.int8)]
    for l, choice in faults:
        comp = {OP_MEAS_X: 4, OP_PREP_X: 4, OP_MEAS_Z: 1, OP_PREP_Z: 1}.get(int(ty[l]))
        if comp is None:
            comp = IDLE_COMP[choice] if ty[l] == OP_IDLE else CNOT_COMP[choice]
        for s, bits in ((0, (4, 8)), (1, (1, 2))):
            ptr, idx, lm = sigs[s]
            for slot, bit in enumerate(bits):
                if comp & bit:
                    e = 2 * l + slot
                    out[2 * s][idx[ptr[e]:ptr[e + 1]].astype(np.int64)] ^= 1
                    out[2 * s + 1] ^= np.array([(int(lm[e]) >> r) & 1 for r in range(S.k)], np.int8)
    return tuple(out)


# ---------------------------------------------------------------------------------------- the literal simulation of chosen faults
def fault_randoms(n_locs, faults):
    """the three arrays of run_trial_with_randoms that insert exactly `faults` = [(location, Pauli choice)] at error_rate 0.5: random_vals 0 at the
    chosen locations and 1 elsewhere, the choice as both the one-qubit and the two-qubit Pauli index (each gate reads its own)"""
    rv = np.ones(n_locs)
    rp, rt = np.zeros(n_locs, np.int32), np.zeros(n_locs, np.int32)
    for l, choice in faults:
        rv[l] = 0.0
        rp[l], rt[l] = min(choice, 2), choice
    return rv, rp, rt


def literal_trial(compiled, Lx, Lz, faults, run=None):
    """One call of run_trial_with_randoms with exactly the given faults inserted -> (sparse_z, true_z, sparse_x, true_x).  run: the function to call
    as run(compiled, 0.5, Lx, Lz, random_vals, random_paulis, random_two_qubit); None is the CPU oracle's edition of the same walk (oracle.run_trial:
    insert the fault gates into the op list, propagate both frames gate by gate), which needs no GPU."""
    rv, rp, rt = fault_randoms(int(np.asarray(compiled.base_ops).size), faults)
    if run is not None:
        return tuple(np.asarray(x, np.int8) for x in run(compiled, 0.5, Lx, Lz, rv, rp, rt))
    from oracle import oracle as orc
    fx = {k: getattr(compiled, k) for k in ("base_ops", "base_q1", "base_q2", "suffix_ops", "suffix_q1", "suffix_q2", "total_qubits", "max_circuit_size",
                                            "max_syndromes_x", "max_syndromes_z", "x_syn_positions", "x_syn_ptrs", "z_syn_positions", "z_syn_ptrs",
                                            "num_x_checks", "num_z_checks", "data_qubit_indices")}
    fx["Lx"], fx["Lz"] = np.asarray(Lx, np.uint8), np.asarray(Lz, np.uint8)
    return orc.run_trial(fx, 0.5, rv, rp, rt)


def random_fault_sets(S, count, seed):
    """`count` sets of 1 .. 8 distinct locations with a Pauli choice each (0 .. 2 on an IDLE, 0 .. 14 on a CNOT, 0 elsewhere); the last location is in
    the first set, and set i holds a location of the (i mod 6)-th gate class the circuit has"""
    rng = np.random.default_rng(seed)
    ty = np.asarray(S.compiled.base_ops)
    classes = np.unique(ty)
    out = []
    for i in range(count):
        locs = rng.choice(S.n_locs, size=int(rng.integers(1, min(8, S.n_locs) + 1)), replace=False).tolist()
        if i == 0 and S.n_locs - 1 not in locs:
            locs[0] = S.n_locs - 1
        want = classes[i % classes.size]
        if not (ty[locs] == want).any():
            locs[-1] = int(rng.choice(np.setdiff1d(np.flatnonzero(ty == want), locs)))
        out.append([(l, int(rng.integers(0, {OP_IDLE: 3, OP_CNOT: 15}.get(int(ty[l]), 1)))) for l in locs])
    return out
