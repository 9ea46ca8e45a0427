"""ctypes binding of csrc/libqldpc_hip.so (C ABI: include/qldpc_hip.h).  Fails loudly; no CPU fallback."""
import ctypes as C
import hashlib
import os
import threading
from collections import OrderedDict

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# the product library.  select_build() switches THIS module to another build of the same ABI before the library is first used:
#   "experiments"  libqldpc_hip_experiments.so: plus the measured-and-rejected kernels (the parity tests load it through tests/conftest.py)
#   "timers"       libqldpc_hip_timers.so: clock reads inside the kernels (tools/ diagnostics; make -C csrc timers)
SO_PATH = os.path.join(_HERE, "csrc", "libqldpc_hip.so")
BUILD = "product"


def select_build(name):
    """Point this module at another build of the library ("product", "experiments", "timers").  Only before the first call into it."""
    global SO_PATH, BUILD
    if _lib is not None and name != BUILD:
        raise QldpcError(f"library already loaded ({BUILD}); select_build must come first")
    fn = {"product": "libqldpc_hip.so", "experiments": "libqldpc_hip_experiments.so", "timers": "libqldpc_hip_timers.so"}.get(name, name)   # or a file name in csrc/ (A/B builds of tools/)
    SO_PATH, BUILD = os.path.join(_HERE, "csrc", fn), name

ALPHA_CONST, ALPHA_DYNAMIC, ALPHA_SEQ = 0, 1, 2
FLAG_FIXED_ITERS, FLAG_KERNEL_STREAM, FLAG_KERNEL_RESIDENT, FLAG_KERNEL_GENERIC, FLAG_MC_UNFUSED = 0x1, 0x10, 0x20, 0x40, 0x80
TALLY_SLOTS = 16
TALLY = {"trials": 0, "z_err": 1, "x_err": 2, "total_err": 3, "bp_conv_z": 4, "bp_conv_x": 5, "osd_z": 6, "osd_x": 7,
         "iters_z": 8, "iters_x": 9, "zero_synd_z": 10, "zero_synd_x": 11, "unsat_z": 12, "unsat_x": 13, "legs_z": 14, "legs_x": 15}

FLAG_WG_EDGE_LANES, FLAG_OSD_LDS, FLAG_WG_IDXLOAD = 0x2, 0x20000, 0x40000
FLAG_OSD_REFORDER, FLAG_OSD_QUEUE, FLAG_WG_TABLES = 0x80000, 0x100000, 0x200000
FLAG_WG_VGLOBAL, FLAG_WG_GENERIC, FLAG_OSD_UG, FLAG_OSD_GLOBAL, FLAG_CLOCK_PROBE, FLAG_WG_ROWMAJOR = 0x100, 0x200, 0x400, 0x800, 0x4000, 0x8000
# qldpc_minsum_decode_path: the decoder form a call takes (QLDPC_PATH_*) and the QLDPC_DETAIL_* bits of the workgroup forms
PATH_REGULAR, PATH_RESIDENT, PATH_WG2, PATH_WG, PATH_STREAM, PATH_WAVE = 0, 1, 2, 3, 4, 5
DETAIL_LEAN, DETAIL_REG_INDICES, DETAIL_VGLOBAL, DETAIL_DAMPING, DETAIL_BLOCK_1024, DETAIL_DEG1, DETAIL_NAN_DEG1_ONLY = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40
DETAIL_RES_CDEG8, DETAIL_RES_CPT2 = 0x80, 0x100         # PATH_RESIDENT: the kernel instantiation (with DETAIL_DAMPING)
# qldpc_osd0_last_path: the OSD-0 kernel the last call on a graph handle took (QLDPC_OSD_PATH_*) and its QLDPC_OSD_DETAIL_* bits
OSD_PATH_NONE, OSD_PATH_SMALL, OSD_PATH_GJ, OSD_PATH_GJG, OSD_PATH_REFORDER_LDS, OSD_PATH_REFORDER_UG, OSD_PATH_GLOBAL = -1, 0, 1, 2, 3, 4, 5
OSD_DETAIL_MODE_MASK, OSD_DETAIL_REDO = 0x3, 0x4
# layered decoder: form selectors (results never depend on them) and the bits qldpc_layered_decoder_info reports beside the threads per workgroup
FLAG_LAYERED_BLOCK_256, FLAG_LAYERED_BLOCK_512, FLAG_LAYERED_BLOCK_1024, FLAG_LAYERED_GLOBAL_IDX, FLAG_LAYERED_VGLOBAL = 0x400000, 0x800000, 0x1000000, 0x2000000, 0x4000000
LAYERED_FORM_BLOCK_MASK, LAYERED_FORM_VGLOBAL, LAYERED_FORM_LDS_INDICES = 0xFFFF, 0x10000, 0x20000
# f32 decoder: form selectors (results never depend on them) and the form bit qldpc_minsum32_decoder_info reports
FLAG_F32_GENERIC, FLAG_F32_BLOCK_256, FLAG_F32_BLOCK_512, FLAG_F32_BLOCK_1024 = 0x1000, 0x2000, 0x10000, 0x8000000
F32_FORM_CLEAN = 0x1
CIRCUIT_PHASES = ("sample", "bp_z", "osd_z", "bp_x", "osd_x", "judge")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "qldpc_hip.h")


class QldpcError(RuntimeError):
    pass


class CircuitDesc(C.Structure):
    """qldpc_circuit_desc (include/qldpc_hip.h)."""
    _fields_ = [("base_len", C.c_int64), ("suffix_len", C.c_int64),
                ("base_ops", C.POINTER(C.c_int32)), ("base_q1", C.POINTER(C.c_int32)), ("base_q2", C.POINTER(C.c_int32)),
                ("suffix_ops", C.POINTER(C.c_int32)), ("suffix_q1", C.POINTER(C.c_int32)), ("suffix_q2", C.POINTER(C.c_int32)),
                ("total_qubits", C.c_int32), ("num_x_checks", C.c_int32), ("num_z_checks", C.c_int32), ("n_data", C.c_int32),
                ("k", C.c_int32), ("reserved", C.c_int32),
                ("x_syn_positions", C.POINTER(C.c_int32)), ("x_syn_ptrs", C.POINTER(C.c_int32)),
                ("z_syn_positions", C.POINTER(C.c_int32)), ("z_syn_ptrs", C.POINTER(C.c_int32)),
                ("data_qubit_indices", C.POINTER(C.c_int32)), ("Lx", C.POINTER(C.c_uint8)), ("Lz", C.POINTER(C.c_uint8))]


class NoiseModelStruct(C.Structure):
    """qldpc_noise_model (include/qldpc_hip.h); simulation.noise_model.NoiseModel.as_struct fills it."""
    _fields_ = [("rate", C.c_double * 7), ("idle_w", C.POINTER(C.c_double)), ("cnot_w", C.POINTER(C.c_double))]


class DemDesc(C.Structure):
    """qldpc_dem_desc (include/qldpc_hip.h)."""
    _fields_ = [("n_mech", C.c_int64), ("prob", C.POINTER(C.c_double)), ("n_sectors", C.c_int32), ("k", C.c_int32 * 2), ("n_det", C.c_int32 * 2),
                ("layer_rows", C.c_int32 * 2), ("det_ptr", C.POINTER(C.c_int32) * 2), ("det_idx", C.POINTER(C.c_uint16) * 2),
                ("logmask", C.POINTER(C.c_uint64) * 2)]


_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "double": C.c_double,
            "int8_t": C.c_int8, "uint8_t": C.c_uint8, "uint16_t": C.c_uint16}


def _ctype_of(decl):
    """One C parameter declaration of the header -> ctypes type (opaque handles and void* -> c_void_p)."""
    decl = decl.replace("const", " ").strip()
    stars = decl.count("*") + decl.count("[")
    pname = decl.replace("*", " ").split("[")[0].split()[-1]
    if stars == 1 and pname.startswith("d_"):
        return C.c_void_p              # device pointer (hipMalloc / torch data_ptr()): passed as an address
    base = decl.replace("*", " ").split("[")[0].split()
    base = base[0] if len(base) == 1 else (base[0] if base[0] in _SCALARS or base[0].startswith("qldpc_") or base[0] in ("void", "char") else base[-2])
    if stars == 0:
        return _SCALARS[base]
    if base == "char" and stars == 1:
        return C.c_char_p              # NUL-terminated name
    if base == "qldpc_circuit_desc":
        t = CircuitDesc
    elif base == "qldpc_dem_desc":
        t = DemDesc
    elif base == "qldpc_noise_model":
        t = NoiseModelStruct
    elif base in ("void", "char") or base.startswith("qldpc_"):
        t = None                       # opaque: void*
    else:
        t = _SCALARS[base]
    if t is None:
        return C.c_void_p if stars == 1 else C.POINTER(C.c_void_p)
    for _ in range(stars):
        t = C.POINTER(t)
    return t


def parse_header(path=HEADER_PATH):
    """{name: (restype, [argtypes])} for every function include/qldpc_hip.h declares: the binding is derived from the C ABI itself,
    so a mistyped or missing argument raises ctypes.ArgumentError instead of corrupting memory."""
    import re
    with open(path) as fh:
        text = fh.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    out = {}
    for ret, name, args in re.findall(r"\b(const\s+char\s*\*|int|void)\s*(qldpc_\w+)\s*\(([^;{}]*?)\)\s*;", text):
        ret = ret.replace(" ", "")
        restype = C.c_char_p if ret.startswith("constchar") else (C.c_int if ret == "int" else None)
        args = args.strip()
        argtypes = [] if args in ("", "void") else [_ctype_of(a) for a in args.split(",")]
        out[name] = (restype, argtypes)
    return out


_SIGNATURES = None


def signatures():
    global _SIGNATURES
    if _SIGNATURES is None:
        _SIGNATURES = parse_header()
    return _SIGNATURES


def exports():
    """Names of every function the C ABI declares."""
    return sorted(signatures())


_lib = None
_lock = threading.Lock()


def lib():
    """The loaded C-ABI library.  Raises if it has not been built (python -c 'import __graft_entry__ as g; g.build()')."""
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(SO_PATH):
                    raise QldpcError(f"HIP extension missing: {SO_PATH} (build it with `make -C {os.path.dirname(SO_PATH)}` "
                                     "or __graft_entry__.build()); there is no CPU fallback")
                # Code-capacity plans keep up to eight small pieces in flight on streams of their own; the HIP runtime multiplexes streams onto
                # GPU_MAX_HW_QUEUES hardware queues (default 4), which is what bounds them: [[72,12,6]] at batch 4096 runs 1.0e8 shots/s on 4 queues,
                # 1.4e8 on 16 (profiles/r04f_other_configs.txt).  Read when the HIP runtime initialises, so it only takes effect if nothing in this process
                # has touched the GPU yet; a value the caller exported wins.
                os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
                L = C.CDLL(SO_PATH)
                for name, (restype, argtypes) in signatures().items():
                    fn = getattr(L, name)          # AttributeError here = the library lacks a declared symbol
                    fn.restype = restype
                    fn.argtypes = argtypes
                _lib = L
    return _lib


def check(rc):
    if rc != 0:
        msg = lib().qldpc_last_error()
        raise QldpcError(f"libqldpc_hip error {rc}: {msg.decode() if msg else '?'}")


def device_count():
    return int(lib().qldpc_device_count())


def set_option(name, value):
    """Process-wide kernel-selection switch (include/qldpc_hip.h: qldpc_set_option); results never depend on it.
    Most are read at a launch or at plan creation; "regular_own_search" is read when a Graph is created, so set it before the handle is made;
    "regular_place" and "regular_wave_classes" (next to "regular_own_edges") are read at every fixed-work launch of the regular min-sum kernel's ownership form."""
    check(lib().qldpc_set_option(name.encode(), int(value)))


class Owner:
    """Base of the wrappers that own a C handle in `_h`: the `handle` property, an idempotent close() that calls the class's destroy function
    (`_destroy`, by name) once, and __del__."""
    _destroy = None
    _h = None

    @property
    def handle(self):
        return self._h

    def _destroy_args(self, h):
        return (h,)

    def close(self):
        h = self._h
        if h is not None and h.value:
            self._h = C.c_void_p()
            getattr(lib(), self._destroy)(*self._destroy_args(h))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def device_memory():
    """qldpc_device_memory -> (buffers, bytes): the device allocations the library holds right now (a diagnostic of its own handles' memory)."""
    nb, by = C.c_int64(0), C.c_int64(0)
    check(lib().qldpc_device_memory(C.byref(nb), C.byref(by)))
    return int(nb.value), int(by.value)


class Stream(Owner):
    """A HIP stream of `device` owned by this object (qldpc_stream_*); `.ptr` goes where the ABI takes a `stream`."""
    _destroy = "qldpc_stream_destroy"

    def _destroy_args(self, h):
        return (self.device, h)

    def __init__(self, device=0):
        require_device()
        self.device = int(device)
        self._h = C.c_void_p()
        check(lib().qldpc_stream_create(self.device, C.byref(self._h)))

    @property
    def ptr(self):
        return self._h.value or 0

    def synchronize(self):
        check(lib().qldpc_stream_sync(self.device, self._h))


def require_device():
    if device_count() <= 0:
        raise QldpcError("no HIP device visible: libqldpc_hip runs on MI355X (gfx950) only and has no CPU fallback")


def ptr(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def i8(a):
    return np.ascontiguousarray(a, dtype=np.int8)


def u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def prior_of(prior, n, name="prior", owner="H"):
    """The prior as contiguous f64[n]; ValueError unless it has one entry per column."""
    prior = f64(prior).reshape(-1)
    if prior.size != n:
        raise ValueError(f"{name} has {prior.size} entries, {owner} has {n} columns")
    return prior


def alpha_args(alpha_mode, alpha):
    """Alpha-mode rules of the reference wrappers (src/decoding/sparse.py:18-29,36-39; dense.py:19-33)."""
    if alpha_mode is None:
        mode = ALPHA_DYNAMIC if alpha == 0 else ALPHA_CONST
    elif alpha_mode == "dynamical":
        mode = ALPHA_DYNAMIC
    elif alpha_mode == "alvarado":
        if alpha <= 0:
            raise ValueError("alpha must be > 0 when alpha_mode='alvarado'")
        mode = ALPHA_CONST
    elif alpha_mode == "alvarado-autoregressive":
        mode = ALPHA_SEQ
    else:
        raise ValueError(f"Unsupported alpha_mode: {alpha_mode}")
    if mode == ALPHA_SEQ:
        seq = np.asarray(alpha, dtype=np.float64)
        if seq.ndim != 1 or seq.size == 0:
            raise ValueError("alpha must be a non-empty 1D sequence for alvarado-autoregressive")
        return mode, 0.0, np.ascontiguousarray(seq)
    return mode, float(alpha), np.zeros(1)


class Graph(Owner):
    """Owning wrapper of a qldpc_graph handle (Tanner graph of a parity-check matrix in canonical CSR)."""
    _destroy = "qldpc_graph_destroy"

    def __init__(self, indptr, indices, n, device=0):
        self.indptr, self.indices = i32(indptr), i32(indices)
        self.m, self.n, self.nnz = self.indptr.size - 1, int(n), int(self.indices.size)
        self.device = device
        self._h = C.c_void_p()
        require_device()
        check(lib().qldpc_graph_create(C.c_int(self.m), C.c_int(self.n), ptr(self.indptr, C.c_int32), ptr(self.indices, C.c_int32),
                                       C.c_int(device), C.byref(self._h)))



_graph_cache = OrderedDict()
_GRAPH_CACHE_MAX = 16


def canonical_csr(H):
    """scipy sparse / dense array -> (indptr int32, indices int32 sorted per row, shape)."""
    import scipy.sparse as sp
    if sp.issparse(H):
        c = H.tocsr()
        if not c.has_sorted_indices:
            c = c.sorted_indices()
        if (c.data == 0).any():
            c = c.copy()
            c.eliminate_zeros()
        return c.indptr.astype(np.int32), c.indices.astype(np.int32), c.shape
    H = np.asarray(H)
    m, n = H.shape
    rows, cols = np.nonzero(H)
    indptr = np.zeros(m + 1, np.int32)
    np.add.at(indptr, rows + 1, 1)
    return np.cumsum(indptr, dtype=np.int64).astype(np.int32), cols.astype(np.int32), (m, n)


def graph_for(indptr, indices, n, device=0):
    """Cached Graph for a CSR structure (the reference passes the same H on every trial)."""
    indptr, indices = i32(indptr), i32(indices)
    key = (device, int(n), hashlib.blake2b(indptr.tobytes() + indices.tobytes(), digest_size=16).digest())
    g = _graph_cache.get(key)
    if g is None:
        g = Graph(indptr, indices, n, device)
        _graph_cache[key] = g
        while len(_graph_cache) > _GRAPH_CACHE_MAX:
            _graph_cache.popitem(last=False)
    else:
        _graph_cache.move_to_end(key)
    return g


def minsum_decode_batch(graph, syndromes, prior, max_iter, alpha_mode, alpha, damping=1.0, clip_llr=20.0, flags=0, want_llr=True):
    """qldpc_minsum_decode_batch on host arrays -> (err int8[B,n], conv uint8[B], llr f64[B,n], iters int32[B]).
    want_llr=False leaves the posteriors on the device (llr is returned as None): 9x fewer result bytes over PCIe."""
    mode, aval, seq = alpha_args(alpha_mode, alpha)
    syndromes = i8(syndromes).reshape(-1, graph.m) if graph.m else np.zeros((np.asarray(syndromes).shape[0], 0), np.int8)
    B = syndromes.shape[0]
    prior = prior_of(prior, graph.n, "initialBelief")
    err = np.zeros((B, graph.n), np.int8)
    llr = np.zeros((B, graph.n), np.float64) if want_llr else None
    conv = np.zeros(B, np.uint8)
    iters = np.zeros(B, np.int32)
    check(lib().qldpc_minsum_decode_batch(graph.handle, C.c_int64(B), ptr(syndromes, C.c_int8), ptr(prior, C.c_double),
                                          C.c_int(int(max_iter)), C.c_int(mode), C.c_double(aval), ptr(seq, C.c_double),
                                          C.c_int(seq.size), C.c_double(float(damping)), C.c_double(float(clip_llr)), C.c_int(flags),
                                          ptr(err, C.c_int8), ptr(llr, C.c_double) if want_llr else None, ptr(conv, C.c_uint8),
                                          ptr(iters, C.c_int32)))
    return err, conv, llr, iters


def minsum_decode_path(graph, prior, max_iter, alpha_mode, alpha, damping=1.0, clip_llr=20.0, flags=0):
    """qldpc_minsum_decode_path -> (path, detail): the decoder form minsum_decode_batch takes for these arguments (PATH_*, DETAIL_* bits);
    prior=None asks for the device-pointer entry point, which does not know the prior.  Launches nothing."""
    mode, aval, seq = alpha_args(alpha_mode, alpha)
    if prior is not None:
        prior = prior_of(prior, graph.n, "initialBelief")
    path, detail = C.c_int(-1), C.c_int(0)
    check(lib().qldpc_minsum_decode_path(graph.handle, ptr(prior, C.c_double) if prior is not None else None, C.c_int(int(max_iter)), C.c_int(mode),
                                         C.c_double(aval), ptr(seq, C.c_double), C.c_int(seq.size), C.c_double(float(damping)),
                                         C.c_double(float(clip_llr)), C.c_int(flags), C.byref(path), C.byref(detail)))
    return path.value, detail.value


def osd0_batch(graph, syndromes, llr, hard, ordering=None, flags=0):
    """qldpc_osd0_batch on host arrays: OSD-0 solutions int8[B, n] (performOSD_enhanced with order = 0, osd.py:5-29)."""
    syndromes = i8(syndromes).reshape(-1, graph.m) if graph.m else np.zeros((np.asarray(hard).reshape(-1, graph.n).shape[0], 0), np.int8)
    B = syndromes.shape[0]
    llr, hard = f64(llr).reshape(B, graph.n), i8(hard).reshape(B, graph.n)
    sol = np.zeros((B, graph.n), np.int8)
    op = None
    if ordering is not None:
        ordering = i32(ordering).reshape(B, graph.n)
        op = ptr(ordering, C.c_int32)
    check(lib().qldpc_osd0_batch(graph.handle, B, ptr(syndromes, C.c_int8), ptr(llr, C.c_double), ptr(hard, C.c_int8), op, int(flags), ptr(sol, C.c_int8)))
    return sol


def osd0_last_path(graph):
    """qldpc_osd0_last_path -> (path, detail): the OSD-0 kernel the last OSD-0 call on this graph handle took (OSD_PATH_*, OSD_DETAIL_* bits)."""
    path, detail = C.c_int(-2), C.c_int(0)
    check(lib().qldpc_osd0_last_path(graph.handle, C.byref(path), C.byref(detail)))
    return path.value, detail.value


def osdw_batch(graph, syndromes, llr, hard, order, max_combinations=None, ordering=None):
    """qldpc_osdw_batch on host arrays: performOSD_enhanced(order, max_combinations) (osd.py:5-77) for B shots -> int8[B, n]."""
    syndromes = i8(syndromes).reshape(-1, graph.m)
    B = syndromes.shape[0]
    llr, hard = f64(llr).reshape(B, graph.n), i8(hard).reshape(B, graph.n)
    sol = np.zeros((B, graph.n), np.int8)
    op = None
    if ordering is not None:
        ordering = i32(ordering).reshape(B, graph.n)
        op = ptr(ordering, C.c_int32)
    check(lib().qldpc_osdw_batch(graph.handle, B, ptr(syndromes, C.c_int8), ptr(llr, C.c_double), ptr(hard, C.c_int8), op, int(order),
                                 int(max_combinations or 0), ptr(sol, C.c_int8)))
    return sol


OSDCS_MAX_ORDER = 64


def osdcs_batch(graph, syndromes, llr, hard, weights, order):
    """qldpc_osdcs_batch on host arrays: OSD-0 followed by a combination sweep of `order` (semantics in include/qldpc_hip.h)
    -> (solution int8[B, n], flips int32[B, 2]); flips holds the non-pivot columns the winner flips, -1 padded."""
    order = int(order)
    if not 0 <= order <= OSDCS_MAX_ORDER:
        raise ValueError(f"OSD-CS order must be in 0..{OSDCS_MAX_ORDER}, got {order}")
    syndromes = i8(syndromes).reshape(-1, graph.m) if graph.m else np.zeros((np.asarray(hard).reshape(-1, graph.n).shape[0], 0), np.int8)
    B = syndromes.shape[0]
    llr, hard = f64(llr).reshape(B, graph.n), i8(hard).reshape(B, graph.n)
    weights = f64(weights)
    if weights.size != graph.n:
        raise ValueError(f"weights has {weights.size} entries, H has {graph.n} columns")
    if not np.isfinite(weights).all():
        raise ValueError("weights must be finite")
    sol = np.zeros((B, graph.n), np.int8)
    flips = np.full((B, 2), -1, np.int32)
    check(lib().qldpc_osdcs_batch(graph.handle, B, ptr(syndromes, C.c_int8), ptr(llr, C.c_double), ptr(hard, C.c_int8), ptr(weights, C.c_double),
                                  order, ptr(sol, C.c_int8), ptr(flips, C.c_int32)))
    return sol, flips


LSD_MAX_BITS, LSD_MAX_ROWS = 64, 1024
LSD_DEFAULTS = {"bits_per_step": 1, "max_rows": 512}


def lsd_params(params=None):
    """The argument rule of BP+LSD, before any device call: None or a dict with bits_per_step (1..LSD_MAX_BITS) and / or max_rows (1..LSD_MAX_ROWS) ->
    the complete dict of ints (LSD_DEFAULTS where a key is missing)."""
    p = dict(LSD_DEFAULTS)
    extra = set(params or {}) - set(p)
    if extra:
        raise ValueError(f"unknown LSD parameter(s) {sorted(extra)} (expected {sorted(p)})")
    for k, v in (params or {}).items():
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
            raise ValueError(f"LSD {k} must be an integer, got {v!r}")
        p[k] = int(v)
    if not 1 <= p["bits_per_step"] <= LSD_MAX_BITS:
        raise ValueError(f"LSD bits_per_step must be in 1..{LSD_MAX_BITS}, got {p['bits_per_step']}")
    if not 1 <= p["max_rows"] <= LSD_MAX_ROWS:
        raise ValueError(f"LSD max_rows must be in 1..{LSD_MAX_ROWS}, got {p['max_rows']}")
    return p


def lsd_batch(graph, syndromes, llr, hard, bits_per_step=1, max_rows=512):
    """qldpc_lsd_batch on host arrays: BP+LSD, cluster-local post-processing of the OSD hand-over (semantics in include/qldpc_hip.h)
    -> (solution int8[B, n], info int32[B, 4] = flag, rounds, cluster rows, added columns; flag 1 capped / 2 no candidates: OSD-0's answer)."""
    p = lsd_params({"bits_per_step": bits_per_step, "max_rows": max_rows})
    syndromes = i8(syndromes).reshape(-1, graph.m) if graph.m else np.zeros((np.asarray(hard).reshape(-1, graph.n).shape[0], 0), np.int8)
    B = syndromes.shape[0]
    llr, hard = f64(llr).reshape(B, graph.n), i8(hard).reshape(B, graph.n)
    sol = np.zeros((B, graph.n), np.int8)
    info = np.zeros((B, 4), np.int32)
    check(lib().qldpc_lsd_batch(graph.handle, B, ptr(syndromes, C.c_int8), ptr(llr, C.c_double), ptr(hard, C.c_int8), p["bits_per_step"], p["max_rows"],
                                ptr(sol, C.c_int8), ptr(info, C.c_int32)))
    return sol, info


LSD_STATS = ("clusters", "cols_1", "cols_2", "cols_inf", "llr_1", "llr_2", "llr_inf", "rows_inf")      # the eight words of qldpc_lsd_stats_batch
NO_STATEMENT = np.uint64(0xFFFFFFFFFFFFFFFF)     # every word of a shot LSD ended with flag 1 or 2, and the score of such a trial
CONF_KINDS = {"cols_1": 0, "cols_2": 1, "cols_inf": 2, "llr_1": 3, "llr_2": 4, "llr_inf": 5}            # QLDPC_CONF_*
CONF_MAX_BINS = 4096


def quantise_weights(prior):
    """The default weight table of the cluster statistics: uint16[n] = min(65535, rint(|prior_j| * 256)), NaN -> 65535 (a cluster's W is then its
    prior weight in units of 1 / 256; include/qldpc_hip.h states the same rule at qldpc_lsd_stats_batch)."""
    a = np.abs(f64(prior).ravel())
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.minimum(np.rint(a * 256.0), 65535.0)
    w[np.isnan(a)] = 65535.0
    return w.astype(np.uint16)


def _weights(weights, n, what="weights"):
    """uint16[n] (C order) or None; ValueError for another size or values outside 0..65535"""
    if weights is None:
        return None
    w = np.asarray(weights)
    if w.size != n:
        raise ValueError(f"{what} has {w.size} entries, the graph has {n} columns")
    if w.dtype != np.uint16:
        if w.dtype.kind not in "iu" or (w.size and (w.min() < 0 or w.max() > 65535)):
            raise ValueError(f"{what} must be integers in 0..65535 (quantise_weights turns a prior into them)")
    return np.ascontiguousarray(w.ravel(), np.uint16)


def conf_kind(kind):
    """A confidence kind by name (CONF_KINDS) or number -> the QLDPC_CONF_* number; ValueError otherwise."""
    if isinstance(kind, str) and kind in CONF_KINDS:
        return CONF_KINDS[kind]
    if not isinstance(kind, (bool, np.bool_)) and isinstance(kind, (int, np.integer)) and 0 <= int(kind) < len(CONF_KINDS):
        return int(kind)
    raise ValueError(f"unknown confidence kind {kind!r} (expected one of {sorted(CONF_KINDS)})")


def conf_edges(edges):
    """The bin edges of a confidence histogram: uint64[nbins - 1], strictly increasing, at most CONF_MAX_BINS - 1 of them; ValueError otherwise."""
    if edges is None:
        edges = []
    if isinstance(edges, np.ndarray) and edges.ndim != 1:
        raise ValueError("edges must be a 1-D sequence of integers in 0..2^64 - 1")
    try:                                                                     # through Python integers: a list that holds 2^64 - 1 stays exact
        vals = [int(v) if isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) else None for v in edges]
    except TypeError:
        vals = [None]
    if any(v is None or not 0 <= v < 1 << 64 for v in vals):
        raise ValueError("edges must be a 1-D sequence of integers in 0..2^64 - 1")
    e = np.array(vals, np.uint64)
    if e.size > CONF_MAX_BINS - 1:
        raise ValueError(f"at most {CONF_MAX_BINS - 1} edges ({CONF_MAX_BINS} bins), got {e.size}")
    if e.size > 1 and not (e[1:] > e[:-1]).all():
        raise ValueError("edges must be strictly increasing")
    return e


def lsd_stats_batch(graph, syndromes, llr, hard, bits_per_step=1, max_rows=512, weights=None):
    """qldpc_lsd_stats_batch on host arrays: lsd_batch plus the cluster statistics -> (solution int8[B, n], info int32[B, 4], stats uint64[B, 8]);
    the words of a row are named by LSD_STATS.  weights: uint16[n] (quantise_weights(prior) is the default table) or None (words 4 .. 6 stay 0).
    A shot with flag 1 or 2 has eight NO_STATEMENT words."""
    p = lsd_params({"bits_per_step": bits_per_step, "max_rows": max_rows})
    w = _weights(weights, graph.n)
    syndromes = i8(syndromes).reshape(-1, graph.m) if graph.m else np.zeros((np.asarray(hard).reshape(-1, graph.n).shape[0], 0), np.int8)
    B = syndromes.shape[0]
    llr, hard = f64(llr).reshape(B, graph.n), i8(hard).reshape(B, graph.n)
    sol = np.zeros((B, graph.n), np.int8)
    info = np.zeros((B, 4), np.int32)
    stats = np.zeros((B, 8), np.uint64)
    check(lib().qldpc_lsd_stats_batch(graph.handle, B, ptr(syndromes, C.c_int8), ptr(llr, C.c_double), ptr(hard, C.c_int8), p["bits_per_step"],
                                      p["max_rows"], ptr(w, C.c_uint16) if w is not None else None, ptr(sol, C.c_int8), ptr(info, C.c_int32),
                                      ptr(stats, C.c_uint64)))
    return sol, info, stats


def gf2_spmv_batch(graph, vectors):
    """s = H e over GF(2) for B vectors (qldpc_gf2_spmv_batch, kernels.py:222-231): int8[B, n] -> int8[B, m]."""
    vectors = i8(vectors).reshape(-1, graph.n)
    out = np.zeros((vectors.shape[0], graph.m), np.int8)
    check(lib().qldpc_gf2_spmv_batch(graph.handle, vectors.shape[0], ptr(vectors, C.c_int8), ptr(out, C.c_int8)))
    return out


# Relay-BP defaults: the published gross-code setting (a starting point; qldpc_relay_decode_batch in include/qldpc_hip.h)
RELAY_DEFAULTS = {"alpha": 1.0, "clip_llr": 20.0, "gamma0": 0.125, "gamma_min": -0.24, "gamma_max": 0.66, "t0": 80, "tr": 60, "max_legs": 300,
                  "stop_after": 5}


def relay_params(params, with_clip=True):
    """RELAY_DEFAULTS updated by `params` and validated: ValueError for an unknown name or a value the C ABI rejects."""
    unknown = set(params) - set(RELAY_DEFAULTS)
    if unknown:
        raise ValueError(f"unknown Relay-BP parameter(s): {sorted(unknown)}")
    p = dict(RELAY_DEFAULTS, **params)
    for k in ("alpha", "clip_llr", "gamma0", "gamma_min", "gamma_max"):
        p[k] = float(p[k])
        if not np.isfinite(p[k]):
            raise ValueError(f"{k} must be finite")
    for k in ("t0", "tr", "max_legs", "stop_after"):
        if int(p[k]) != p[k]:
            raise ValueError(f"{k} must be an integer")
        p[k] = int(p[k])
    if p["alpha"] <= 0 or p["clip_llr"] <= 0:
        raise ValueError("alpha and clip_llr must be > 0")
    if p["gamma_min"] > p["gamma_max"]:
        raise ValueError(f"gamma_min ({p['gamma_min']}) > gamma_max ({p['gamma_max']})")
    if p["t0"] < 1 or p["tr"] < 1:
        raise ValueError("t0 and tr must be >= 1")
    if not 0 <= p["max_legs"] < 2 ** 20:
        raise ValueError("max_legs must be in [0, 2**20)")
    if p["stop_after"] < 1:
        raise ValueError("stop_after must be >= 1")
    if not with_clip:
        p.pop("clip_llr")
    return p


def relay_check_inputs(prior, tag):
    """ValueError unless every prior is finite and 0 <= tag <= 15."""
    if not np.all(np.isfinite(prior)):
        raise ValueError("Relay-BP needs a finite prior")
    if int(tag) != tag or not 0 <= int(tag) <= 15:
        raise ValueError("tag must be an integer in 0..15")


def relay_decode_batch(graph, syndromes, prior, seed, shot_begin=0, tag=0, **params):
    """qldpc_relay_decode_batch on host arrays -> (err int8[B, n], conv uint8[B], legs int32[B], iters int32[B], solutions int32[B])."""
    p = relay_params(params)
    prior = prior_of(prior, graph.n)
    relay_check_inputs(prior, tag)
    syndromes = i8(syndromes).reshape(-1, graph.m)
    B = syndromes.shape[0]
    err = np.zeros((B, graph.n), np.int8)
    conv = np.zeros(B, np.uint8)
    legs, iters, sols = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    check(lib().qldpc_relay_decode_batch(graph.handle, C.c_int64(B), ptr(syndromes, C.c_int8), ptr(prior, C.c_double), p["alpha"], p["clip_llr"],
                                         p["gamma0"], p["gamma_min"], p["gamma_max"], p["t0"], p["tr"], p["max_legs"], p["stop_after"],
                                         C.c_uint64(int(seed)), C.c_int64(int(shot_begin)), int(tag), ptr(err, C.c_int8), ptr(conv, C.c_uint8),
                                         ptr(legs, C.c_int32), ptr(iters, C.c_int32), ptr(sols, C.c_int32)))
    return err, conv, legs, iters, sols


# Guided decimation: the starting point of the sweep in tools/kbench_decimation.py (see DESIGN 4.8 for what has been measured); the tests pass every
# parameter explicitly
DECIM_DEFAULTS = {"alpha": 1.0, "clip_llr": 20.0, "t_round": 12, "max_rounds": 32, "per_round": 8, "fix_llr": 50.0}


def decim_params(params, with_clip=True):
    """DECIM_DEFAULTS updated by `params` and validated: ValueError for an unknown name or a value qldpc_decim_decode_batch rejects."""
    unknown = set(params) - set(DECIM_DEFAULTS)
    if unknown:
        raise ValueError(f"unknown decimation parameter(s): {sorted(unknown)}")
    p = dict(DECIM_DEFAULTS, **params)
    for k in ("alpha", "clip_llr", "fix_llr"):
        p[k] = float(p[k])
        if not np.isfinite(p[k]) or p[k] <= 0:
            raise ValueError(f"{k} must be finite and > 0")
    for k in ("t_round", "max_rounds", "per_round"):
        if int(p[k]) != p[k]:
            raise ValueError(f"{k} must be an integer")
        p[k] = int(p[k])
    if p["t_round"] < 1:
        raise ValueError("t_round must be >= 1")
    if not 0 <= p["max_rounds"] < 2 ** 20:
        raise ValueError("max_rounds must be in [0, 2**20)")
    if not 1 <= p["per_round"] <= 64:
        raise ValueError("per_round must be in 1..64")
    if not with_clip:
        p.pop("clip_llr")
    return p


def decim_decode_batch(graph, syndromes, prior, **params):
    """qldpc_decim_decode_batch on host arrays -> (err int8[B, n], llr f64[B, n], conv uint8[B], iters int32[B], rounds int32[B], fixed int32[B])."""
    p = decim_params(params)
    prior = prior_of(prior, graph.n)
    if not np.all(np.isfinite(prior)):
        raise ValueError("guided decimation needs a finite prior")
    syndromes = i8(syndromes).reshape(-1, graph.m)
    B = syndromes.shape[0]
    err, llr = np.zeros((B, graph.n), np.int8), np.zeros((B, graph.n), np.float64)
    conv = np.zeros(B, np.uint8)
    iters, rounds, fixed = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    check(lib().qldpc_decim_decode_batch(graph.handle, C.c_int64(B), ptr(syndromes, C.c_int8), ptr(prior, C.c_double), p["alpha"], p["clip_llr"],
                                         p["t_round"], p["max_rounds"], p["per_round"], p["fix_llr"], ptr(err, C.c_int8), ptr(llr, C.c_double),
                                         ptr(conv, C.c_uint8), ptr(iters, C.c_int32), ptr(rounds, C.c_int32), ptr(fixed, C.c_int32)))
    return err, llr, conv, iters, rounds, fixed


def shotprior_params(alpha=1.0, clip_llr=20.0, max_iter=50):
    """The scalar arguments of qldpc_shotprior_decode_batch, validated: ValueError for a value it rejects -> (alpha, clip_llr, max_iter)."""
    alpha, clip_llr = float(alpha), float(clip_llr)
    for name, v in (("alpha", alpha), ("clip_llr", clip_llr)):
        if not np.isfinite(v) or v <= 0:
            raise ValueError(f"{name} must be finite and > 0")
    if int(max_iter) != max_iter or int(max_iter) < 1:
        raise ValueError("max_iter must be an integer >= 1")
    return alpha, clip_llr, int(max_iter)


def link_tables(links, n):
    """links: None, or an object with ptr / src / llr (simulation.correlated.CorrelationLinks), or a (ptr, src, llr) triple -> contiguous
    (ptr int32[n + 1], src int32[>= 1], llr f64[>= 1], number of links); None gives empty runs.  The rules themselves are checked by the library."""
    if links is None:
        return np.zeros(n + 1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.float64), 0
    lp, ls, ll = (links.ptr, links.src, links.llr) if hasattr(links, "ptr") else links
    lp, ls, ll = i32(lp).ravel(), i32(ls).ravel(), f64(ll).ravel()
    if lp.size != n + 1:
        raise ValueError(f"link ptr has {lp.size} entries, the graph has {n} columns (n + 1 expected)")
    if ls.size != ll.size:
        raise ValueError(f"link src has {ls.size} entries, link llr {ll.size}")
    if ls.size < int(lp[-1]) or int(lp[-1]) < 0:
        raise ValueError(f"link ptr ends at {int(lp[-1])}, the tables hold {ls.size} links")
    nl = int(lp[-1])
    if ls.size == 0:
        ls, ll = np.zeros(1, np.int32), np.zeros(1, np.float64)
    return lp, ls, ll, nl


def shotprior_decode_batch(graph, syndromes, priors, alpha=1.0, clip_llr=20.0, max_iter=50, links=None, src_err=None, want_prior=False):
    """qldpc_shotprior_decode_batch on host arrays: min-sum with the prior priors[n] (every shot) or priors[B, n] (per shot), lowered per shot by the
    `links` (link_tables) whose source fired in src_err int8[B, n_src] -> (err int8[B, n], llr f64[B, n], conv uint8[B], iters int32[B]) and, with
    want_prior, the per-shot prior f64[B, n] the shots were decoded with as a fifth entry."""
    alpha, clip_llr, max_iter = shotprior_params(alpha, clip_llr, max_iter)
    syndromes = i8(syndromes).reshape(-1, graph.m)
    B, n = syndromes.shape[0], graph.n
    priors = f64(priors)
    if priors.shape not in ((n,), (B, n)):
        raise ValueError(f"priors must have shape ({n},) or ({B}, {n}), got {priors.shape}")
    stride = n if priors.ndim == 2 else 0
    if (links is None) != (src_err is None):
        raise ValueError("links and src_err go together")
    if links is not None:
        src_err = i8(src_err)
        if src_err.ndim != 2 or src_err.shape[0] != B:
            raise ValueError(f"src_err must be int8[{B}, n_src], got shape {src_err.shape}")
        n_src = src_err.shape[1]
        lp, ls, ll, _ = link_tables(links, n)
        if src_err.size == 0:
            src_err = np.zeros(1, np.int8)
        tabs = (C.c_int32(n_src), ptr(src_err, C.c_int8), ptr(lp, C.c_int32), ptr(ls, C.c_int32), ptr(ll, C.c_double))
    else:
        tabs = (C.c_int32(0), None, None, None, None)
    err, llr = np.zeros((B, n), np.int8), np.zeros((B, n), np.float64)
    conv, iters = np.zeros(B, np.uint8), np.zeros(B, np.int32)
    pout = np.zeros((B, n), np.float64) if want_prior else None
    check(lib().qldpc_shotprior_decode_batch(graph.handle, C.c_int64(B), ptr(syndromes, C.c_int8), ptr(priors, C.c_double), C.c_int64(stride), *tabs,
                                             alpha, clip_llr, max_iter, ptr(err, C.c_int8), ptr(llr, C.c_double), ptr(conv, C.c_uint8),
                                             ptr(iters, C.c_int32), ptr(pout, C.c_double) if want_prior else None))
    return (err, llr, conv, iters, pout) if want_prior else (err, llr, conv, iters)


def erasure_table_args(tables, n=None, n_locs=None):
    """One sector's erasure tables -- an object with loc_ptr / loc_col / loc_h / lut_ptr / lut (simulation.erasure.ErasureTables) or that 5-tuple ->
    contiguous (loc_ptr int32, loc_col int32[>= 1], loc_h uint8[>= 1], lut_ptr int32, lut f64[>= 1]).  The shapes are checked here (the library reads
    n_locs + 1, loc_ptr[n_locs], n + 1 and lut_ptr[n] entries), the rules themselves by the library."""
    t = tables
    lp, lc, lh, up, lu = (t.loc_ptr, t.loc_col, t.loc_h, t.lut_ptr, t.lut) if hasattr(t, "loc_ptr") else t
    lp, lc, lh, up, lu = i32(lp).ravel(), i32(lc).ravel(), u8(lh).ravel(), i32(up).ravel(), f64(lu).ravel()
    if lp.size < 1 or (n_locs is not None and lp.size != n_locs + 1):
        raise ValueError(f"erasure tables: loc_ptr has {lp.size} entries" + (f", the plan has {n_locs} locations (n_locs + 1 expected)" if n_locs is not None else ""))
    if up.size < 2 or (n is not None and up.size != n + 1):
        raise ValueError(f"erasure tables: lut_ptr has {up.size} entries" + (f", the sector has {n} columns (n + 1 expected)" if n is not None else ""))
    if lc.size != lh.size or lc.size < max(int(lp[-1]), 0):
        raise ValueError(f"erasure tables: loc_ptr ends at {int(lp[-1])}, loc_col holds {lc.size} entries and loc_h {lh.size}")
    if lu.size < max(int(up[-1]), 0):
        raise ValueError(f"erasure tables: lut_ptr ends at {int(up[-1])}, lut holds {lu.size} entries")
    if lc.size == 0:
        lc, lh = np.zeros(1, np.int32), np.ones(1, np.uint8)
    if lu.size == 0:
        lu = np.zeros(1, np.float64)
    return lp, lc, lh, up, lu


def _erasure_table_ptrs(t):
    return ptr(t[0], C.c_int32), ptr(t[1], C.c_int32), ptr(t[2], C.c_uint8), ptr(t[3], C.c_int32), ptr(t[4], C.c_double)


def erasure_priors(erased, tables):
    """qldpc_erasure_priors on host arrays: the herald record erased uint32[B, ceil(n_locs / 32)] and one sector's tables (erasure_table_args) ->
    the per-shot prior f64[B, n]."""
    lp, lc, lh, up, lu = t = erasure_table_args(tables)
    n_locs, n = lp.size - 1, up.size - 1
    erased = np.ascontiguousarray(erased, np.uint32)
    nw = (n_locs + 31) // 32
    if erased.ndim != 2 or erased.shape[1] != nw:
        raise ValueError(f"erased must be uint32[B, {nw}] for {n_locs} locations, got shape {erased.shape}")
    B = erased.shape[0]
    prior = np.zeros((B, n), np.float64)
    if erased.size == 0:
        erased = np.zeros(1, np.uint32)
    p = _erasure_table_ptrs(t)
    check(lib().qldpc_erasure_priors(C.c_int64(B), C.c_int32(n_locs), ptr(erased, C.c_uint32), *p[:3], C.c_int32(n), *p[3:], ptr(prior, C.c_double)))
    return prior


def soft_table_args(tables, n=None, n_meas=None):
    """One sector's soft tables -- an object with meas_col / meas_w / lut_ptr / lut / levels (simulation.soft.SoftTables) or that 5-tuple ->
    (contiguous meas_col int32[>= 1], meas_w int32[>= 1], lut_ptr int32, lut f64[>= 1], levels, n_meas).  The shapes are checked here (the library
    reads n_meas, n + 1 and lut_ptr[n] entries), the rules themselves by the library."""
    t = tables
    mc, mw, up, lu, K = (t.meas_col, t.meas_w, t.lut_ptr, t.lut, t.levels) if hasattr(t, "meas_col") else t
    mc, mw, up, lu = i32(mc).ravel(), i32(mw).ravel(), i32(up).ravel(), f64(lu).ravel()
    if isinstance(K, (bool, np.bool_)) or not isinstance(K, (int, np.integer)):
        raise ValueError(f"soft tables: levels must be an integer, got {K!r}")
    if mc.size != mw.size or (n_meas is not None and mc.size != n_meas):
        raise ValueError(f"soft tables: meas_col has {mc.size} entries and meas_w {mw.size}" + (f", the plan has {n_meas} measurements" if n_meas is not None else ""))
    if up.size < 2 or (n is not None and up.size != n + 1):
        raise ValueError(f"soft tables: lut_ptr has {up.size} entries" + (f", the sector has {n} columns (n + 1 expected)" if n is not None else ""))
    if lu.size < max(int(up[-1]), 0):
        raise ValueError(f"soft tables: lut_ptr ends at {int(up[-1])}, lut holds {lu.size} entries")
    nm = mc.size
    if nm == 0:
        mc, mw = np.full(1, -1, np.int32), np.ones(1, np.int32)
    if lu.size == 0:
        lu = np.zeros(1, np.float64)
    return mc, mw, up, lu, int(K), nm


def _soft_table_ptrs(t):
    return ptr(t[0], C.c_int32), ptr(t[1], C.c_int32), ptr(t[2], C.c_int32), ptr(t[3], C.c_double)


def soft_priors(levels, tables):
    """qldpc_soft_priors on host arrays: the level record uint8[B, n_meas] and one sector's tables (soft_table_args) -> the per-shot prior f64[B, n]."""
    mc, mw, up, lu, K, nm = t = soft_table_args(tables)
    n = up.size - 1
    levels = np.ascontiguousarray(levels, np.uint8)
    if levels.ndim != 2 or levels.shape[1] != nm:
        raise ValueError(f"levels must be uint8[B, {nm}], got shape {levels.shape}")
    B = levels.shape[0]
    prior = np.zeros((B, n), np.float64)
    if levels.size == 0:
        levels = np.zeros(1, np.uint8)
    p = _soft_table_ptrs(t)
    check(lib().qldpc_soft_priors(C.c_int64(B), C.c_int32(K), C.c_int32(nm), ptr(levels, C.c_uint8), *p[:2], C.c_int32(n), *p[2:], ptr(prior, C.c_double)))
    return prior


def check_window_args(layer_rows, window, commit, m=None):
    """ValueError unless window >= 1, 1 <= commit <= window and layer_rows >= 1 (dividing m when m is given) -> the three as ints."""
    for name, v in (("layer_rows", layer_rows), ("window", window), ("commit", commit)):
        if int(v) != v:
            raise ValueError(f"{name} must be an integer")
    layer_rows, window, commit = int(layer_rows), int(window), int(commit)
    if window < 1 or not 1 <= commit <= window:
        raise ValueError(f"need window >= 1 and 1 <= commit <= window (got window={window}, commit={commit})")
    if layer_rows < 1 or (m is not None and (m < 1 or m % layer_rows)):
        raise ValueError(f"layer_rows={layer_rows} does not divide the {m} rows")
    return layer_rows, window, commit


class WindowDecoder(Owner):
    """Owning wrapper of a qldpc_window_decoder (sliding-window min-sum + OSD-0 over the row layers of `graph`; semantics in include/qldpc_hip.h)."""
    _destroy = "qldpc_window_decoder_destroy"

    def __init__(self, graph, layer_rows, window, commit, prior, max_iter=50, alpha_mode="dynamical", alpha=1.0, clip_llr=20.0, flags=0):
        layer_rows, window, commit = check_window_args(layer_rows, window, commit, graph.m)
        mode, aval, seq = alpha_args(alpha_mode, alpha)
        prior = prior_of(prior, graph.n)
        if not np.isfinite(prior).all():
            raise ValueError("sliding-window decoding needs a finite prior")
        self.graph = graph                     # keeps the full graph alive as long as the decoder
        self._h = C.c_void_p()
        check(lib().qldpc_window_decoder_create(graph.handle, layer_rows, window, commit, ptr(prior, C.c_double), int(max_iter), mode, aval,
                                                ptr(seq, C.c_double), seq.size, float(clip_llr), int(flags), C.byref(self._h)))

    def info(self):
        """{windows, graphs (distinct handles), max_rows, max_cols (of the largest window), wg2_windows (windows on the LDS-resident decoder)}"""
        v = [C.c_int(0) for _ in range(5)]
        check(lib().qldpc_window_decoder_info(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("windows", "graphs", "max_rows", "max_cols", "wg2_windows"), (x.value for x in v)))

    def decode(self, syndromes):
        """int8[B, m] -> (err int8[B, n], conv int32[B], iters int32[B], osd int32[B], unsat uint8[B])"""
        syndromes = i8(syndromes).reshape(-1, self.graph.m)
        B = syndromes.shape[0]
        err = np.zeros((B, self.graph.n), np.int8)
        conv, iters, osd = np.zeros(B, np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
        unsat = np.zeros(B, np.uint8)
        check(lib().qldpc_window_decode_batch(self._h, C.c_int64(B), ptr(syndromes, C.c_int8), ptr(err, C.c_int8), ptr(conv, C.c_int32),
                                              ptr(iters, C.c_int32), ptr(osd, C.c_int32), ptr(unsat, C.c_uint8)))
        return err, conv, iters, osd, unsat


def check_layered_args(max_iter, clip_llr):
    """ValueError unless max_iter is an integer >= 1 and clip_llr > 0 -> (int, float)."""
    if int(max_iter) != max_iter or int(max_iter) < 1:
        raise ValueError(f"the layered decoder needs an integer max_iter >= 1, got {max_iter}")
    clip_llr = float(clip_llr)
    if not clip_llr > 0:
        raise ValueError(f"clip_llr must be > 0, got {clip_llr}")
    return int(max_iter), clip_llr


def check_row_layer(row_layer, m):
    """ValueError unless row_layer is m integers >= 0 -> int32[m] (None stays None: the greedy colouring)."""
    if row_layer is None:
        return None
    a = np.asarray(row_layer)
    if a.ndim != 1 or a.size != m:
        raise ValueError(f"layers has shape {a.shape}, H has {m} rows")
    if a.size and not np.issubdtype(a.dtype, np.integer):
        if not np.all(np.isfinite(a.astype(np.float64))) or not np.array_equal(a, np.floor(a.astype(np.float64))):
            raise ValueError("layers must be integers")
    if a.size and (a.min() < 0 or a.max() > np.iinfo(np.int32).max):
        bad = int(np.flatnonzero((a < 0) | (a > np.iinfo(np.int32).max))[0])
        raise ValueError(f"layers[{bad}] = {a[bad]} is outside 0 .. 2^31 - 1")
    return i32(a)


def graph_check_layers(graph):
    """qldpc_check_layers: the greedy colouring of the rows of `graph` -> (row_layer int32[m], number of layers)."""
    lay = np.zeros(max(graph.m, 1), np.int32)
    nl = C.c_int(0)
    check(lib().qldpc_check_layers(graph.handle, ptr(lay, C.c_int32), C.byref(nl)))
    return lay[:graph.m], nl.value


class LayeredDecoder(Owner):
    """Owning wrapper of a qldpc_layered_decoder (normalised min-sum with a layered schedule on `graph`; semantics in include/qldpc_hip.h)."""
    _destroy = "qldpc_layered_decoder_destroy"

    def __init__(self, graph, prior, max_iter=50, alpha_mode="dynamical", alpha=1.0, clip_llr=20.0, layers=None, flags=0):
        max_iter, clip_llr = check_layered_args(max_iter, clip_llr)
        mode, aval, seq = alpha_args(alpha_mode, alpha)
        prior = prior_of(prior, graph.n)
        layers = check_row_layer(layers, graph.m)
        self.graph = graph                     # the decoder keeps a pointer to the graph handle
        self._h = C.c_void_p()
        check(lib().qldpc_layered_decoder_create(graph.handle, ptr(layers, C.c_int32) if layers is not None else None, ptr(prior, C.c_double), max_iter,
                                                 mode, aval, ptr(seq, C.c_double), seq.size, clip_llr, int(flags), C.byref(self._h)))

    def info(self):
        """{layers, max_layer_rows, max_layer_edges, lds_bytes, block (threads per workgroup), v_global, lds_indices}"""
        v = [C.c_int(0) for _ in range(5)]
        check(lib().qldpc_layered_decoder_info(self._h, *[C.byref(x) for x in v]))
        form = v[4].value
        return dict(layers=v[0].value, max_layer_rows=v[1].value, max_layer_edges=v[2].value, lds_bytes=v[3].value, block=form & LAYERED_FORM_BLOCK_MASK,
                    v_global=bool(form & LAYERED_FORM_VGLOBAL), lds_indices=bool(form & LAYERED_FORM_LDS_INDICES))

    def layers(self):
        """the row_layer in use, int32[m]"""
        lay = np.zeros(max(self.graph.m, 1), np.int32)
        check(lib().qldpc_layered_decoder_layers(self._h, ptr(lay, C.c_int32)))
        return lay[:self.graph.m]

    def decode(self, syndromes):
        """int8[B, m] -> (err int8[B, n], conv uint8[B], llr f64[B, n], iters int32[B]): the outputs of minsum_decode_batch"""
        syndromes = i8(syndromes).reshape(-1, self.graph.m)
        B = syndromes.shape[0]
        err, llr = np.zeros((B, self.graph.n), np.int8), np.zeros((B, self.graph.n), np.float64)
        conv, iters = np.zeros(B, np.uint8), np.zeros(B, np.int32)
        check(lib().qldpc_layered_decode_batch(self._h, C.c_int64(B), ptr(syndromes, C.c_int8), ptr(err, C.c_int8), ptr(llr, C.c_double),
                                               ptr(conv, C.c_uint8), ptr(iters, C.c_int32)))
        return err, conv, llr, iters


def check_minsum32_args(max_iter, clip_llr):
    """ValueError unless max_iter is an integer >= 1 and clip_llr is finite and > 0 once rounded to f32 -> (int, float)."""
    if int(max_iter) != max_iter or int(max_iter) < 1:
        raise ValueError(f"the f32 decoder needs an integer max_iter >= 1, got {max_iter}")
    clip_llr = float(clip_llr)
    with np.errstate(over="ignore"):
        c32 = float(np.float32(clip_llr))
    if not (c32 > 0 and np.isfinite(c32)):
        raise ValueError(f"clip_llr must be finite and > 0 as an f32, got {clip_llr}")
    return int(max_iter), clip_llr


class Minsum32Decoder(Owner):
    """Owning wrapper of a qldpc_minsum32_decoder (single-precision flooding min-sum on `graph`; semantics in include/qldpc_hip.h)."""
    _destroy = "qldpc_minsum32_decoder_destroy"

    def __init__(self, graph, prior, max_iter=50, alpha_mode="dynamical", alpha=1.0, clip_llr=20.0, flags=0):
        max_iter, clip_llr = check_minsum32_args(max_iter, clip_llr)
        mode, aval, seq = alpha_args(alpha_mode, alpha)
        prior = prior_of(prior, graph.n)
        self.graph = graph                     # the decoder keeps a pointer to the graph handle
        self._h = C.c_void_p()
        check(lib().qldpc_minsum32_decoder_create(graph.handle, ptr(prior, C.c_double), max_iter, mode, aval, ptr(seq, C.c_double), seq.size, clip_llr,
                                                  int(flags), C.byref(self._h)))

    def info(self):
        """{lds_bytes, block (threads per workgroup), wg_per_cu (resident workgroups per CU, the runtime's occupancy query), clean}"""
        v = [C.c_int(0) for _ in range(4)]
        check(lib().qldpc_minsum32_decoder_info(self._h, *[C.byref(x) for x in v]))
        return dict(lds_bytes=v[0].value, block=v[1].value, wg_per_cu=v[2].value, clean=bool(v[3].value & F32_FORM_CLEAN))

    def decode(self, syndromes):
        """int8[B, m] -> (err int8[B, n], conv uint8[B], llr f64[B, n] (f32 values widened), iters int32[B]): the outputs of minsum_decode_batch"""
        syndromes = i8(syndromes).reshape(-1, self.graph.m)
        B = syndromes.shape[0]
        err, llr = np.zeros((B, self.graph.n), np.int8), np.zeros((B, self.graph.n), np.float64)
        conv, iters = np.zeros(B, np.uint8), np.zeros(B, np.int32)
        check(lib().qldpc_minsum32_decode_batch(self._h, C.c_int64(B), ptr(syndromes, C.c_int8), ptr(err, C.c_int8), ptr(llr, C.c_double),
                                                ptr(conv, C.c_uint8), ptr(iters, C.c_int32)))
        return err, conv, llr, iters


def osd_timers(reset=True):
    """Phase counters of the OSD-0 kernels [0..15] and of the workgroup BP kernel [16..31] (diagnostic build only, see csrc/clocks.h) -> uint64[32]."""
    out = np.zeros(32, np.uint64)
    check(lib().qldpc_osd_timers_read(ptr(out, C.c_uint64), int(reset)))
    return out


class Comm(Owner):
    """RCCL communicator of the tally all-reduce (qldpc_comm_*): `Comm.init_all(ndev)` for one process driving ndev GPUs,
    `Comm.init_rank(nranks, rank, id, device)` for one process per GPU (id = Comm.unique_id() of rank 0, handed over by the launcher)."""
    _destroy = "qldpc_comm_destroy"

    def __init__(self, handle):
        self._h = handle
        nr, nl = C.c_int(0), C.c_int(0)
        check(lib().qldpc_comm_size(self._h, C.byref(nr), C.byref(nl)))
        self.nranks, self.nlocal = nr.value, nl.value

    @staticmethod
    def unique_id():
        buf = np.zeros(128, np.uint8)
        check(lib().qldpc_comm_unique_id(ptr(buf, C.c_uint8)))
        return buf.tobytes()

    @classmethod
    def init_all(cls, ndev, devices=None):
        require_device()
        h = C.c_void_p()
        dv = None if devices is None else ptr(np.ascontiguousarray(devices, np.int32), C.c_int)
        check(lib().qldpc_comm_init_all(int(ndev), dv, C.byref(h)))
        return cls(h)

    @classmethod
    def init_rank(cls, nranks, rank, uid, device):
        require_device()
        h = C.c_void_p()
        buf = np.frombuffer(bytes(uid), np.uint8).copy()
        check(lib().qldpc_comm_init_rank(int(nranks), int(rank), ptr(buf, C.c_uint8), int(device), C.byref(h)))
        return cls(h)

    def allreduce(self, tallies):
        """int64[nlocal, 16] (or [16] when nlocal == 1) -> the sum over all ranks, same shape."""
        t = np.ascontiguousarray(tallies, np.int64).reshape(self.nlocal, TALLY_SLOTS).copy()
        check(lib().qldpc_tally_allreduce(self._h, ptr(t, C.c_int64)))
        return t.reshape(np.shape(tallies))


def cc_sample_decode_tally(graph, L, p, seed, shot_begin, count, max_iter=50, alpha=1.0, alpha_mode="dynamical", damping=1.0,
                           clip_llr=20.0, use_osd=True, flags=0):
    mode, aval, seq = alpha_args(alpha_mode, alpha)
    L = u8(L).reshape(-1, graph.n)
    tally = np.zeros(TALLY_SLOTS, np.int64)
    check(lib().qldpc_cc_sample_decode_tally(graph.handle, C.c_int(L.shape[0]), ptr(L, C.c_uint8), C.c_double(p), C.c_uint64(seed),
                                             C.c_int64(shot_begin), C.c_int64(count), C.c_int(max_iter), C.c_int(mode),
                                             C.c_double(aval), ptr(seq, C.c_double), C.c_int(seq.size), C.c_double(damping),
                                             C.c_double(clip_llr), C.c_int(int(use_osd)), C.c_int(flags), ptr(tally, C.c_int64)))
    return tally


class CodeCapacityPlan(Owner):
    """Asynchronous code-capacity Monte-Carlo plan (qldpc_cc_plan_*): device-resident sample -> decode -> tally."""
    _destroy = "qldpc_cc_plan_destroy"

    def __init__(self, graph, L, p, max_iter=50, alpha=1.0, alpha_mode="dynamical", damping=1.0, clip_llr=20.0, use_osd=True,
                 flags=0, batch=1 << 18, min_launch=0):
        """batch: shots per piece, taken literally (the plan's device buffers hold `batch` shots per piece in flight).  min_launch (extension): let THIS plan
        cut its calls at a larger granule instead -- fewer, larger launches; results never depend on the cut."""
        mode, aval, seq = alpha_args(alpha_mode, alpha)
        L = u8(L).reshape(-1, graph.n)
        self.graph = graph
        self._h = C.c_void_p()
        check(lib().qldpc_cc_plan_create(graph.handle, C.c_int(L.shape[0]), ptr(L, C.c_uint8), C.c_double(p), C.c_int(max_iter),
                                         C.c_int(mode), C.c_double(aval), ptr(seq, C.c_double), C.c_int(seq.size), C.c_double(damping),
                                         C.c_double(clip_llr), C.c_int(int(use_osd)), C.c_int(flags), C.c_int64(batch), C.c_int64(min_launch), C.byref(self._h)))

    def run(self, seed, shot_begin, count, stream=0):
        check(lib().qldpc_cc_plan_run(self._h, C.c_uint64(seed), C.c_int64(shot_begin), C.c_int64(count), C.c_void_p(stream)))

    def read(self, stream=0, clear=False):
        tally = np.zeros(TALLY_SLOTS, np.int64)
        check(lib().qldpc_cc_plan_read(self._h, C.c_void_p(stream), C.c_int(int(clear)), ptr(tally, C.c_int64)))
        return tally

    def first_iteration_time(self):
        """ms spent in the bit-sliced first-iteration kernel since the last kernel_time() (call before it)"""
        ms = C.c_double()
        check(lib().qldpc_cc_plan_first_iteration_time(self._h, C.byref(ms)))
        return ms.value

    def kernel_time(self):
        ms, nl = C.c_double(0), C.c_int64(0)
        check(lib().qldpc_cc_plan_kernel_time(self._h, C.byref(ms), C.byref(nl)))
        return ms.value, nl.value

    def clock(self, stream=0):
        """Shader clock (MHz) held under the last fused decode launch (plan created with FLAG_CLOCK_PROBE)."""
        mhz = C.c_double(0)
        check(lib().qldpc_cc_plan_clock(self._h, C.c_void_p(stream), C.byref(mhz)))
        return float(mhz.value)


def _attr(src, name):
    return src[name] if isinstance(src, dict) else getattr(src, name)


def logical_column_masks(logical_rows, n):
    """k x n logical rows of H*_full (dense 0/1 or (indptr, indices) CSR) -> uint64[n] with bit r = row r."""
    lm = np.zeros(n, np.uint64)
    if isinstance(logical_rows, tuple):
        ip, ix = logical_rows
        for r in range(len(ip) - 1):
            lm[np.asarray(ix[ip[r]:ip[r + 1]], dtype=np.int64)] |= np.uint64(1) << np.uint64(r)
    else:
        M = np.asarray(logical_rows)
        for r in range(M.shape[0]):
            lm[np.flatnonzero(M[r])] |= np.uint64(1) << np.uint64(r)
    return lm


def make_circuit_desc(compiled, Lx, Lz):
    """CompiledCircuit-like object (or dict of its arrays) -> (CircuitDesc, keep-alive dict)."""
    keep = {k: i32(_attr(compiled, k)) for k in ("base_ops", "base_q1", "base_q2", "suffix_ops", "suffix_q1", "suffix_q2", "x_syn_positions",
                                                 "x_syn_ptrs", "z_syn_positions", "z_syn_ptrs", "data_qubit_indices")}
    keep["Lx"], keep["Lz"] = u8(Lx), u8(Lz)
    d = CircuitDesc()
    d.base_len, d.suffix_len = keep["base_ops"].size, keep["suffix_ops"].size
    for k in ("base_ops", "base_q1", "base_q2", "suffix_ops", "suffix_q1", "suffix_q2", "x_syn_positions", "x_syn_ptrs", "z_syn_positions",
              "z_syn_ptrs", "data_qubit_indices"):
        setattr(d, k, ptr(keep[k], C.c_int32))
    d.total_qubits = int(_attr(compiled, "total_qubits"))
    d.num_x_checks, d.num_z_checks = keep["x_syn_ptrs"].size - 1, keep["z_syn_ptrs"].size - 1
    d.n_data, d.k = keep["data_qubit_indices"].size, keep["Lx"].shape[0]
    d.Lx, d.Lz = ptr(keep["Lx"], C.c_uint8), ptr(keep["Lz"], C.c_uint8)
    return d, keep


def circuit_fault_signatures(compiled, Lx, Lz, sector_is_x):
    """(ptr int32[2*L+1], idx uint16[...], logmask uint64[2*L]) of every single-qubit flip at every base-circuit location."""
    require_device()
    d, keep = make_circuit_desc(compiled, Lx, Lz)
    L = keep["base_ops"].size
    sp = np.zeros(2 * L + 1, np.int32)
    lm = np.zeros(2 * L, np.uint64)
    cap = max(1024, 64 * 2 * L)
    idx = np.zeros(cap, np.uint16)
    need = C.c_int64(0)
    check(lib().qldpc_circuit_fault_signatures(C.byref(d), C.c_int(int(sector_is_x)), ptr(sp, C.c_int32), ptr(idx, C.c_uint16), C.c_int64(cap),
                                               ptr(lm, C.c_uint64), C.byref(need)))
    return sp, idx[:need.value].copy(), lm


STATS_CHECK_MESSAGES, STATS_POSTERIOR = 0, 1


class MessageStats(Owner):
    """Device-resident samples of an estimator trial loop (qldpc_msgstats_*): check messages after `iters` decoder iterations
    (alpha.py:119-137, 206-255) or the decoder's final posteriors (scopt.py:80-134), split by the true error bit."""
    _destroy = "qldpc_msgstats_destroy"

    def __init__(self, graph, errors, prior, kind, iters, alpha_mode="dynamical", alpha=1.0, damping=1.0, clip_llr=20.0):
        errors = i8(errors).reshape(-1, graph.n)
        prior = prior_of(prior, graph.n, owner="the graph")
        mode, aval, seq = alpha_args(alpha_mode, alpha)
        rng, fin = np.zeros(2), np.zeros(2, np.int64)
        self._h = C.c_void_p()
        check(lib().qldpc_msgstats_create(graph.handle, C.c_int64(errors.shape[0]), ptr(errors, C.c_int8), ptr(prior, C.c_double),
                                          C.c_int(kind), C.c_int(iters), C.c_int(mode), C.c_double(aval), ptr(seq, C.c_double),
                                          C.c_int(seq.size), C.c_double(damping), C.c_double(clip_llr), ptr(rng, C.c_double),
                                          ptr(fin, C.c_int64), C.byref(self._h)))
        self.range = (float(rng[0]), float(rng[1]))
        self.finite = (int(fin[0]), int(fin[1]))

    def histogram(self, edges):
        """Counts per bin for the two classes, np.histogram's bin rule -> (int64[bins], int64[bins])."""
        edges = f64(edges)
        bins = edges.size - 1
        h0, h1 = np.zeros(bins, np.int64), np.zeros(bins, np.int64)
        check(lib().qldpc_msgstats_histogram(self._h, ptr(edges, C.c_double), C.c_int(bins), ptr(h0, C.c_int64), ptr(h1, C.c_int64)))
        return h0, h1


def pack_events(bits):
    """bool / 0-1 array [count, n_bits] -> bit-packed records uint8[count, ceil(n_bits / 8)], bit d of a record = (rec[d >> 3] >> (d & 7)) & 1 (Stim's b8)."""
    bits = np.asarray(bits)
    if bits.ndim != 2:
        raise ValueError(f"bits must be [count, n_bits], got shape {bits.shape}")
    return np.packbits(bits != 0, axis=1, bitorder="little")


def unpack_bits(packed, n_bits):
    """The inverse of pack_events: uint8[count, >= ceil(n_bits / 8)] -> uint8[count, n_bits] of 0 / 1."""
    packed = np.asarray(packed, np.uint8)
    if packed.ndim != 2 or packed.shape[1] * 8 < n_bits:
        raise ValueError(f"packed must be uint8[count, >= {(n_bits + 7) // 8}], got shape {packed.shape}")
    return np.unpackbits(packed, axis=1, count=int(n_bits), bitorder="little")


FIXED_WEIGHT_MAX, FIXED_WEIGHT_MAX_LOCS = 4096, 524288      # QLDPC_FIXED_WEIGHT_MAX, QLDPC_FIXED_WEIGHT_MAX_LOCS


def check_fixed_weight(weight):
    """The argument rule of use_fixed_weight, before any device call: None or -1 -> -1 (the independent draws); an integer 0..FIXED_WEIGHT_MAX -> int."""
    if weight is None:
        return -1
    if isinstance(weight, (bool, np.bool_)) or not isinstance(weight, (int, np.integer)):
        raise ValueError(f"fixed weight must be an integer (or None), got {weight!r}")
    weight = int(weight)
    if weight < -1:
        raise ValueError(f"fixed weight must be >= 0 (None or -1 switches back), got {weight}")
    return weight


class CircuitPlan(Owner):
    """Circuit-level Monte-Carlo plan (qldpc_circuit_plan_*): Philox fault sampling through precomputed fault signatures,
    decode of both sectors, OSD-0, logical comparison and tally, all on the device."""
    _destroy = "qldpc_circuit_plan_destroy"

    def __init__(self, compiled, Lx, Lz, graph_z, graph_x, prior_z, prior_x, logmask_z, logmask_x, p, max_iter=50, alpha_z=1.0, alpha_x=1.0,
                 alpha_mode="dynamical", damping=1.0, clip_llr=20.0, use_osd=True, flags=0, batch=16384):
        mode, az, sz = alpha_args(alpha_mode, alpha_z)
        _, ax, sx = alpha_args(alpha_mode, alpha_x)
        d, keep = make_circuit_desc(compiled, Lx, Lz)
        pz, px = f64(prior_z), f64(prior_x)
        lz, lx = np.ascontiguousarray(logmask_z, np.uint64), np.ascontiguousarray(logmask_x, np.uint64)
        self.k, self.nsx, self.nsz = d.k, int(keep["x_syn_ptrs"][-1]), int(keep["z_syn_ptrs"][-1])
        self.n_locs = int(d.base_len)                       # fault locations: what use_fixed_weight counts
        self.fixed_weight = None                            # the sampler axis: None = the independent draws, else the weight in force
        self.erasure_rates = None                           # ... and None = no erasure noise, else the rates in force (f64[7] by op code)
        self.noise_model = None                             # ... and None = the plan's own p and uniform Paulis, else the NoiseModel in force
        self.soft_readout = None                            # ... and None = hard measurements, else the simulation.soft.SoftReadout in force
        from .noise.constants import GATE_TO_OPCODE as OP
        base_ops = np.asarray(compiled.base_ops if hasattr(compiled, "base_ops") else compiled["base_ops"])
        self.n_meas = int(np.isin(base_ops, (OP["MeasX"], OP["MeasZ"])).sum())      # what the level record of sample_soft counts
        self.graph_z, self.graph_x = graph_z, graph_x
        self.flags = flags
        self._h = C.c_void_p()
        check(lib().qldpc_circuit_plan_create(C.byref(d), graph_z.handle, graph_x.handle, ptr(pz, C.c_double), ptr(px, C.c_double),
                                              ptr(lz, C.c_uint64), ptr(lx, C.c_uint64), C.c_double(p), C.c_int(max_iter), C.c_int(mode),
                                              C.c_double(az), C.c_double(ax), ptr(sz, C.c_double), C.c_int(sz.size), ptr(sx, C.c_double),
                                              C.c_int(sx.size), C.c_double(damping), C.c_double(clip_llr), C.c_int(int(use_osd)), C.c_int(flags),
                                              C.c_int64(batch), C.byref(self._h)))

    def use_relay(self, **params):
        """Decode both sectors with Relay-BP from now on (one-way; qldpc_circuit_plan_use_relay).  The plan's clip_llr applies."""
        if "clip_llr" in params:
            raise ValueError("a circuit plan's clip_llr is set when the plan is created")
        p = relay_params(params, with_clip=False)
        check(lib().qldpc_circuit_plan_use_relay(self._h, p["alpha"], p["gamma0"], p["gamma_min"], p["gamma_max"], p["t0"], p["tr"], p["max_legs"],
                                                 p["stop_after"]))
        self.relay = p

    def use_osd_cs(self, order):
        """Run OSD-CS of `order` in the OSD stage from now on, with the plan's priors as the weights (one-way; qldpc_circuit_plan_use_osd_cs)."""
        order = int(order)
        if not 0 <= order <= OSDCS_MAX_ORDER:
            raise ValueError(f"OSD-CS order must be in 0..{OSDCS_MAX_ORDER}, got {order}")
        check(lib().qldpc_circuit_plan_use_osd_cs(self._h, order))
        self.osd_cs_order = order

    def use_lsd(self, bits_per_step=1, max_rows=512):
        """Run BP+LSD in the OSD stage from now on (qldpc_circuit_plan_use_lsd; again with new parameters is allowed).  Goes with flooding, the layered
        schedule, guided decimation, f32, correlated, erasure-aware and soft-aware decoding; not with Relay-BP, windows or OSD-CS."""
        p = lsd_params({"bits_per_step": bits_per_step, "max_rows": max_rows})
        check(lib().qldpc_circuit_plan_use_lsd(self._h, p["bits_per_step"], p["max_rows"]))
        self.lsd = p

    def use_confidence(self, kind, edges=None, weight_z=None, weight_x=None):
        """Score every trial from the LSD cluster statistics of its sectors and keep a histogram of (score, outcome) (qldpc_circuit_plan_use_confidence):
        kind by name (CONF_KINDS) or number, edges uint64[nbins - 1] strictly increasing (None: one bin), weights uint16[n] per sector
        (quantise_weights(prior); None goes with the cols_* kinds only).  After use_lsd; again with new arguments clears the histogram."""
        k, e = conf_kind(kind), conf_edges(edges)
        nz, nx = self.graph_z.n, (self.graph_x.n if self.graph_x is not None else 0)
        wz, wx = _weights(weight_z, nz, "weight_z"), (_weights(weight_x, nx, "weight_x") if self.graph_x is not None else None)
        opt = lambda a, t: ptr(a, t) if a is not None and a.size else None      # noqa: E731
        check(lib().qldpc_circuit_plan_use_confidence(self._h, C.c_int(k), C.c_int(e.size + 1), opt(e, C.c_uint64), opt(wz, C.c_uint16), opt(wx, C.c_uint16)))
        self.confidence = {"kind": k, "edges": e}

    def confidence_hist(self, stream=0, clear=False):
        """uint64[nbins, 4]: hist[bin, outcome] of the trials since the last clear, bin = #{edges <= score}, outcome = bit0 z_err | bit1 x_err
        (qldpc_circuit_plan_confidence_read)."""
        if getattr(self, "confidence", None) is None:
            raise QldpcError("the plan has no confidence (use_confidence)")
        hist = np.zeros((self.confidence["edges"].size + 1, 4), np.uint64)
        check(lib().qldpc_circuit_plan_confidence_read(self._h, C.c_void_p(stream), C.c_int(int(clear)), ptr(hist, C.c_uint64)))
        return hist

    def run_scores(self, seed, trial_begin, count, stream=0):
        """run_outcomes() + the score of every trial: (uint8[count], uint64[count]) (qldpc_circuit_plan_run_scores)."""
        out, score = np.zeros(max(int(count), 0), np.uint8), np.zeros(max(int(count), 0), np.uint64)
        check(lib().qldpc_circuit_plan_run_scores(self._h, C.c_uint64(seed), C.c_int64(trial_begin), C.c_int64(count), C.c_void_p(stream),
                                                  ptr(out, C.c_uint8), ptr(score, C.c_uint64)))
        return out, score

    def lsd_counts(self, stream=0, clear=False):
        """int64[2, 3]: the shots per sector that the LSD stage ended with flag 0 (solved in clusters) / 1 (capped) / 2 (no candidates) since the last
        clear (qldpc_circuit_plan_lsd_counts); a row adds up to the sector's OSD tally slot over the same batches."""
        counts = np.zeros((2, 3), np.int64)
        check(lib().qldpc_circuit_plan_lsd_counts(self._h, C.c_void_p(stream), C.c_int(int(clear)), ptr(counts, C.c_int64)))
        return counts

    def use_window(self, window, commit):
        """Decode both sectors window by window from now on: `window` syndrome cycles at a time, the first `commit` of them committed
        (one-way; qldpc_circuit_plan_use_window)."""
        _, window, commit = check_window_args(1, window, commit)
        check(lib().qldpc_circuit_plan_use_window(self._h, window, commit))
        self.window = (window, commit)

    def use_layered(self, layers_z=None, layers_x=None):
        """Run the BP stage of both sectors with the layered schedule from now on (qldpc_circuit_plan_use_layered); layers_*: a row_layer per
        sector, None = the greedy colouring.  Goes with OSD-0 and OSD-CS; not with Relay-BP or windows."""
        lz = check_row_layer(layers_z, self.graph_z.m)
        lx = check_row_layer(layers_x, self.graph_x.m) if self.graph_x is not None else None      # (a one-sector DemPlan has no sector X)
        check(lib().qldpc_circuit_plan_use_layered(self._h, ptr(lz, C.c_int32) if lz is not None else None, ptr(lx, C.c_int32) if lx is not None else None))
        self.layered = True

    def use_f32(self):
        """Run the BP stage of both sectors in single precision from now on (one-way; qldpc_circuit_plan_use_f32) with the plan's priors, alpha table,
        max_iter and clip_llr.  Goes with OSD-0 and OSD-CS; not with Relay-BP, windows, the layered schedule or guided decimation."""
        check(lib().qldpc_circuit_plan_use_f32(self._h))
        self.precision = "f32"

    def use_decimation(self, **params):
        """Run the BP stage of both sectors as BP with guided decimation from now on (qldpc_circuit_plan_use_decimation): alpha, t_round, max_rounds,
        per_round, fix_llr; the plan's clip_llr applies and its max_iter / alpha table are not used by that stage.  Goes with OSD-0 and OSD-CS; not
        with Relay-BP, windows or the layered schedule."""
        if "clip_llr" in params:
            raise ValueError("a circuit plan's clip_llr is set when the plan is created")
        p = decim_params(params, with_clip=False)
        check(lib().qldpc_circuit_plan_use_decimation(self._h, p["alpha"], p["t_round"], p["max_rounds"], p["per_round"], p["fix_llr"]))
        self.decimation = p

    def use_correlated(self, alpha=1.0, links=None, base=None):
        """Decode the two sectors in two passes from now on (qldpc_circuit_plan_use_correlated): sector 0 as constant-alpha min-sum with its own
        prior, then sector 1 with a per-shot prior -- `base` (f64[n_x]; None: the plan's sector-1 prior) lowered to a link's llr wherever the link's
        sector-0 column is in sector 0's correction.  links: a simulation.correlated.CorrelationLinks or (ptr, src, llr); None = no links (the same
        kernel with nothing to raise).  The plan's max_iter and clip_llr apply, its alpha table does not.  Goes with OSD-0, OSD-CS and LSD; with no
        other path; needs two sectors.  Again with new arguments is allowed."""
        alpha = shotprior_params(alpha)[0]
        n_x = self.graph_x.n if self.graph_x is not None else 0                  # (a one-sector DemPlan: the library refuses it)
        lp, ls, ll, nl = link_tables(links, n_x)
        if base is not None:
            base = f64(base).ravel()
            if base.size != n_x:
                raise ValueError(f"base has {base.size} entries, sector 1 has {n_x} columns")
        check(lib().qldpc_circuit_plan_use_correlated(self._h, alpha, ptr(base, C.c_double) if base is not None else None, C.c_int64(nl),
                                                      ptr(lp, C.c_int32), ptr(ls, C.c_int32), ptr(ll, C.c_double)))
        self.correlated = {"alpha": alpha, "links": nl, "base": base is not None}

    def use_fixed_weight(self, weight):
        """Draw exactly `weight` faulty locations (mechanisms of a DemPlan) per trial from now on, uniformly among the subsets of that size
        (qldpc_circuit_plan_use_fixed_weight); None or -1: back to the independent draws.  The sampler axis of the plan: two-way, any number of
        times, and it goes with every other use_* in either order.  run, run_outcomes and sample honour it."""
        weight = check_fixed_weight(weight)
        check(lib().qldpc_circuit_plan_use_fixed_weight(self._h, C.c_int(weight)))
        self.fixed_weight = None if weight < 0 else weight

    def use_erasure_noise(self, rates):
        """Draw heralded erasures on top of the plan's ordinary faults from now on (qldpc_circuit_plan_use_erasure_noise): `rates` is a number (every
        location class) or a dict keyed by the gate names CNOT, PrepX, PrepZ, MeasX, MeasZ, IDLE; None: off again.  The sampler axis, beside
        use_fixed_weight (the two refuse each other): two-way, and it goes with every other use_* in either order.  Circuit plans only."""
        if rates is None:
            check(lib().qldpc_circuit_plan_use_erasure_noise(self._h, None))
            self.erasure_rates = None
            return
        from .simulation.erasure import erasure_rates
        r = erasure_rates(rates)
        check(lib().qldpc_circuit_plan_use_erasure_noise(self._h, ptr(r, C.c_double)))
        self.erasure_rates = r

    def use_noise_model(self, model):
        """Draw the plan's Pauli faults by `model` from now on (qldpc_circuit_plan_use_noise_model): a simulation.noise_model.NoiseModel -- a rate per
        location class and, optionally, weights for the Paulis of a faulty IDLE and of a faulty CNOT; None: back to the plan's own p and uniform
        Paulis.  The sampler axis, beside use_fixed_weight and use_erasure_noise (a model refuses both, and they refuse it): two-way, and it goes
        with every other use_* in either order.  The plan's priors stay what it was created with (NoiseModel.prior_llrs gives the matched ones).
        Circuit plans only."""
        if model is None:
            check(lib().qldpc_circuit_plan_use_noise_model(self._h, None))
            self.noise_model = None
            return
        from .simulation.noise_model import NoiseModel
        if not isinstance(model, NoiseModel):
            raise ValueError(f"use_noise_model takes a simulation.noise_model.NoiseModel (or None), got {model!r}")
        s, keep = model.as_struct()
        check(lib().qldpc_circuit_plan_use_noise_model(self._h, C.byref(s)))
        del keep                                            # (the library copied what it needs)
        self.noise_model = model

    def use_erasure_aware(self, alpha=1.0, tables=None):
        """Decode both sectors with the heralds from now on (qldpc_circuit_plan_use_erasure_aware): constant-alpha min-sum whose prior is computed
        per shot from the sampler's herald record.  tables: (sector Z, sector X), each a simulation.erasure.ErasureTables or its 5-tuple -- what
        erasure_tables_from_circuit returns.  The plan's max_iter and clip_llr apply, its alpha table does not.  Goes with OSD-0, OSD-CS (which still
        scores with the shared prior) and LSD; with no other path; circuit plans only.  Again with new arguments is allowed."""
        alpha = shotprior_params(alpha)[0]
        if tables is None or len(tables) != 2:
            raise ValueError("use_erasure_aware needs the tables of both sectors (simulation.erasure.erasure_tables_from_circuit)")
        ns = [g.n if g is not None else None for g in (self.graph_z, self.graph_x)]
        keep = [erasure_table_args(t, n, self.n_locs) for t, n in zip(tables, ns)]
        check(lib().qldpc_circuit_plan_use_erasure_aware(self._h, alpha, *_erasure_table_ptrs(keep[0]), *_erasure_table_ptrs(keep[1])))
        self.erasure_aware = {"alpha": alpha}

    def use_soft_readout(self, readout):
        """Draw a soft readout per measurement on top of the plan's ordinary faults from now on (qldpc_circuit_plan_use_soft_readout): `readout` is a
        simulation.soft.SoftReadout; None: hard measurements again.  The sampler axis, beside use_fixed_weight, use_erasure_noise and use_noise_model
        (soft readout refuses all three, and they refuse it): two-way, and it goes with every other use_* in either order.  Circuit plans only."""
        if readout is None:
            check(lib().qldpc_circuit_plan_use_soft_readout(self._h, C.c_int32(0), None, None))
            self.soft_readout = None
            return
        from .simulation.soft import SoftReadout
        if not isinstance(readout, SoftReadout):
            raise ValueError(f"use_soft_readout takes a simulation.soft.SoftReadout (or None), got {readout!r}")
        f, k = f64(readout.flip_mass), f64(readout.keep_mass)
        check(lib().qldpc_circuit_plan_use_soft_readout(self._h, C.c_int32(readout.levels), ptr(f, C.c_double), ptr(k, C.c_double)))
        self.soft_readout = readout

    def use_soft_aware(self, alpha=1.0, tables=None):
        """Decode both sectors with the readout levels from now on (qldpc_circuit_plan_use_soft_aware): constant-alpha min-sum whose prior is computed
        per shot from the sampler's level record.  tables: (sector Z, sector X), each a simulation.soft.SoftTables or its 5-tuple -- what
        soft_tables_from_circuit returns.  The plan's max_iter and clip_llr apply, its alpha table does not.  Goes with OSD-0, OSD-CS (which still
        scores with the shared prior) and LSD; with no other path; circuit plans only.  Again with new arguments is allowed."""
        alpha = shotprior_params(alpha)[0]
        if tables is None or len(tables) != 2:
            raise ValueError("use_soft_aware needs the tables of both sectors (simulation.soft.soft_tables_from_circuit)")
        ns = [g.n if g is not None else None for g in (self.graph_z, self.graph_x)]
        keep = [soft_table_args(t, n, self.n_meas) for t, n in zip(tables, ns)]
        if keep[0][4] != keep[1][4]:
            raise ValueError(f"use_soft_aware: the tables of sector Z have {keep[0][4]} levels, those of sector X {keep[1][4]}")
        check(lib().qldpc_circuit_plan_use_soft_aware(self._h, alpha, C.c_int32(keep[0][4]), *_soft_table_ptrs(keep[0]), *_soft_table_ptrs(keep[1])))
        self.soft_aware = {"alpha": alpha, "levels": keep[0][4]}

    def sample_soft(self, seed, trial_begin, count, want_priors=False):
        """sample() plus the level record -> (sparse_z, true_z, sparse_x, true_x, levels uint8[count, n_meas]) and, with want_priors (the soft-aware
        path), the per-shot priors f64[count, n_z], f64[count, n_x] the plan decodes those trials with (qldpc_circuit_plan_sample_soft)."""
        spz, spx = np.zeros((count, self.nsx), np.int8), np.zeros((count, self.nsz), np.int8)
        tz, tx = np.zeros((count, self.k), np.int8), np.zeros((count, self.k), np.int8)
        levels = np.zeros((count, self.n_meas), np.uint8)
        pz = np.zeros((count, self.graph_z.n), np.float64) if want_priors else None
        px = np.zeros((count, self.graph_x.n), np.float64) if want_priors else None
        check(lib().qldpc_circuit_plan_sample_soft(self._h, C.c_uint64(seed), C.c_int64(trial_begin), C.c_int64(count), ptr(spz, C.c_int8),
                                                   ptr(tz, C.c_int8), ptr(spx, C.c_int8), ptr(tx, C.c_int8), ptr(levels, C.c_uint8),
                                                   ptr(pz, C.c_double) if want_priors else None, ptr(px, C.c_double) if want_priors else None))
        return (spz, tz, spx, tx, levels, pz, px) if want_priors else (spz, tz, spx, tx, levels)

    def sample_erasures(self, seed, trial_begin, count, want_priors=False):
        """sample() plus the herald record -> (sparse_z, true_z, sparse_x, true_x, erased uint32[count, ceil(n_locs / 32)]) and, with want_priors (the
        erasure-aware path), the per-shot priors f64[count, n_z], f64[count, n_x] the plan decodes those trials with (qldpc_circuit_plan_sample_erasures)."""
        spz, spx = np.zeros((count, self.nsx), np.int8), np.zeros((count, self.nsz), np.int8)
        tz, tx = np.zeros((count, self.k), np.int8), np.zeros((count, self.k), np.int8)
        erased = np.zeros((count, (self.n_locs + 31) // 32), np.uint32)
        pz = np.zeros((count, self.graph_z.n), np.float64) if want_priors else None
        px = np.zeros((count, self.graph_x.n), np.float64) if want_priors else None
        check(lib().qldpc_circuit_plan_sample_erasures(self._h, C.c_uint64(seed), C.c_int64(trial_begin), C.c_int64(count), ptr(spz, C.c_int8),
                                                       ptr(tz, C.c_int8), ptr(spx, C.c_int8), ptr(tx, C.c_int8), ptr(erased, C.c_uint32),
                                                       ptr(pz, C.c_double) if want_priors else None, ptr(px, C.c_double) if want_priors else None))
        return (spz, tz, spx, tx, erased, pz, px) if want_priors else (spz, tz, spx, tx, erased)

    def run(self, seed, trial_begin, count, stream=0):
        check(lib().qldpc_circuit_plan_run(self._h, C.c_uint64(seed), C.c_int64(trial_begin), C.c_int64(count), C.c_void_p(stream)))

    def run_outcomes(self, seed, trial_begin, count, stream=0):
        """run() + the per-trial verdicts in trial order: uint8[count], bit0 = z_err, bit1 = x_err."""
        out = np.zeros(max(int(count), 0), np.uint8)
        check(lib().qldpc_circuit_plan_run_outcomes(self._h, C.c_uint64(seed), C.c_int64(trial_begin), C.c_int64(count), C.c_void_p(stream),
                                                    ptr(out, C.c_uint8)))
        return out

    def read(self, stream=0, clear=False):
        tally = np.zeros(TALLY_SLOTS, np.int64)
        check(lib().qldpc_circuit_plan_read(self._h, C.c_void_p(stream), C.c_int(int(clear)), ptr(tally, C.c_int64)))
        return tally

    def phase_times(self):
        """({phase: ms summed over the batches since the last call}, batches): hipEvent brackets of sampler / BP / OSD-0 per sector / judge."""
        ms = (C.c_double * len(CIRCUIT_PHASES))()
        nb = C.c_int64(0)
        check(lib().qldpc_circuit_plan_phase_times(self._h, ms, C.byref(nb)))
        return {k: float(ms[i]) for i, k in enumerate(CIRCUIT_PHASES)}, int(nb.value)

    def clock(self, stream=0):
        """Shader clock (MHz) under the sector-Z decode and OSD-0 kernels of the last batch (plan created with FLAG_CLOCK_PROBE)."""
        mhz = (C.c_double * 2)()
        check(lib().qldpc_circuit_plan_clock(self._h, C.c_void_p(stream), mhz))
        return float(mhz[0]), float(mhz[1])

    def sample(self, seed, trial_begin, count):
        """Batched run_trial_fast -> (sparse_z int8[count, nsx], true_z int8[count, k], sparse_x, true_x)."""
        spz, spx = np.zeros((count, self.nsx), np.int8), np.zeros((count, self.nsz), np.int8)
        kz, kx = getattr(self, "ks", (self.k, self.k))                         # (a DemPlan has a k per sector)
        tz, tx = np.zeros((count, kz), np.int8), np.zeros((count, kx), np.int8)
        check(lib().qldpc_circuit_plan_sample(self._h, C.c_uint64(seed), C.c_int64(trial_begin), C.c_int64(count), ptr(spz, C.c_int8),
                                              ptr(tz, C.c_int8), ptr(spx, C.c_int8), ptr(tx, C.c_int8)))
        return spz, tz, spx, tx

    def set_event_layout(self, n_bits, rows0=None, rows1=None):
        """Which bit of an event record every row reads (qldpc_circuit_plan_set_event_layout): rows<s>[r] = the bit of row r of sector s, -1 = the row is
        constant 0, None = a contiguous run at the sector's default base.  Without a call: sector 0's rows, then sector 1's."""
        tabs = []
        for s, (rows, m) in enumerate(((rows0, self.nsx), (rows1, self.nsz))):
            if rows is None or (s == 1 and getattr(self, "n_sectors", 2) == 1):
                tabs.append(None)
                continue
            rows = i32(rows).ravel()
            if rows.size != m:
                raise ValueError(f"rows{s} has {rows.size} entries, sector {s} has {m} rows")
            tabs.append(rows)
        check(lib().qldpc_circuit_plan_set_event_layout(self._h, C.c_int32(int(n_bits)), *(ptr(x, C.c_int32) if x is not None else None for x in tabs)))
        self.event_bits = int(n_bits)

    def _events(self, events):
        """uint8[count, stride] records (C order) of at least ceil(event_bits / 8) bytes each"""
        events = u8(events)
        if events.ndim != 2:
            raise ValueError(f"events must be uint8[count, stride], got shape {events.shape}")
        return events

    def decode_events(self, events, seed=0, shot_begin=0, stream=0, scores=False):
        """Bit-packed records uint8[count, stride] (pack_events) -> (pred0 uint64[count], pred1 uint64[count], flags uint8[count]): the predicted observable
        flips per sector (bit r = observable r) and, per shot, bit 0 / 1 = converged, 2 / 3 = correction does not reproduce the syndrome, 4 / 5 = zero
        syndrome of sector 0 / 1 (qldpc_circuit_plan_decode_events).  A one-sector plan returns zeros for sector 1.  scores=True (a plan with
        use_confidence): a fourth array, the score uint64[count] of every shot (qldpc_circuit_plan_decode_events_scored)."""
        events = self._events(events)
        count = events.shape[0]
        pred0, pred1, flags = np.zeros(count, np.uint64), np.zeros(count, np.uint64), np.zeros(count, np.uint8)
        if scores:
            score = np.zeros(count, np.uint64)
            check(lib().qldpc_circuit_plan_decode_events_scored(self._h, C.c_uint64(seed), C.c_int64(shot_begin), C.c_int64(count), ptr(events, C.c_uint8),
                                                                C.c_int64(events.shape[1]), C.c_void_p(stream), ptr(pred0, C.c_uint64),
                                                                ptr(pred1, C.c_uint64), ptr(flags, C.c_uint8), ptr(score, C.c_uint64)))
            return pred0, pred1, flags, score
        check(lib().qldpc_circuit_plan_decode_events(self._h, C.c_uint64(seed), C.c_int64(shot_begin), C.c_int64(count), ptr(events, C.c_uint8),
                                                     C.c_int64(events.shape[1]), C.c_void_p(stream), ptr(pred0, C.c_uint64), ptr(pred1, C.c_uint64),
                                                     ptr(flags, C.c_uint8)))
        return pred0, pred1, flags

    def decode_events_dev(self, d_events, count, stride, d_pred0, d_pred1, d_flags, seed=0, shot_begin=0, stream=0):
        """decode_events on device addresses (e.g. torch data_ptr()): enqueued on `stream`, nothing synchronised (qldpc_circuit_plan_decode_events_dev)."""
        check(lib().qldpc_circuit_plan_decode_events_dev(self._h, C.c_uint64(seed), C.c_int64(shot_begin), C.c_int64(count), C.c_void_p(d_events),
                                                         C.c_int64(stride), C.c_void_p(stream), C.c_void_p(d_pred0), C.c_void_p(d_pred1), C.c_void_p(d_flags)))

    def unpack_events(self, events):
        """The unpacker alone (qldpc_circuit_plan_unpack_events): records -> (sparse0 int8[count, rows of sector 0], sparse1), the syndromes a decode sees."""
        events = self._events(events)
        count = events.shape[0]
        sp0, sp1 = np.zeros((count, self.nsx), np.int8), np.zeros((count, self.nsz), np.int8)
        check(lib().qldpc_circuit_plan_unpack_events(self._h, C.c_int64(count), ptr(events, C.c_uint8), C.c_int64(events.shape[1]), ptr(sp0, C.c_int8),
                                                     ptr(sp1, C.c_int8)))
        return sp0, sp1


def make_dem_desc(prob, sectors):
    """(prob, [(n_det, k, layer_rows, det_ptr, det_idx, logmask) per sector]) -> (DemDesc, keep-alive dict)."""
    keep = {"prob": f64(prob)}
    d = DemDesc()
    d.n_mech, d.prob, d.n_sectors = keep["prob"].size, ptr(keep["prob"], C.c_double), len(sectors)
    for s, (n_det, k, layer_rows, det_ptr, det_idx, logmask) in enumerate(sectors[:2]):
        keep[s] = (i32(det_ptr), np.ascontiguousarray(det_idx, np.uint16), np.ascontiguousarray(logmask, np.uint64))
        d.n_det[s], d.k[s], d.layer_rows[s] = int(n_det), int(k), int(layer_rows or 0)
        d.det_ptr[s], d.det_idx[s], d.logmask[s] = ptr(keep[s][0], C.c_int32), ptr(keep[s][1], C.c_uint16), ptr(keep[s][2], C.c_uint64)
    return d, keep


class DemPlan(CircuitPlan):
    """A circuit plan whose sampler draws from a detector error model (qldpc_circuit_plan_create_dem): independent mechanisms with a probability each,
    one or two sectors.  `sectors`: per sector (n_det, k, layer_rows, det_ptr, det_idx, logmask) -- the mechanisms projected onto it; graphs, priors,
    logmasks: the decoder's view per sector (same length).  Every use_*, run, run_outcomes, read, sample and close is CircuitPlan's; with one sector
    sample() returns zeros for sector 1 (no detectors) and every X slot of the tally stays 0."""

    def __init__(self, prob, sectors, graphs, priors, logmasks, max_iter=50, alphas=(1.0, 1.0), alpha_mode="dynamical", damping=1.0, clip_llr=20.0,
                 use_osd=True, flags=0, batch=16384):
        nsec = len(sectors)
        if not (len(graphs) == len(priors) == len(logmasks) == nsec):
            raise ValueError(f"the detector error model has {nsec} sector(s): give as many graphs, priors and logmasks")
        d, keep = make_dem_desc(prob, sectors)
        self._h = C.c_void_p()
        g = list(graphs) + [None] * (2 - nsec)
        al = [alpha_args(alpha_mode, alphas[s]) for s in range(2)]               # (mode, value, sequence) per sector
        mode, al = al[0][0], [x[1:] for x in al]
        pri = [f64(x) for x in priors] + [None] * (2 - nsec)
        lms = [np.ascontiguousarray(x, np.uint64) for x in logmasks] + [None] * (2 - nsec)
        nd, ks = [int(x[0]) for x in sectors] + [0, 0], [int(x[1]) for x in sectors] + [0, 0]
        self.n_sectors, self.k, self.ks, self.nsx, self.nsz = nsec, max(ks), (ks[0], ks[1]), nd[0], nd[1]
        self.n_locs = int(d.n_mech)
        self.fixed_weight = None
        self.erasure_rates = None
        self.noise_model = None
        self.soft_readout = None
        self.n_meas = 0
        self.graph_z, self.graph_x = g[0], g[1]
        self.flags = flags
        opt = lambda a, t: ptr(a, t) if a is not None else None
        check(lib().qldpc_circuit_plan_create_dem(C.byref(d), g[0].handle if g[0] is not None else None, g[1].handle if g[1] is not None else None,
                                                  opt(pri[0], C.c_double), opt(pri[1], C.c_double), opt(lms[0], C.c_uint64), opt(lms[1], C.c_uint64),
                                                  C.c_int(max_iter), C.c_int(mode), C.c_double(al[0][0]), C.c_double(al[1][0]), ptr(al[0][1], C.c_double),
                                                  C.c_int(al[0][1].size), ptr(al[1][1], C.c_double), C.c_int(al[1][1].size), C.c_double(damping),
                                                  C.c_double(clip_llr), C.c_int(int(use_osd)), C.c_int(flags), C.c_int64(batch), C.byref(self._h)))
