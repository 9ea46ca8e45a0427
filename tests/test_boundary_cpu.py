"""CPU suite for the boundary: the C-ABI library loads and exports every symbol include/qldpc_hip.h declares, the
Python mirror validates arguments like the reference, and the product path FAILS LOUDLY without a GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "qldpc_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(qldpc_[a-z0-9_]+)\s*\(", text)))


def test_library_exports_every_declared_symbol(L):
    lib = L.lib()
    decl = declared_symbols()
    assert len(decl) >= 20
    for s in decl:
        assert hasattr(lib, s), f"{s} declared in include/qldpc_hip.h but not exported"
    assert L.exports() == decl                      # the binding is derived from the header: every declaration is bound ...
    for s in decl:                                  # ... with its full argument list (a mistyped call raises instead of corrupting memory)
        fn = getattr(lib, s)
        assert fn.argtypes is not None, s
        assert len(fn.argtypes) == len(L.signatures()[s][1])
    out = subprocess.run(["nm", "-D", "--defined-only", L.SO_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert set(decl) <= exported
    assert all(e.startswith("qldpc_") for e in exported if not e.startswith("_")), exported


def test_mistyped_calls_are_rejected(L):
    import ctypes as C
    lib = L.lib()
    with pytest.raises((C.ArgumentError, TypeError)):
        lib.qldpc_graph_dims(C.c_void_p(), 1.5, None, None)           # a float where int* is expected
    with pytest.raises((C.ArgumentError, TypeError)):
        lib.qldpc_osd0_batch(C.c_void_p(), 0, None, None, None, None, None)   # one argument short (flags)
    sig = L.signatures()
    assert sig["qldpc_minsum_decode_batch_dev"][1][2] is C.c_void_p   # device pointers are passed as addresses
    assert sig["qldpc_minsum_decode_batch"][1][2] == C.POINTER(C.c_int8)


def test_version_and_host_helpers(L, oracle):
    import ctypes as C
    assert L.lib().qldpc_version() >= 100
    assert L.device_count() >= 0
    c = np.array([1, 2, 3, 4], np.uint32); k = np.array([5, 6], np.uint32); o = np.zeros(4, np.uint32)
    L.lib().qldpc_philox4x32_10(L.ptr(c, C.c_uint32), L.ptr(k, C.c_uint32), L.ptr(o, C.c_uint32))
    assert np.array_equal(o, oracle.philox(c, k))
    # Random123 known-answer vectors for Philox4x32-10
    for ctr, key, want in (([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
                           ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
                           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
                            [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])):
        assert oracle.philox(ctr, key).tolist() == want


def test_argument_validation_matches_reference(L):
    from qldpc_amd.decoding.sparse import performMinSum_Symmetric_Sparse
    from qldpc_amd.decoding.dense import performMinSum_Symmetric
    H = np.eye(3)
    for fn in (performMinSum_Symmetric_Sparse, performMinSum_Symmetric):
        with pytest.raises(ValueError, match="Unsupported alpha_mode"):
            fn(H, [0, 0, 0], [1.0, 1.0, 1.0], alpha_mode="bogus")
        with pytest.raises(ValueError, match="alpha must be > 0"):
            fn(H, [0, 0, 0], [1.0, 1.0, 1.0], alpha_mode="alvarado", alpha=0)
        with pytest.raises(ValueError, match="non-empty 1D"):
            fn(H, [0, 0, 0], [1.0, 1.0, 1.0], alpha_mode="alvarado-autoregressive", alpha=np.zeros((2, 2)))


def test_no_cpu_fallback(L):
    """Without a GPU the product path must raise, never compute."""
    if L.device_count() > 0:
        pytest.skip("GPU present")
    from qldpc_amd.decoding.sparse import performMinSum_Symmetric_Sparse
    with pytest.raises(L.QldpcError, match="no CPU fallback"):
        performMinSum_Symmetric_Sparse(np.eye(3), [0, 0, 0], [1.0, 1.0, 1.0])
    import ctypes as C
    h = C.c_void_p()
    ip = np.array([0, 1], np.int32); ix = np.array([0], np.int32)
    rc = L.lib().qldpc_graph_create(1, 1, L.ptr(ip, C.c_int32), L.ptr(ix, C.c_int32), 0, C.byref(h))
    assert rc == -2 and b"no CPU fallback" in L.lib().qldpc_last_error()


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "qldpc-branched-off_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dp, f)).read()
                assert "oracle" not in txt.lower(), f"{f} mentions the oracle"


def test_canonical_csr_and_data(L):
    import scipy.sparse as sp
    from qldpc_amd.data import load_code, load_circuit_matrices
    c = load_code("bb144")
    assert c["Hx"].shape == (72, 144) and c["Hx_indptr"][-1] == 432 and c["Lx"].shape == (12, 144)
    assert not ((c["Hx"].astype(int) @ c["Hz"].T.astype(int)) % 2).any()          # CSS commutation
    assert not ((c["Hx"].astype(int) @ c["Lz"].T.astype(int)) % 2).any()
    ip, ix, shape = L.canonical_csr(sp.csr_matrix(c["Hx"]))
    assert np.array_equal(ip, c["Hx_indptr"]) and np.array_equal(ix, c["Hx_indices"])
    ip2, ix2, _ = L.canonical_csr(c["Hx"].astype(float))
    assert np.array_equal(ip2, ip) and np.array_equal(ix2, ix)
    d = load_circuit_matrices("circ144")
    assert tuple(d["HdecZ_shape"]) == (1008, 8785) and d["HdecZ_indptr"][-1] == 30672


def test_cache_key_and_format(tmp_path):
    """the key recipe must reproduce the names of the reference's own cache files (matrix_cache/matrices_<key>.npz)."""
    import qldpc_amd  # noqa: F401
    from qldpc_amd.data import load_code
    from qldpc_amd.utils.caching import compute_cache_key, save_matrices, load_matrices
    for tag, cycles, want in (("bb144", 12, "d63ef327adf94be6"), ("bb72", 6, "61d7ee9cf7e4c9ee")):
        c = load_code(tag)
        key = compute_cache_key(c["Hx"].astype(np.int64), c["Hz"].astype(np.int64), c["Lx"].astype(np.uint8), c["Lz"].astype(np.uint8), cycles, 0.005)
        assert key == want
    M = {"HdecZ": np.eye(3, 5, dtype=int), "HdecX": np.eye(3, 4, dtype=int), "channel_probsZ": np.arange(5) / 10, "channel_probsX": np.arange(4) / 7,
         "HZ_full": np.ones((4, 5), int), "HX_full": np.ones((4, 4), int), "first_logical_rowZ": 3, "first_logical_rowX": 3, "num_cycles": 2, "k": 1}
    path = save_matrices(str(tmp_path), "abc", M)
    assert os.path.basename(path) == "matrices_abc.npz"
    back = load_matrices(str(tmp_path), "abc")
    assert all(np.array_equal(back[k], M[k]) for k in M)
    assert load_matrices(str(tmp_path), "missing") is None


def test_estimator_host_logic_without_gpu(oracle, golden):
    """Host side of the alpha / beta estimators (decoding/_fit.py, alpha.py): fed with range + integer histograms computed from the
    ORACLE's samples (what the device returns), it reproduces the factors the reference fitted (tests/golden/estimators.npz)."""
    import numpy as np
    from conftest import estimator_cases
    import qldpc_amd  # noqa: F401
    from qldpc_amd.decoding.alpha import _alpha_from_stats
    from qldpc_amd.simulation.engine import _estimation_trials

    class HostStats:
        def __init__(self, samples, bits):
            fin = np.isfinite(samples)
            self.s0, self.s1 = samples[fin & (bits == 0)], samples[fin & (bits == 1)]
            self.finite = (self.s0.size, self.s1.size)
            both = np.concatenate([self.s0, self.s1])
            self.range = (float(both.min()), float(both.max()))

        def histogram(self, edges):
            return (np.histogram(self.s0, bins=edges)[0].astype(np.int64), np.histogram(self.s1, bins=edges)[0].astype(np.int64))

    done = 0
    for c in estimator_cases(golden("estimators")):
        if c["kind"] != "alvarado":
            continue
        R = oracle.alpha_messages(c["indptr"], c["indices"], c["n"], c["errors"], c["prior"])
        st = HostStats(R.ravel(), c["errors"][:, np.asarray(c["indices"])].ravel())
        a, r2 = _alpha_from_stats(st, c["bins"])
        assert abs(a - c["out"]["alpha"]) <= 1e-9 and abs(r2 - c["out"]["r2"]) <= 1e-9, c["name"]
        done += 1
    assert done == 3
    # engine.py:230-246: dynamic number of estimation trials unless the caller changed the default of 5000
    assert _estimation_trials(5000, 8785, 0.005) == 500 and _estimation_trials(5000, 144, 0.005) == 2777
    assert _estimation_trials(5000, 10, 0.0001) == 50000 and _estimation_trials(1234, 8785, 0.005) == 1234


def test_circuit_generator_matches_reference_arrays(golden):
    """Host logic, no GPU: BBCodeCircuit (arithmetic neighbour computation) + CompiledCircuit (table-driven lowering) reproduce the arrays the
    REFERENCE's codes/bb_code.py + noise/compiled.py produced for [[72,12,6]] x 6 and [[144,12,12]] x 12 cycles (tests/golden/circ*_noise.npz)."""
    import numpy as np
    import qldpc_amd  # noqa: F401
    from qldpc_amd.data import load_code
    from qldpc_amd.codes.bb_code import BBCodeCircuit
    from qldpc_amd.noise.compiled import CompiledCircuit
    for tag, code in (("circ72", "bb72"), ("circ144", "bb144")):
        g = golden(tag + "_noise")
        c = load_code(code)
        cb = BBCodeCircuit(c["Hx"], c["Hz"], num_cycles=int(g["num_cycles"]), ell=c["ell"], m=c["m_dim"], a_x_powers=c["a_x_powers"],
                           a_y_powers=c["a_y_powers"], b_y_powers=c["b_y_powers"], b_x_powers=c["b_x_powers"])
        comp = CompiledCircuit(cb.get_full_circuit(), cb.cycle * 2, cb.lin_order, cb.data_qubits, cb.Xchecks, cb.Zchecks)
        for k in ("base_ops", "base_q1", "base_q2", "suffix_ops", "suffix_q1", "suffix_q2", "x_syn_positions", "x_syn_ptrs", "z_syn_positions", "z_syn_ptrs",
                  "x_check_indices", "x_check_ptrs", "z_check_indices", "z_check_ptrs", "data_qubit_indices"):
            assert np.array_equal(getattr(comp, k), g[k]), (tag, k)
        for k in ("total_qubits", "num_error_locs", "max_circuit_size", "max_syndromes_x", "max_syndromes_z", "num_x_checks", "num_z_checks"):
            assert int(getattr(comp, k)) == int(g[k]), (tag, k)


def test_bench_launcher_fails_loudly():
    """bench.py --gpus N: a WORLD_SIZE that disagrees is an error (it used to run one rank silently), and with WORLD_SIZE unset the parent
    starts N ranks itself -- on this GPU-less box every rank fails with "no HIP device" and the parent passes the failure on."""
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=dict(env, WORLD_SIZE="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--gpus 2 but WORLD_SIZE=1" in r.stderr
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    if _lib.device_count() > 0:
        pytest.skip("GPU present: the self-launch is exercised by the -m gpu suite")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and r.stderr.count("no HIP device") >= 1 and "{" not in r.stdout


def test_bench_plain_and_full_arguments():
    """A plain bench run is the headline leg alone; every other leg needs --full, and asking for one without it is an error, not a silent no-op."""
    import bench
    a = bench.parse_args(["--steps", "7", "--warmup", "3", "--dump-outputs", "d"])
    assert (a.steps, a.warmup, a.dump_outputs, a.full) == (7, 3, "d", False)
    assert (a.legs, a.circuit, a.no_cpu_baseline) == ("fixed", "none", True)
    f = bench.parse_args(["--full"])
    assert (f.legs, f.circuit, f.no_cpu_baseline) == ("both", "circ144", False)
    assert bench.parse_args(["--full", "--circuit", "circ72", "--p-sweep", "0.004"]).circuit == "circ72"
    assert bench.parse_args(["--circuit", "none"]).circuit == "none"
    for bad in (["--p-sweep", "0.004"], ["--circuit", "circ72"], ["--no-code-capacity"], ["--steps", "0"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)


def test_collective_device_rule():
    """RCCL reduces device tensors, gloo host tensors: one rule for the tally all-reduce and the verdict gather."""
    import qldpc_amd  # noqa: F401
    from qldpc_amd import parallel
    import torch
    assert parallel.collective_device("gloo") == torch.device("cpu")
    assert parallel.collective_device("gloo", 3) == torch.device("cpu")
    assert parallel.collective_device("nccl", 3) == torch.device("cuda", 3)
    os.environ["LOCAL_RANK"] = "5"
    try:
        assert parallel.local_device() == 5 and parallel.local_device(2) == 2
    finally:
        del os.environ["LOCAL_RANK"]
    assert parallel.local_device() == 0


def test_flag_constants_follow_the_header():
    """Every QLDPC_FLAG_* of include/qldpc_hip.h has a `_lib.FLAG_*` twin with the same value (and no two public flags share a bit)."""
    import re
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    with open(_lib.HEADER_PATH) as fh:
        defs = dict(re.findall(r"#define\s+QLDPC_FLAG_(\w+)\s+(0x[0-9a-fA-F]+)", fh.read()))
    assert len(defs) >= 16
    seen = {}
    for name, val in defs.items():
        v = int(val, 16)
        assert getattr(_lib, "FLAG_" + name) == v, name
        assert v & (v - 1) == 0 and v not in seen, (name, seen.get(v))
        assert v < 0x10000000                      # the public mask (csrc/launchers.h: QLDPC_FLAG_PUBLIC_MASK)
        seen[v] = name


def test_path_and_detail_constants_follow_the_header():
    """Every QLDPC_PATH_* / QLDPC_DETAIL_* of include/qldpc_hip.h (qldpc_minsum_decode_path) has a `_lib.PATH_*` / `_lib.DETAIL_*` twin with the same
    value, and the other way round; paths are distinct small integers, detail bits distinct single bits."""
    import re
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    with open(_lib.HEADER_PATH) as fh:
        text = fh.read()
    paths = {k: int(v) for k, v in re.findall(r"#define\s+QLDPC_PATH_(\w+)\s+(\d+)\b", text)}
    bits = {k: int(v, 16) for k, v in re.findall(r"#define\s+QLDPC_DETAIL_(\w+)\s+(0x[0-9a-fA-F]+)", text)}
    assert set(paths) == {"REGULAR", "RESIDENT", "WG2", "WG", "STREAM", "WAVE"} and sorted(paths.values()) == list(range(6))
    assert len(bits) == 9 and all(v & (v - 1) == 0 and v for v in bits.values()) and len(set(bits.values())) == 9
    # the seven bits of the workgroup forms keep their values; the two of the resident kernel lie above them
    assert [bits[k] for k in ("LEAN", "REG_INDICES", "VGLOBAL", "DAMPING", "BLOCK_1024", "DEG1", "NAN_DEG1_ONLY")] == [1 << i for i in range(7)]
    assert sorted(k for k, v in bits.items() if v > 0x40) == ["RES_CDEG8", "RES_CPT2"]
    for name, v in paths.items():
        assert getattr(_lib, "PATH_" + name) == v, name
    for name, v in bits.items():
        assert getattr(_lib, "DETAIL_" + name) == v, name
    assert {k[5:] for k in vars(_lib) if k.startswith("PATH_")} == set(paths)
    assert {k[7:] for k in vars(_lib) if k.startswith("DETAIL_")} == set(bits)
