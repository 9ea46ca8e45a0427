"""The host-pointer entry points on the MI355X, as far as their staging goes (csrc/common.h, HostStage): batch sizes that make no region a multiple of the
alignment, an empty batch, optional arguments given and omitted, the graph handle's grow-only slab reused by three decoders in turn, every host entry
against its device-pointer twin on the same inputs (the kernels are the same on both sides, so a difference is a staging fault) and against the CPU
oracle where it has the function.  Everything runs on the 3 x 7 Hamming matrix, which every entry here accepts, and on a matrix without rows where
the entry accepts one; a call takes milliseconds."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

pytestmark = pytest.mark.gpu

IP = np.array([0, 4, 8, 12], np.int32)
IX = np.array([0, 2, 4, 6, 1, 2, 5, 6, 3, 4, 5, 6], np.int32)
M, N = 3, 7
PRIOR = np.array([2.0, 2.25, 1.5, 3.0, 2.75, 1.75, 2.5])
SIZES = (1, 3)                                                    # 1 x 7 and 3 x 7 bytes, doubles and words: no region is a multiple of 256 bytes
RELAY = dict(t0=5, tr=4, max_legs=3, stop_after=1)
DECIM = dict(alpha=1.0, clip_llr=20.0, t_round=3, max_rounds=3, per_round=2, fix_llr=50.0)
NULL = C.c_void_p(0)
ERR_INVALID = -1                                                  # QLDPC_ERR_INVALID of include/qldpc_hip.h


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


@pytest.fixture(scope="module")
def shots(oracle):
    """nine syndromes (single errors, double errors, one all-zero), decoded once by the oracle: (synd, err, conv, llr, iters), read-only"""
    rng = np.random.default_rng(20261019)
    E = np.zeros((9, N), np.int8)
    for b in range(8):
        E[b, rng.choice(N, 1 + b % 2, replace=False)] = 1
    synd = np.array([oracle.syndrome_check(IP, IX, e) for e in E])
    ref = oracle.minsum_decode_batch(IP, IX, N, synd, PRIOR, max_iter=10)
    out = (synd, E) + tuple(ref)
    for a in out:
        a.setflags(write=False)
    return out


def fresh(L):
    return L.Graph(IP, IX, N)


def empty(L):
    return L.Graph(np.zeros(1, np.int32), np.zeros(0, np.int32), 4)


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                               # a copy: the shared shots are read-only


def same(a, b, what=""):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if x is None or y is None:
            assert x is None and y is None, what
            continue
        x, y = np.asarray(x), np.asarray(y)
        assert x.dtype == y.dtype and x.shape == y.shape, what
        assert np.array_equal(x, y, equal_nan=(x.dtype.kind == "f")), what


def minsum(L, g, synd, want_llr=True):
    return L.minsum_decode_batch(g, synd, PRIOR if g.n == N else np.array([1.0, -2.0, 0.0, 3.0]), 10, "dynamical", 1.0, want_llr=want_llr)


def relay(L, g, synd):
    return L.relay_decode_batch(g, synd, PRIOR, 77, 3, 1, **RELAY)


def decim(L, g, synd):
    return L.decim_decode_batch(g, synd, PRIOR, **DECIM)


def test_minsum_sizes_null_llr_device_twin_and_oracle(L, shots):
    synd = shots[0]
    g = fresh(L)
    for B in SIZES:
        got = minsum(L, g, synd[:B])
        same(got, [a[:B] for a in shots[2:]], f"B={B}")
        e, c, l, it = minsum(L, g, synd[:B], want_llr=False)
        assert l is None
        same((e, c, it), (got[0], got[1], got[3]), f"B={B} without llr")
    e, c, l, it = minsum(L, g, synd[:0])
    assert e.shape == (0, N) and c.shape == (0,) and l.shape == (0, N) and it.shape == (0,)
    B = 3
    de, dl = torch.zeros((B, N), dtype=torch.int8, device="cuda"), torch.zeros((B, N), dtype=torch.float64, device="cuda")
    dc, di = torch.zeros(B, dtype=torch.uint8, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
    ds, dp = dev(synd[:B]), dev(PRIOR)
    L.check(L.lib().qldpc_minsum_decode_batch_dev(g.handle, C.c_int64(B), ds.data_ptr(), dp.data_ptr(), 10, L.ALPHA_DYNAMIC, C.c_double(1.0), None, 0,
                                                  C.c_double(1.0), C.c_double(20.0), 0, de.data_ptr(), dl.data_ptr(), dc.data_ptr(), di.data_ptr(), NULL))
    torch.cuda.synchronize()
    same(minsum(L, g, synd[:B]), [t.cpu().numpy() for t in (de, dc, dl, di)], "device twin")
    g0 = empty(L)                                                              # no rows: every shot converges at iteration 0 with the prior
    for B in SIZES:
        e, c, l, it = minsum(L, g0, np.zeros((B, 0), np.int8))
        assert c.all() and (it == 0).all() and np.array_equal(l, np.tile([1.0, -2.0, 0.0, 3.0], (B, 1))) and np.array_equal(e, np.tile([0, 1, 0, 0], (B, 1)))
        e2, c2, l2, it2 = minsum(L, g0, np.zeros((B, 0), np.int8), want_llr=False)
        assert l2 is None and np.array_equal(e2, e) and np.array_equal(c2, c) and np.array_equal(it2, it)


def test_grow_only_slab_shared_by_three_decoders(L, shots):
    """B = 5, 1, 9 on ONE handle, the three users of its slab interleaved: every result is the one a fresh handle gives, bit for bit"""
    synd = shots[0]
    g = fresh(L)
    calls = (minsum, relay, decim)
    for k, B in enumerate((5, 1, 9)):
        for j in range(3):
            fn = calls[(j + k) % 3]
            same(fn(L, g, synd[:B]), fn(L, fresh(L), synd[:B]), f"{fn.__name__} B={B}")
    same(minsum(L, g, synd), shots[2:], "min-sum after the others")


def test_relay_and_decimation_sizes_and_device_twins(L, shots):
    synd = shots[0]
    g = fresh(L)
    nine_r, nine_d = relay(L, fresh(L), synd), decim(L, fresh(L), synd)
    for B in SIZES:                                                            # shots are independent: a batch is a prefix of a longer one
        same(relay(L, g, synd[:B]), [a[:B] for a in nine_r], f"Relay-BP B={B}")
        same(decim(L, g, synd[:B]), [a[:B] for a in nine_d], f"decimation B={B}")
    assert [a.shape for a in relay(L, g, synd[:0])] == [(0, N), (0,), (0,), (0,), (0,)]
    assert [a.shape for a in decim(L, g, synd[:0])] == [(0, N), (0, N), (0,), (0,), (0,), (0,)]
    B = 3
    ds, dp = dev(synd[:B]), dev(PRIOR)
    p = dict(L.RELAY_DEFAULTS, **RELAY)
    out = (torch.zeros((B, N), dtype=torch.int8, device="cuda"), torch.zeros(B, dtype=torch.uint8, device="cuda")) + tuple(
        torch.zeros(B, dtype=torch.int32, device="cuda") for _ in range(3))
    L.check(L.lib().qldpc_relay_decode_batch_dev(g.handle, B, ds.data_ptr(), dp.data_ptr(), p["alpha"], p["clip_llr"], p["gamma0"], p["gamma_min"],
                                                 p["gamma_max"], p["t0"], p["tr"], p["max_legs"], p["stop_after"], C.c_uint64(77), 3, 1,
                                                 *[t.data_ptr() for t in out], NULL))
    torch.cuda.synchronize()
    same(relay(L, g, synd[:B]), [t.cpu().numpy() for t in out], "Relay-BP device twin")
    out = (torch.zeros((B, N), dtype=torch.int8, device="cuda"), torch.zeros((B, N), dtype=torch.float64, device="cuda"),
           torch.zeros(B, dtype=torch.uint8, device="cuda")) + tuple(torch.zeros(B, dtype=torch.int32, device="cuda") for _ in range(3))
    L.check(L.lib().qldpc_decim_decode_batch_dev(g.handle, B, ds.data_ptr(), dp.data_ptr(), DECIM["alpha"], DECIM["clip_llr"], DECIM["t_round"],
                                                 DECIM["max_rounds"], DECIM["per_round"], DECIM["fix_llr"], *[t.data_ptr() for t in out], NULL))
    torch.cuda.synchronize()
    same(decim(L, g, synd[:B]), [t.cpu().numpy() for t in out], "decimation device twin")


def test_osd0_and_osdw_orderings_sizes_and_oracle(L, oracle, shots):
    synd, _, hard, _, llr, _ = shots
    g = fresh(L)
    order = np.array([oracle.argsort_abs(x)[::-1] for x in llr]).astype(np.int32)             # some other order than the default one
    for B in SIZES:
        for o in (None, order[:B]):
            ref0 = np.array([oracle.osd0(IP, IX, N, synd[b], llr[b], hard[b], None if o is None else o[b]) for b in range(B)])
            assert np.array_equal(L.osd0_batch(g, synd[:B], llr[:B], hard[:B], ordering=o), ref0)
            ref2 = np.array([oracle.osdw(IP, IX, N, synd[b], llr[b], hard[b], 2, None, None if o is None else o[b]) for b in range(B)])
            assert np.array_equal(L.osdw_batch(g, synd[:B], llr[:B], hard[:B], 2, ordering=o), ref2)
    assert L.osd0_batch(g, synd[:0], llr[:0], hard[:0]).shape == (0, N)
    assert L.osdw_batch(g, synd[:0], llr[:0], hard[:0], 2).shape == (0, N)
    B = 3
    for o in (None, order[:B]):
        dsol = torch.zeros((B, N), dtype=torch.int8, device="cuda")
        ds, dl, dh = dev(synd[:B]), dev(llr[:B]), dev(hard[:B])
        do = None if o is None else dev(o)
        L.check(L.lib().qldpc_osd0_batch_dev(g.handle, C.c_int64(B), ds.data_ptr(), dl.data_ptr(), dh.data_ptr(), None if o is None else do.data_ptr(), None,
                                             None, 0, dsol.data_ptr(), NULL))
        torch.cuda.synchronize()
        assert np.array_equal(L.osd0_batch(g, synd[:B], llr[:B], hard[:B], ordering=o), dsol.cpu().numpy())


def test_osdcs_spmv_sizes_and_device_twins(L, oracle, shots):
    synd, E, hard, _, llr, _ = shots
    g = fresh(L)
    nine = L.osdcs_batch(fresh(L), synd, llr, hard, PRIOR, 3)
    for B in SIZES:
        same(L.osdcs_batch(g, synd[:B], llr[:B], hard[:B], PRIOR, 3), [a[:B] for a in nine], f"OSD-CS B={B}")
        assert np.array_equal(L.gf2_spmv_batch(g, E[:B]), synd[:B])
    sol, flips = L.osdcs_batch(g, synd[:0], llr[:0], hard[:0], PRIOR, 3)
    assert sol.shape == (0, N) and flips.shape == (0, 2) and L.gf2_spmv_batch(g, E[:0]).shape == (0, M)
    for b in range(9):
        assert np.array_equal(oracle.syndrome_check(IP, IX, nine[0][b]), synd[b])              # every solution satisfies its syndrome (the code has full rank)
    B = 3
    ds, dl, dh, dw = dev(synd[:B]), dev(llr[:B]), dev(hard[:B]), dev(PRIOR)
    dsol, dfl = torch.zeros((B, N), dtype=torch.int8, device="cuda"), torch.zeros((B, 2), dtype=torch.int32, device="cuda")
    L.check(L.lib().qldpc_osdcs_batch_dev(g.handle, C.c_int64(B), ds.data_ptr(), dl.data_ptr(), dh.data_ptr(), dw.data_ptr(), 3, None, None, dsol.data_ptr(),
                                          dfl.data_ptr(), NULL))
    torch.cuda.synchronize()
    same(L.osdcs_batch(g, synd[:B], llr[:B], hard[:B], PRIOR, 3), (dsol.cpu().numpy(), dfl.cpu().numpy()), "OSD-CS device twin")
    dv, dout = dev(E[:B]), torch.zeros((B, M), dtype=torch.int8, device="cuda")
    L.check(L.lib().qldpc_gf2_spmv_batch_dev(g.handle, C.c_int64(B), dv.data_ptr(), dout.data_ptr(), NULL))
    torch.cuda.synchronize()
    assert np.array_equal(L.gf2_spmv_batch(g, E[:B]), dout.cpu().numpy())
    g0 = empty(L)
    h0 = np.array([[0, 1, 0, 0], [1, 1, 0, 1], [0, 0, 0, 0]], np.int8)
    for B in SIZES:
        sol, flips = L.osdcs_batch(g0, np.zeros((B, 0), np.int8), np.ones((B, 4)), h0[:B], np.ones(4), 3)
        assert np.array_equal(sol, h0[:B]) and (flips == -1).all()
        assert L.gf2_spmv_batch(g0, h0[:B]).shape == (B, 0)


def test_decoder_objects_sizes_and_device_twins(L, shots):
    """layered, f32 and sliding-window decoders (one layer, one window: the Hamming matrix has no layer structure)"""
    synd = shots[0]
    g = fresh(L)
    B = 3
    for make, what in ((lambda: L.LayeredDecoder(g, PRIOR, max_iter=10), "layered"), (lambda: L.Minsum32Decoder(g, PRIOR, max_iter=10), "f32")):
        dec = make()
        nine = dec.decode(synd)
        for b in SIZES:
            same(dec.decode(synd[:b]), [a[:b] for a in nine], f"{what} B={b}")
        assert [a.shape for a in dec.decode(synd[:0])] == [(0, N), (0,), (0, N), (0,)]
        ds = dev(synd[:B])
        de, dl = torch.zeros((B, N), dtype=torch.int8, device="cuda"), torch.zeros((B, N), dtype=torch.float64, device="cuda")
        dc, di = torch.zeros(B, dtype=torch.uint8, device="cuda"), torch.zeros(B, dtype=torch.int32, device="cuda")
        fn = L.lib().qldpc_layered_decode_batch_dev if what == "layered" else L.lib().qldpc_minsum32_decode_batch_dev
        L.check(fn(dec.handle, C.c_int64(B), ds.data_ptr(), de.data_ptr(), dl.data_ptr(), dc.data_ptr(), di.data_ptr(), NULL))
        torch.cuda.synchronize()
        same(dec.decode(synd[:B]), [t.cpu().numpy() for t in (de, dc, dl, di)], f"{what} device twin")
        dec.close()
    dec = L.WindowDecoder(g, 3, 1, 1, PRIOR, max_iter=10)
    nine = dec.decode(synd)
    for b in SIZES:
        same(dec.decode(synd[:b]), [a[:b] for a in nine], f"window B={b}")
    assert [a.shape for a in dec.decode(synd[:0])] == [(0, N), (0,), (0,), (0,), (0,)]
    ds, de, du = dev(synd[:B]), torch.zeros((B, N), dtype=torch.int8, device="cuda"), torch.zeros(B, dtype=torch.uint8, device="cuda")
    dc, di, dq = (torch.zeros(B, dtype=torch.int32, device="cuda") for _ in range(3))
    L.check(L.lib().qldpc_window_decode_batch_dev(dec.handle, C.c_int64(B), ds.data_ptr(), de.data_ptr(), dc.data_ptr(), di.data_ptr(), dq.data_ptr(),
                                                  du.data_ptr(), NULL))
    torch.cuda.synchronize()
    same(dec.decode(synd[:B]), [t.cpu().numpy() for t in (de, dc, di, dq, du)], "window device twin")
    dec.close()


def test_message_statistics_sizes(L, shots):
    """qldpc_msgstats_create / _histogram: the posteriors of B trials, their range, their counts by error bit and a histogram"""
    synd, E, _, _, llr, _ = shots
    g = fresh(L)
    for B in SIZES + (0,):
        st = L.MessageStats(g, E[:B], PRIOR, L.STATS_POSTERIOR, 10)
        x, bit = llr[:B].ravel(), E[:B].ravel()
        fin = np.isfinite(x)
        assert st.finite == (int((fin & (bit == 0)).sum()), int((fin & (bit == 1)).sum()))
        assert st.range == ((float(x[fin].min()), float(x[fin].max())) if fin.any() else (0.0, 0.0))
        edges = np.linspace(-25.0, 25.0, 8)
        h0, h1 = st.histogram(edges)
        assert np.array_equal(h0, np.histogram(x[fin & (bit == 0)], edges)[0]) and np.array_equal(h1, np.histogram(x[fin & (bit == 1)], edges)[0])
        st.close()
    st = L.MessageStats(g, E[:3], PRIOR, L.STATS_CHECK_MESSAGES, 2)
    assert sum(st.finite) == 3 * len(IX)
    h0, h1 = st.histogram(np.linspace(st.range[0], st.range[1] + 1.0, 6))
    assert int(h0.sum()) + int(h1.sum()) == 3 * len(IX)
    st.close()


# ---- the entries the package reaches through _lib.lib() with one shot per call: the same calls at B = 3, 1 and 0 --------------------------------------
def _rc(L, rc):
    L.check(rc)


def test_noise_entries_sizes_against_the_recorded_draws(L, golden):
    """qldpc_noisy_circuit_batch, qldpc_frame_sim_batch, qldpc_sparsify_batch: draws of tests/golden/circ72_noise.npz in one call (the reference's per-draw
    results are in the fixture); a capacity that is too small must leave the caller's circuits alone; an empty circuit with cap = 0"""
    g = golden("circ72_noise")
    lib, p32, p64, p8, pd = L.lib(), (lambda a: L.ptr(a, C.c_int32)), (lambda a: L.ptr(a, C.c_int64)), (lambda a: L.ptr(a, C.c_int8)), (lambda a: L.ptr(a, C.c_double))
    ops, q1, q2 = (np.ascontiguousarray(g[k]) for k in ("base_ops", "base_q1", "base_q2"))
    cap, tq, nloc, p = int(g["max_circuit_size"]), int(g["total_qubits"]), int(g["num_error_locs"]), float(g["error_rates"][0])
    assert (g["error_rates"][:3] == p).all()

    def noisy(B, cap):
        rv, rp, rt = (np.ascontiguousarray(g[k][:B]) for k in ("random_vals", "random_paulis", "random_two_qubit"))
        oo, o1, o2 = (np.full((B, cap), -5, np.int32) for _ in range(3))
        n = np.full(B, -1, np.int64)
        rc = lib.qldpc_noisy_circuit_batch(C.c_int64(B), C.c_int64(ops.size), p32(ops), p32(q1), p32(q2), C.c_double(p), C.c_int64(nloc), pd(rv), p32(rp),
                                           p32(rt), C.c_int64(cap), p32(oo), p32(o1), p32(o2), p64(n))
        return rc, oo, o1, o2, n
    for B in SIZES + (0,):
        rc, oo, o1, o2, n = noisy(B, cap)
        _rc(L, rc)
        assert np.array_equal(n, g["noisy_len"][:B])
        for b in range(B):
            for got, key in ((oo, "noisy_ops"), (o1, "noisy_q1"), (o2, "noisy_q2")):
                assert np.array_equal(got[b, :n[b]], g[key][b, :n[b]]) and not got[b, n[b]:].any(), (B, b, key)
    rc, oo, o1, o2, n = noisy(3, 16)                                            # every draw needs ~3 480 slots
    assert rc != 0 and "capacity 16" in lib.qldpc_last_error().decode() and (oo == -5).all() and (o1 == -5).all() and (o2 == -5).all()
    n = np.full(3, -1, np.int64)
    _rc(L, lib.qldpc_noisy_circuit_batch(C.c_int64(3), C.c_int64(0), None, None, None, C.c_double(p), C.c_int64(0), None, None, None, C.c_int64(0), None,
                                         None, None, p64(n)))
    assert not n.any()
    # a byte count beyond size_t (2^62 doubles per draw) is refused before anything is allocated or copied; it used to wrap
    one, onei = np.zeros(1), np.zeros(1, np.int32)
    rc = lib.qldpc_noisy_circuit_batch(C.c_int64(1), C.c_int64(0), None, None, None, C.c_double(p), C.c_int64(1 << 62), pd(one), p32(onei), p32(onei),
                                       C.c_int64(0), None, None, None, p64(n))
    assert rc == ERR_INVALID and "does not fit size_t" in lib.qldpc_last_error().decode()

    ln = g["noisy_len"][:3] + g["suffix_ops"].size
    width = int(ln.max())
    circ = [np.zeros((3, width), np.int32) for _ in range(3)]
    for b in range(3):
        for a, key, suf in zip(circ, ("noisy_ops", "noisy_q1", "noisy_q2"), ("suffix_ops", "suffix_q1", "suffix_q2")):
            a[b, :ln[b]] = np.concatenate([g[key][b, :g["noisy_len"][b]], g[suf]])
    for is_x, hk, sk, col, ms in ((0, "hist_z", "state_z", 0, int(g["max_syndromes_x"])), (1, "hist_x", "state_x", 2, int(g["max_syndromes_z"]))):
        for B in SIZES + (0,):
            hist, state, counts = np.full((B, ms), 9, np.int8), np.full((B, tq), 9, np.int8), np.full((B, 2), -1, np.int64)
            lens = np.ascontiguousarray(ln[:B], np.int64)
            _rc(L, lib.qldpc_frame_sim_batch(is_x, C.c_int64(B), C.c_int64(width), p64(lens), p32(circ[0]), p32(circ[1]), p32(circ[2]), tq, ms, p8(hist),
                                             p8(state), p64(counts)))
            assert np.array_equal(hist, g[hk][:B]) and np.array_equal(state, g[sk][:B]) and np.array_equal(counts, g["counts"][:B, col:col + 2]), (is_x, B)

    stride = g["hist_z"].shape[1]
    pos, ptrs, nchk = np.ascontiguousarray(g["x_syn_positions"]), np.ascontiguousarray(g["x_syn_ptrs"]), int(g["num_x_checks"])
    for B in SIZES + (0,):
        hist, sc = np.ascontiguousarray(g["hist_z"][:B]), np.ascontiguousarray(g["counts"][:B, 0])
        out = np.full((B, stride), 9, np.int8)
        _rc(L, lib.qldpc_sparsify_batch(C.c_int64(B), C.c_int64(stride), p8(hist), p64(sc), p32(pos), p32(ptrs), nchk, p8(out)))
        for b in range(B):
            assert np.array_equal(out[b, :sc[b]], g["sparse_z"][b]) and np.array_equal(out[b, sc[b]:], hist[b, sc[b]:])      # the rest: the copy of the history
        out = np.full((B, stride), 9, np.int8)
        _rc(L, lib.qldpc_sparsify_batch(C.c_int64(B), C.c_int64(stride), p8(hist), p64(sc), None, None, 0, p8(out)))             # no checks: the copy alone
        assert np.array_equal(out, hist)


def test_gf2_elimination_sizes_against_the_oracle(L, oracle):
    """qldpc_gf2_eliminate and _packed on B matrices at once: reduced matrix, right-hand side and pivots of every shot are the oracle's; pivot slots beyond
    the rank are zero; a matrix without rows or columns has no pivots"""
    lib, rng = L.lib(), np.random.default_rng(20261020)
    m, n = 5, 70
    nw = ((n + 7) // 8 + 7) // 8
    A = (rng.random((3, m, n)) < 0.3).astype(np.uint8)
    A[1, 3] = A[1, 0] ^ A[1, 2]                                                # shot 1 has rank 4
    rhs = (rng.random((3, m)) < 0.5).astype(np.uint8)
    ref = [oracle.gf2_elimination(A[b], rhs[b]) for b in range(3)]
    refp = [oracle.gf2_elimination_packed(A[b], rhs[b]) for b in range(3)]
    assert len(ref[1][2]) == 4 and nw == 2
    for B in SIZES + (0,):
        for packed in (False, True):
            Ain = np.ascontiguousarray(np.array([oracle.pack_rows_u64(A[b]) for b in range(B)], np.uint64).reshape(B, m, nw) if packed else A[:B].copy())
            bin_ = rhs[:B].copy()
            pr, pc, k = np.full((B, m), -1, np.int64), np.full((B, m), -1, np.int64), np.full(B, -1, np.int32)
            if packed:
                _rc(L, lib.qldpc_gf2_eliminate_packed(C.c_int64(B), m, n, nw, L.ptr(Ain, C.c_uint64), L.ptr(bin_, C.c_uint8), L.ptr(pr, C.c_int64),
                                                      L.ptr(pc, C.c_int64), L.ptr(k, C.c_int32)))
            else:
                _rc(L, lib.qldpc_gf2_eliminate(C.c_int64(B), m, n, L.ptr(Ain, C.c_uint8), L.ptr(bin_, C.c_uint8), L.ptr(pr, C.c_int64), L.ptr(pc, C.c_int64),
                                               L.ptr(k, C.c_int32)))
            for b in range(B):
                Ar, br, rr, rc_ = (refp if packed else ref)[b]
                assert np.array_equal(Ain[b], Ar) and np.array_equal(bin_[b], br) and k[b] == len(rr), (B, packed, b)
                assert np.array_equal(pr[b, :k[b]], rr) and np.array_equal(pc[b, :k[b]], rc_) and not pr[b, k[b]:].any() and not pc[b, k[b]:].any()
    k = np.full(3, -1, np.int32)
    _rc(L, lib.qldpc_gf2_eliminate(C.c_int64(3), 0, n, None, None, None, None, L.ptr(k, C.c_int32)))
    assert not k.any()


def test_check_passes_and_bp_decode_sizes(L, oracle, shots):
    """qldpc_minsum_check_pass against the oracle per shot; qldpc_bp_check_pass and qldpc_bp_decode_batch at B = 3 against their own one-shot calls (what the
    package makes); all three on a matrix without rows; B = 0"""
    lib, rng, synd = L.lib(), np.random.default_rng(20261021), shots[0]
    pd = lambda a: L.ptr(a, C.c_double)          # noqa: E731

    def check_pass(fn, g, Q, ss, param):
        B = Q.shape[0]
        R, Rs = np.full((B, g.nnz), 7.0), np.full((B, g.n), 7.0)
        _rc(L, fn(g.handle, C.c_int64(B), pd(Q), pd(ss), C.c_double(param), pd(R), pd(Rs)))
        return R, Rs

    def bp(g, s, prior):
        B = s.shape[0]
        err, llr, conv, it = np.full((B, g.n), 9, np.int8), np.full((B, g.n), 7.0), np.full(B, 9, np.uint8), np.full(B, -1, np.int32)
        _rc(L, lib.qldpc_bp_decode_batch(g.handle, C.c_int64(B), L.ptr(s, C.c_int8), pd(prior), 10, L.ptr(err, C.c_int8), pd(llr), L.ptr(conv, C.c_uint8),
                                         L.ptr(it, C.c_int32)))
        return err, llr, conv, it
    g, g0 = fresh(L), empty(L)
    Q = np.ascontiguousarray(rng.normal(0.0, 3.0, (3, len(IX))))
    ss = np.ascontiguousarray(np.where(rng.random((3, M)) < 0.5, -1.0, 1.0))
    for B in SIZES + (0,):
        R, Rs = check_pass(lib.qldpc_minsum_check_pass, g, Q[:B].copy(), ss[:B].copy(), 0.75)
        for b in range(B):
            same((R[b], Rs[b]), oracle.minsum_core_sparse(IP, IX, N, Q[b], ss[b], 0.75), f"min-sum check pass B={B} shot {b}")
        Rb, Rsb = check_pass(lib.qldpc_bp_check_pass, g, Q[:B].copy(), ss[:B].copy(), 0.9999999)
        for b in range(B):
            same((Rb[b:b + 1], Rsb[b:b + 1]), check_pass(lib.qldpc_bp_check_pass, g, Q[b:b + 1].copy(), ss[b:b + 1].copy(), 0.9999999), f"BP check pass shot {b}")
        got = bp(g, np.ascontiguousarray(synd[:B]), PRIOR)
        for b in range(B):
            same([a[b:b + 1] for a in got], bp(g, np.ascontiguousarray(synd[b:b + 1]), PRIOR), f"BP decode B={B} shot {b}")
        # no rows: no message, the column sums are zero, every shot converges on the sign of its prior
        for fn in (lib.qldpc_minsum_check_pass, lib.qldpc_bp_check_pass):
            R, Rs = check_pass(fn, g0, np.zeros((B, 0)), np.zeros((B, 0)), 0.75)
            assert R.shape == (B, 0) and not Rs.any()
        err, llr, conv, it = bp(g0, np.zeros((B, 0), np.int8), np.array([1.0, -2.0, 0.5, 3.0]))
        assert np.array_equal(err, np.tile(np.array([0, 1, 0, 0], np.int8), (B, 1))) and np.array_equal(llr, np.tile([1.0, -2.0, 0.5, 3.0], (B, 1))) and conv.all()
    assert bp(g, np.ascontiguousarray(synd[:3]), PRIOR)[2].any()                # single errors on the Hamming code converge


def test_decimation_without_the_optional_outputs(L, shots):
    """qldpc_decim_decode_batch with llr, rounds and fixed NULL: the other three outputs are those of the full call"""
    synd, g = np.ascontiguousarray(shots[0][:3]), fresh(L)
    full = decim(L, g, synd)
    err, conv, it = np.full((3, N), 9, np.int8), np.full(3, 9, np.uint8), np.full(3, -1, np.int32)
    _rc(L, L.lib().qldpc_decim_decode_batch(g.handle, C.c_int64(3), L.ptr(synd, C.c_int8), L.ptr(PRIOR, C.c_double), DECIM["alpha"], DECIM["clip_llr"],
                                            DECIM["t_round"], DECIM["max_rounds"], DECIM["per_round"], DECIM["fix_llr"], L.ptr(err, C.c_int8), None,
                                            L.ptr(conv, C.c_uint8), L.ptr(it, C.c_int32), None, None))
    same((err, conv, it), (full[0], full[2], full[3]), "decimation without llr / rounds / fixed")
    same(decim(L, g, synd), full, "and the full call after it")
