"""BP+LSD on the MI355X over the families of tests/lsd_domain_shapes.py (tests/test_lsd_domain_cpu.py asserts on the model that they reach the edges they
are named for): qldpc_lsd_batch equals tests/lsd_model.py bit for bit in solution and info (flag 1 / 2 shots: qldpc_osd0_batch's answer),
qldpc_lsd_stats_batch equals tests/lsd_stats_model.py in all eight words without weights, with a seeded table and with every weight 65535, the device
entry points with a select list, the refusals on the far side of every computed edge (return code, error text, outputs untouched), and a circuit plan
beyond bb72 (hgp) with LSD and a confidence against the pieces put together by hand."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lsd_domain_shapes as D  # noqa: E402
import lsd_shapes as LS  # noqa: E402
import lsd_stats_model as SM  # noqa: E402
import osd_shapes as S  # noqa: E402

pytestmark = pytest.mark.gpu

NONE = SM.NONE
_GRAPHS = {}


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


def _graph(L, name):
    if name not in _GRAPHS:
        f = D.family(name)
        _GRAPHS[name] = L.Graph(f.indptr, f.indices, f.n)
    return _GRAPHS[name]


def _held(L, name, bps, cap):
    """library == model on every shot of the family at (bps, cap): solution, info and the eight words under the three weight tables"""
    g, sh = _graph(L, name), D.shots(name)
    want_sol, want_info, _ = D.answers(name, bps, cap)
    sol, info = L.lsd_batch(g, sh.synd, sh.llr, sh.hard, bps, cap)
    what = f"{name} bits {bps} cap {cap}"
    flagged = np.flatnonzero(want_info[:, 0] != 0)
    want = want_sol.copy()
    if flagged.size:
        want[flagged] = L.osd0_batch(g, sh.synd[flagged], sh.llr[flagged], sh.hard[flagged])
    for b in range(sh.synd.shape[0]):
        assert tuple(info[b]) == tuple(want_info[b]), f"{what} shot {b}: info {info[b]} vs model {want_info[b]}"
        assert np.array_equal(sol[b], want[b]), f"{what} shot {b} (flag {info[b, 0]}): solution differs in {np.flatnonzero(sol[b] != want[b])[:8]}"
    for weight in (None, "seeded", "ones"):
        w, want_stats = D.stats(name, bps, cap, weight)
        sol1, info1, stats = L.lsd_stats_batch(g, sh.synd, sh.llr, sh.hard, bps, cap, w)
        assert np.array_equal(sol1, sol) and np.array_equal(info1, info), f"{what} weights {weight}: solution or info differ from the plain call"
        for b in range(sh.synd.shape[0]):
            assert stats[b].tolist() == want_stats[b].tolist(), f"{what} weights {weight} shot {b} (flag {info[b, 0]}): {stats[b].tolist()} vs model {want_stats[b].tolist()}"
    return info


@pytest.mark.parametrize("name", D.NAMES)
def test_family(L, name):
    """every (bits_per_step, max_rows) of the family; the edge it is there for is written beside it in lsd_domain_shapes"""
    for bps, cap in D.params(name):
        _held(L, name, bps, cap)


def test_dev_entries_with_a_select_list(L):
    """device pointers and a select list on a family whose clusters pass 256 rows: the listed shots are the host call's, the others untouched"""
    name, bps, cap = "s129d2", 1, 257                                        # (shots 0 .. 2 end capped, shot 3 on 256 rows)
    g, sh = _graph(L, name), D.shots(name)
    w = D.weights(g.n)
    whole = L.lsd_stats_batch(g, sh.synd, sh.llr, sh.hard, bps, cap, w)
    assert set(whole[1][:, 0]) == {0, 1}
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)        # noqa: E731
    p = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None      # noqa: E731
    ds, dl, dh, dw = t(sh.synd), t(sh.llr), t(sh.hard), t(w.view(np.int16))
    B = sh.synd.shape[0]
    sel = np.array([3, 0], np.int32)
    dsel, dcnt = t(sel), t(np.array([sel.size], np.int32))
    for with_stats in (False, True):
        dinfo = torch.full((B, 4), -7, dtype=torch.int32, device=dev)
        dstats = torch.full((B, 8), 12345, dtype=torch.int64, device=dev)
        dsol = torch.full((B, g.n), 3, dtype=torch.int8, device=dev)
        if with_stats:
            rc = L.lib().qldpc_lsd_stats_batch_dev(g.handle, B, p(ds), p(dl), p(dh), bps, cap, p(dsel), p(dcnt), p(dw), p(dsol), p(dinfo), p(dstats), C.c_void_p(0))
        else:
            rc = L.lib().qldpc_lsd_batch_dev(g.handle, B, p(ds), p(dl), p(dh), bps, cap, p(dsel), p(dcnt), p(dsol), p(dinfo), C.c_void_p(0))
        assert rc == 0
        torch.cuda.synchronize()
        sol, info, stats = dsol.cpu().numpy(), dinfo.cpu().numpy(), dstats.cpu().numpy().view(np.uint64)
        for i in range(B):
            if i in sel:
                assert np.array_equal(sol[i], whole[0][i]) and np.array_equal(info[i], whole[1][i]), i
                assert np.array_equal(stats[i], whole[2][i]) if with_stats else (stats[i] == 12345).all(), i
            else:
                assert (sol[i] == 3).all() and (info[i] == -7).all() and (stats[i] == 12345).all(), i


def _refused(L, f, cap, text, stats=False):
    """the call returns QLDPC_ERR_UNSUPPORTED with `text` and writes no output byte (two shots; one has a seed, so a launch would have had work)"""
    g = L.Graph(f.indptr, f.indices, f.n)
    synd, llr, hard = np.zeros((2, f.m), np.int8), np.ones((2, f.n)), np.zeros((2, f.n), np.int8)
    synd[1, 0] = 1
    sol, info, st = np.full((2, f.n), 5, np.int8), np.full((2, 4), -9, np.int32), np.full((2, 8), 77, np.uint64)
    a = (g.handle, 2, L.ptr(synd, C.c_int8), L.ptr(llr, C.c_double), L.ptr(hard, C.c_int8), 1, int(cap))
    if stats:
        rc = L.lib().qldpc_lsd_stats_batch(*a, None, L.ptr(sol, C.c_int8), L.ptr(info, C.c_int32), L.ptr(st, C.c_uint64))
    else:
        rc = L.lib().qldpc_lsd_batch(*a, L.ptr(sol, C.c_int8), L.ptr(info, C.c_int32))
    err = L.lib().qldpc_last_error().decode()
    assert rc == -4 and text in err, (f.m, f.n, cap, rc, err)
    assert (sol == 5).all() and (info == -9).all() and (st == 77).all()
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)        # noqa: E731
    p = lambda x: C.c_void_p(x.data_ptr())                                  # noqa: E731
    ds, dl, dh, dsol, dinfo = t(synd), t(llr), t(hard), t(sol), t(info)
    assert L.lib().qldpc_lsd_batch_dev(g.handle, 2, p(ds), p(dl), p(dh), 1, int(cap), None, None, p(dsol), p(dinfo), C.c_void_p(0)) == -4
    assert text in L.lib().qldpc_last_error().decode()
    dst = t(st.view(np.int64))
    assert L.lib().qldpc_lsd_stats_batch_dev(g.handle, 2, p(ds), p(dl), p(dh), 1, int(cap), None, None, None, p(dsol), p(dinfo), p(dst), C.c_void_p(0)) == -4
    assert text in L.lib().qldpc_last_error().decode()
    torch.cuda.synchronize()
    assert (dsol.cpu().numpy() == 5).all() and (dinfo.cpu().numpy() == -9).all() and (dst.cpu().numpy() == 77).all()
    g.close()
    return err


def test_refusals_beyond_the_layout_edges(L):
    """one column more than the widest matrix at max_rows = 1024, and one row more of cap than the 65534-column matrix takes: the LDS text"""
    E = D.edges()
    f = S.build_matrix("lsd_domain_dep_over", "dep", D.M_DEP, E.n_wide + 1)
    assert f.max_col_deg == E.cd_wide and not D.accepted(f.m, f.n, f.max_col_deg, D.CAP) and D.accepted(f.m, f.n, f.max_col_deg, 960)
    _refused(L, f, D.CAP, D.LDS_TEXT)
    _refused(L, f, D.CAP, D.LDS_TEXT, stats=True)
    u = D.family("u200")
    assert not D.accepted(u.m, u.n, u.max_col_deg, E.cap_u200 + 1)
    _refused(L, u, E.cap_u200 + 1, D.LDS_TEXT)


def test_refusals_beyond_the_hand_over_edge(L):
    """a matrix OSD-0 refuses is refused before anything is launched, whether or not a shot would have been handed over; m = 65536 as before"""
    E = D.edges()
    for m, cap in ((E.m_tall + 1, 512), (65535, E.cap_65535), (65535, 1)):
        f = S.build_matrix("lsd_domain_tall_over", "plain", m, 64)
        assert f.max_col_deg == E.cd_tall and LS.supported(f.m, f.n, f.max_col_deg, cap) and not D.accepted(f.m, f.n, f.max_col_deg, cap)
        err = _refused(L, f, cap, D.HANDOVER_TEXT)
        assert f"{m} x 64" in err
    _refused(L, S.build_matrix("lsd_domain_tall_over", "plain", E.m_tall + 1, 64), 512, D.HANDOVER_TEXT, stats=True)
    _refused(L, S.build_matrix("lsd_domain_tall_over", "plain", 65535, 64), E.cap_65535 + 1, D.LDS_TEXT)      # (the layout is asked first)
    _refused(L, S.build_matrix("lsd_domain_tall_over", "plain", 65536, 64), 1, D.ROWS_TEXT)


# ---------------------------------------------------------------------------------------------------------------- a circuit plan beyond bb72
PLAN = "hgp"
EDGES = np.array([1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96, 128, 256, 512, 1024, 1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20, 1 << 24, 1 << 28, 1 << 32], np.uint64)


def test_circuit_plan_beyond_bb72_matches_the_pieces(L):
    """hgp (sectors of 280 and 315 detectors, decoding matrices of unequal width), 1024 trials, LSD with a confidence: verdicts, LSD counts, scores and
    histogram equal sampler -> min-sum -> qldpc_lsd_stats_batch -> numpy judge put together by hand; both sectors hand shots over"""
    import test_circuit_shapes_cpu as TC
    from test_circuit_shapes_gpu import setup
    Sh, sigs, Mx, graphs, priors, masks, plan = setup(L, PLAN)
    count, seed, bps, max_rows, p_err = 1024, 4321, 2, 128, TC.P_HIGH[PLAN]
    q = plan(p_err, batch=count)
    spz, tz, spx, tx = q.sample(seed, 0, count)
    q.close()
    verdict = np.zeros(count, np.uint8)
    stats, osd, flags = [], [], []
    for sec, (g, prior, mask, synd, true) in enumerate(((graphs[0], priors[0], masks[0], spz, tz), (graphs[1], priors[1], masks[1], spx, tx))):
        det, conv, llr, iters = L.minsum_decode_batch(g, synd, prior, 50, "dynamical", 1.0)
        bad = np.flatnonzero(conv == 0)
        st = np.zeros((count, 8), np.uint64)
        det[bad], info, st[bad] = L.lsd_stats_batch(g, synd[bad], llr[bad], det[bad], bps, max_rows, L.quantise_weights(prior))
        rows = np.stack([(mask >> np.uint64(r)) & np.uint64(1) for r in range(true.shape[1])]).astype(np.int64)
        dec = (det.astype(np.int64) @ rows.T) % 2
        verdict |= (np.any(dec != true.astype(np.int64), axis=1).astype(np.uint8) << sec)
        stats.append(st)
        osd.append(int(bad.size))
        flags.append(np.bincount(info[:, 0], minlength=3))
    flags = np.stack(flags)
    print(PLAN, "p", p_err, "handed over Z / X:", osd, "flags:", flags.tolist(), "errors:", int(np.count_nonzero(verdict)))
    assert min(osd) > 0                                                      # both sectors handed shots over
    wz, wx = (L.quantise_weights(p) for p in priors)
    T = L.TALLY
    for batch in (1024, 300):
        q = plan(p_err, batch=batch)
        q.use_lsd(bps, max_rows)
        for kind in ("cols_1", "llr_2", "llr_inf"):
            q.use_confidence(kind, EDGES, wz, wx)
            q.read(clear=True)
            q.lsd_counts(clear=True)
            out, score = q.run_scores(seed, 0, count)
            want = SM.scores(kind, stats[0], stats[1])
            assert np.array_equal(out, verdict) and np.array_equal(score, want), (kind, batch)
            assert np.array_equal(q.confidence_hist(), SM.histogram(want, verdict, EDGES)), (kind, batch)
            tally, counts = q.read(), q.lsd_counts()
            assert np.array_equal(counts, flags) and counts.sum(axis=1).tolist() == osd == [tally[T["osd_z"]], tally[T["osd_x"]]]
            assert tally[T["trials"]] == count and tally[T["total_err"]] == np.count_nonzero(verdict)
        q.close()
