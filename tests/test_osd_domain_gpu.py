"""OSD-0 (qldpc_osd0_batch, qldpc_osd0_batch_dev) over every kernel form its dispatch reaches and both sides of every boundary between them, on the
families and shot classes of tests/osd_shapes.py.  Every solution is compared bit for bit with the oracle's, and after every call
qldpc_osd0_last_path must report the kernel the family is labelled with: a test aimed at a boundary shows that it ran there.
tests/test_osd_domain_cpu.py checks the cases themselves without a GPU."""
import os
import threading

import numpy as np
import pytest

try:            # two HIP runtimes in this image: torch first (see test_gpu_parity.py)
    import torch  # noqa: F401
except ImportError:
    torch = None

import osd_shapes as OS

pytestmark = pytest.mark.gpu
_GRAPHS = {}


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        import __graft_entry__
        __graft_entry__.build()
    _lib.require_device()
    return _lib


def graph_of(L, name):
    if name not in _GRAPHS:
        f = OS.family(name)
        _GRAPHS[name] = L.Graph(f.indptr, f.indices, f.n)
    return _GRAPHS[name]


def reported(L, r):
    """what qldpc_osd0_last_path must answer where the mirror says r"""
    return getattr(L, "OSD_PATH_" + r.path), r.mode | (L.OSD_DETAIL_REDO if r.redo else 0)


def run_family(L, oracle, name, flags=0, what=""):
    """both batches of the family through qldpc_osd0_batch: the reported path is the mirror's for these flags, every solution is the oracle's"""
    f, g = OS.family(name), graph_of(L, name)
    r = OS.rule_path(f.m, f.n, f.max_col_deg, flags)
    for (cls, synd, llr, hard, ordering), want in zip(OS.batches(name), OS.solutions(oracle, name)):
        sol = L.osd0_batch(g, synd, llr, hard, ordering=ordering, flags=flags)
        assert L.osd0_last_path(g) == reported(L, r), (name, hex(flags), what, r)
        bad = np.flatnonzero((sol != want).any(axis=1))
        assert np.array_equal(sol, want), (name, hex(flags), what, [(int(b), cls[b]) for b in bad])
    return r


@pytest.mark.parametrize("name", [n for n in OS.TABLE if n != "refused"])
def test_family_default_flags(L, oracle, name):
    """every family x every class; the kernel is the one the family's label names, in the form (W16, threads) the mirror derives from m"""
    f = OS.family(name)
    r = run_family(L, oracle, name)
    assert (r.path, r.w16) == (f.path, f.w16), name
    print(f"osd-domain {name}: {f.m} x {f.n}, max column degree {f.max_col_deg}, rank {f.rank} -> {r.path}{' W16' if r.w16 else ''}, {r.block} threads, "
          f"reference-order form {r.mode}{', redo queued' if r.redo else ''}")


@pytest.mark.parametrize("name", OS.FLAG_FAMILIES)
def test_family_under_flags(L, oracle, name):
    """the boundary families under the size-class flags, each where the mirror says it changes the kernel, the reference-order form or the redo"""
    f = OS.family(name)
    base = OS.rule_path(f.m, f.n, f.max_col_deg)
    for flags in OS.honoured(f):
        r = run_family(L, oracle, name, flags)
        assert (r.path, r.mode, r.redo) != (base.path, base.mode, base.redo)
        print(f"osd-domain {name} flags {flags:#x} -> {r.path}, reference-order form {r.mode}{', redo queued' if r.redo else ''}")


@pytest.mark.parametrize("name", OS.PRESORT_FAMILIES)
def test_presort_heads(L, oracle, name):
    """a sorted head of 16 columns (the rest path on nearly every shot) and the whole order up front, at the W16 / osd_gjg edges"""
    try:
        for presort in (16, 0):
            L.set_option("osd_presort", presort)
            run_family(L, oracle, name, what=f"presort {presort}")
    finally:
        L.set_option("osd_presort", -1)


def big_batch(oracle, cls):
    f = OS.family("s129x1024")
    s = OS.class_shots(f, cls, B=OS.BIG_BATCH)
    return f, s, OS.oracle_osd0(oracle, f, s.synd, s.llr, s.hard)


def test_batch_larger_than_the_grid(L, oracle):
    """600 shots on 512 workgroups: the work queue hands a second shot to some of them"""
    f, s, want = big_batch(oracle, "sparse error")
    g = graph_of(L, "s129x1024")
    sol = L.osd0_batch(g, s.synd, s.llr, s.hard)
    assert L.osd0_last_path(g) == (L.OSD_PATH_GJ, 1 | L.OSD_DETAIL_REDO)
    assert np.array_equal(sol, want), np.flatnonzero((sol != want).any(axis=1))


def test_redo_list_holds_every_shot(L, oracle):
    """600 syndromes outside the column space: the free-pivot kernel lists every one of them, the reference-order kernel behind it answers them all"""
    f, s, want = big_batch(oracle, "random syndrome")
    assert OS.outside(f, s.synd).all()
    g = graph_of(L, "s129x1024")
    sol = L.osd0_batch(g, s.synd, s.llr, s.hard)
    path, detail = L.osd0_last_path(g)
    assert path == L.OSD_PATH_GJ and detail & L.OSD_DETAIL_REDO and detail & L.OSD_DETAIL_MODE_MASK == 1
    assert np.array_equal(sol, want), np.flatnonzero((sol != want).any(axis=1))


def test_device_entry_on_a_side_stream_with_a_select_list(L, oracle):
    """qldpc_osd0_batch_dev at m = 1024 on a stream of its own, every third shot listed: the listed rows are the oracle's, the others keep their sentinel"""
    import ctypes as C
    name = "m1024"
    f, g = OS.family(name), graph_of(L, name)
    cls, synd, llr, hard, _ = OS.batches(name)[0]
    want = OS.solutions(oracle, name)[0]
    B = synd.shape[0]
    listed = np.arange(0, B, 3)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ds, dl, dh = torch.from_numpy(synd).cuda(), torch.from_numpy(llr).cuda(), torch.from_numpy(hard).cuda()
        sel = torch.from_numpy(listed.astype(np.int32)).cuda()
        cnt = torch.tensor([listed.size], dtype=torch.int32, device="cuda")
        dsol = torch.full((B, f.n), 7, dtype=torch.int8, device="cuda")
        st.synchronize()
        p = lambda t: C.c_void_p(t.data_ptr())       # noqa: E731
        L.check(L.lib().qldpc_osd0_batch_dev(g.handle, C.c_int64(B), p(ds), p(dl), p(dh), None, p(sel), p(cnt), 0, p(dsol), C.c_void_p(st.cuda_stream)))
        st.synchronize()
    assert L.osd0_last_path(g) == (L.OSD_PATH_GJ, 1 | L.OSD_DETAIL_REDO)
    sol = dsol.cpu().numpy()
    rest = np.setdiff1d(np.arange(B), listed)
    assert (sol[rest] == 7).all()
    assert np.array_equal(sol[listed], want[listed]), [(int(b), cls[b]) for b in listed[(sol[listed] != want[listed]).any(axis=1)]]


def test_two_host_threads_on_one_handle(L, oracle):
    """two threads in qldpc_osd0_batch on the same graph handle at m = 1025 (the workspaces are shared and handed over): both get the oracle's answers"""
    name = "m1025"
    g = graph_of(L, name)
    batches, want = OS.batches(name), OS.solutions(oracle, name)
    out, errs = {}, []

    def work(k):
        try:
            _, synd, llr, hard, ordering = batches[k]
            out[k] = [L.osd0_batch(g, synd, llr, hard, ordering=ordering) for _ in range(2)]
        except Exception as e:       # noqa: BLE001
            errs.append(e)
    threads = [threading.Thread(target=work, args=(k,)) for k in (0, 1)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    for k in (0, 1):
        for sol in out[k]:
            assert np.array_equal(sol, want[k]), (k, np.flatnonzero((sol != want[k]).any(axis=1)))
    assert L.osd0_last_path(g)[0] == L.OSD_PATH_GJG


@pytest.mark.parametrize("name", ["m1022", "m1023", "m1024", "ident1024"])
def test_queue_form_of_the_experiments_build_at_the_last_rows(oracle, name):
    """the look-ahead-queue form of the W16 kernel (csrc/osd_gjq.hip, experiments build only) shared the defect the m = 1023 family found in
    osd_gj.hip: the right-hand side row m + 1 >= 1024 had no lane in the overlapped row updates.  Same families, same oracle."""
    from conftest import experiments_lib
    X = experiments_lib()
    if not os.path.exists(X.SO_PATH):
        import __graft_entry__
        __graft_entry__.build()
    X.require_device()
    f = OS.family(name)
    g = X.Graph(f.indptr, f.indices, f.n)
    for (cls, synd, llr, hard, ordering), want in zip(OS.batches(name), OS.solutions(oracle, name)):
        sol = X.osd0_batch(g, synd, llr, hard, ordering=ordering, flags=X.FLAG_OSD_QUEUE)
        assert X.osd0_last_path(g)[0] == X.OSD_PATH_GJ
        bad = np.flatnonzero((sol != want).any(axis=1))
        assert np.array_equal(sol, want), (name, [(int(b), cls[b]) for b in bad])


def test_refused_matrix(L):
    """m = 30720: the global kernel's elimination scratch does not fit; QLDPC_ERR_UNSUPPORTED with its message, and no kernel is reported"""
    f = OS.family("refused")
    g = L.Graph(f.indptr, f.indices, f.n)
    s = OS.class_shots(f, "sparse error", B=2)
    with pytest.raises(L.QldpcError) as e:
        L.osd0_batch(g, s.synd, s.llr, s.hard)
    assert "error -4" in str(e.value) and OS.UNSUPPORTED_TEXT in str(e.value), str(e.value)
    assert L.osd0_last_path(g) == (L.OSD_PATH_NONE, 0)
