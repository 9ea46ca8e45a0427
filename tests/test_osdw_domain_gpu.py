"""OSD-w (qldpc_osdw_batch: performOSD_enhanced with order > 0) on the cases of tests/osdw_shapes.py: the K edges, the capacity of the candidate slab, every
max_combinations cut-off, the reachable branches of the selection rule, second and third shots of a workgroup, and the literal elimination's LDS scratch on
both sides of 64 KiB and of the 150 KiB line.  Every solution is compared bit for bit with the oracle's and, where the model of tests/osdw_model.py ran (at
most 5000 candidates per shot; the three capacity cases are above), with the model's.  tests/test_osdw_domain_cpu.py checks the cases themselves without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

try:            # two HIP runtimes in this image: torch first (see test_gpu_parity.py)
    import torch  # noqa: F401
except ImportError:
    torch = None

import osdw_shapes as S

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


def graph_of(L, c):
    key = c.H.tobytes(), c.H.shape
    if key not in _GRAPHS:
        _GRAPHS[key] = L.Graph(c.indptr, c.indices, c.n)
    return _GRAPHS[key]


def run(L, c, rows=slice(None)):
    return L.osdw_batch(graph_of(L, c), c.synd[rows], c.llr[rows], c.hard[rows], c.order, c.maxc, None if c.ordering is None else c.ordering[rows])


@pytest.mark.parametrize("name", S.RUN)
def test_case(L, oracle, name):
    c = S.case(name)
    sol = run(L, c)
    want = S.oracle_answers(oracle, name)
    assert np.array_equal(sol, want), (name, c.note, np.flatnonzero((sol != want).any(axis=1)))
    if c.modelled:
        model = S.model_answers(name)[0]
        assert np.array_equal(sol, model), (name, c.note, np.flatnonzero((sol != model).any(axis=1)))
    print(f"osdw-domain {name}: {c.m} x {c.n}, {c.B} shots, order {c.order}, max_combinations {c.maxc}, K {c.expect['K']}, {c.expect['tested']} candidates, "
          f"elimination scratch {S.elim_lds_bytes(c.m, S.nwords_of(c.n))} bytes, {'model and oracle' if c.modelled else 'oracle'}")


@pytest.mark.parametrize("name", S.REFUSED)
def test_refused(L, name):
    """by return code and message; nothing is written"""
    c = S.case(name)
    g = graph_of(L, c)
    sol = np.full((c.B, c.n), 7, np.int8)
    rc = L.lib().qldpc_osdw_batch(g.handle, C.c_int64(c.B), L.ptr(c.synd, C.c_int8), L.ptr(c.llr, C.c_double), L.ptr(c.hard, C.c_int8), None, C.c_int(c.order),
                                  C.c_int64(c.maxc or 0), L.ptr(sol, C.c_int8))
    code, text = c.refused
    assert rc == code and text in L.lib().qldpc_last_error().decode(), (name, rc, L.lib().qldpc_last_error())
    assert (sol == 7).all()
    with pytest.raises(L.QldpcError) as e:
        run(L, c)
    assert f"error {code}" in str(e.value) and text in str(e.value)


@pytest.mark.parametrize("name", S.TRIPS)
def test_batch_of_three_trips_equals_its_one_shot_calls(L, oracle, name):
    """B = 133 on 64 workgroups: what a workgroup keeps from one shot to the next (s_w0, s_best, isp, eperm, dead[], the candidate slab) must not reach the
    next answer -- a one-shot call has no previous shot"""
    c = S.case(name)
    assert c.B == 133 and S.trips_of(c.B) == 3
    sol = run(L, c)
    single = np.concatenate([run(L, c, slice(b, b + 1)) for b in range(c.B)])
    assert np.array_equal(sol, single), (name, np.flatnonzero((sol != single).any(axis=1)))
    assert np.array_equal(sol, S.oracle_answers(oracle, name))


@pytest.mark.parametrize("name", S.WRAPPER_CASES)
def test_wrapper_of_the_package(L, oracle, name):
    """decoding/osd.py's performOSD_enhanced (host argsort; these cases have no two equal |llr| in a shot) returns the oracle's answers as int64"""
    from qldpc_amd.decoding.osd import performOSD_enhanced
    c = S.case(name)
    assert all(np.unique(np.abs(c.llr[b])).size == c.n for b in range(c.B))
    want = S.oracle_answers(oracle, name)
    for b in range(c.B):
        sol = performOSD_enhanced(c.H.astype(np.float64), c.synd[b], c.llr[b], c.hard[b], order=c.order, max_combinations=c.maxc)
        assert sol.dtype == np.int64 and np.array_equal(sol, want[b]), (name, b)


def test_delegations(L, oracle):
    """order 0 is qldpc_osd0_batch; B = 0 and n = 0 write nothing; a matrix without rows returns `hard`"""
    lib = L.lib()
    c = S.case("sel_deep")
    g = graph_of(L, c)
    sol0 = L.osdw_batch(g, c.synd, c.llr, c.hard, 0)
    assert np.array_equal(sol0, L.osd0_batch(g, c.synd, c.llr, c.hard))
    assert np.array_equal(sol0, np.stack([oracle.osd0(c.indptr, c.indices, c.n, c.synd[b], c.llr[b], c.hard[b]) for b in range(c.B)]))
    assert not np.array_equal(sol0, run(L, c))                                   # (and the sweep is not a delegation)
    assert L.osdw_batch(g, c.synd[:0], c.llr[:0], c.hard[:0], 3).shape == (0, c.n)
    assert lib.qldpc_osdw_batch(g.handle, C.c_int64(0), None, None, None, None, C.c_int(3), C.c_int64(0), None) == 0
    # no rows: the answer is `hard` (raw call: there is no syndrome to pass)
    g0 = L.Graph(np.zeros(1, np.int32), np.zeros(0, np.int32), 5)
    rng = np.random.default_rng(3)
    hard, llr = (rng.random((3, 5)) < 0.5).astype(np.int8), rng.normal(0, 1, (3, 5))
    for order in (0, 2):
        sol = np.full((3, 5), 7, np.int8)
        L.check(lib.qldpc_osdw_batch(g0.handle, C.c_int64(3), None, L.ptr(llr, C.c_double), L.ptr(hard, C.c_int8), None, C.c_int(order), C.c_int64(0),
                                     L.ptr(sol, C.c_int8)))
        assert np.array_equal(sol, hard), order
    # no columns: nothing to write
    gn = L.Graph(np.zeros(4, np.int32), np.zeros(0, np.int32), 0)
    synd = np.ones((2, 3), np.int8)
    for order in (0, 2):
        assert lib.qldpc_osdw_batch(gn.handle, C.c_int64(2), L.ptr(synd, C.c_int8), None, None, None, C.c_int(order), C.c_int64(0), None) == 0
    assert lib.qldpc_osdw_batch(g.handle, C.c_int64(1), L.ptr(c.synd, C.c_int8), L.ptr(c.llr, C.c_double), L.ptr(c.hard, C.c_int8), None, C.c_int(-1),
                                C.c_int64(0), L.ptr(sol0, C.c_int8)) == S.ERR_INVALID
