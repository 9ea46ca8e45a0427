"""qldpc_gf2_eliminate and qldpc_gf2_eliminate_packed on the cases of tests/elim_shapes.py against the oracle: the reduced matrix, the right-hand side, the
pivots, the pivot count and the zeroed tail of the pivot arrays, bit for bit -- at the block-size switch, on both sides of 64 KiB and of the 150 KiB line of
the LDS scratch, and on the small edges.  tests/test_elim_domain_cpu.py checks the cases themselves without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

try:            # two HIP runtimes in this image: torch first (see test_gpu_parity.py)
    import torch  # noqa: F401
except ImportError:
    torch = None

import elim_shapes as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    if not os.path.exists(_lib.SO_PATH):
        import __graft_entry__
        __graft_entry__.build()
    _lib.require_device()
    return _lib


def eliminate(L, A, b, n, packed):
    """-> (rc, A, b, pivot_rows, pivot_cols, num_pivots) of one call; A [B, m, n] bytes or [B, m, nwords] words"""
    A, b = np.ascontiguousarray(A).copy(), np.ascontiguousarray(b).copy()
    B, m = b.shape
    maxp = max(min(m, n), 1)
    pr, pc, k = np.full((B, maxp), -1, np.int64), np.full((B, maxp), -1, np.int64), np.full(B, -1, np.int32)
    if packed:
        rc = L.lib().qldpc_gf2_eliminate_packed(C.c_int64(B), m, n, A.shape[2], L.ptr(A, C.c_uint64), L.ptr(b, C.c_uint8), L.ptr(pr, C.c_int64),
                                                L.ptr(pc, C.c_int64), L.ptr(k, C.c_int32))
    else:
        rc = L.lib().qldpc_gf2_eliminate(C.c_int64(B), m, n, L.ptr(A, C.c_uint8), L.ptr(b, C.c_uint8), L.ptr(pr, C.c_int64), L.ptr(pc, C.c_int64),
                                         L.ptr(k, C.c_int32))
    return rc, A, b, pr, pc, k


def same(got, want, where):
    rc, A, b, pr, pc, k = got
    assert rc == 0, where
    for s, (wA, wb, wpr, wpc) in enumerate(want):
        assert k[s] == len(wpr), where + (s, "pivot count")
        assert np.array_equal(A[s], wA), where + (s, "reduced matrix")
        assert np.array_equal(b[s], wb), where + (s, "right-hand side")
        assert np.array_equal(pr[s, :k[s]], wpr) and np.array_equal(pc[s, :k[s]], wpc), where + (s, "pivots")
        assert not pr[s, k[s]:].any() and not pc[s, k[s]:].any(), where + (s, "tail of the pivot arrays")


@pytest.mark.parametrize("name", [n for n in E.TABLE if not E.case(n).refused])
def test_case(L, oracle, name):
    c = E.case(name)
    same(eliminate(L, c.A, c.b, c.n, False), [oracle.gf2_elimination(c.A[s], c.b[s]) for s in range(c.B)], (name, "bytes"))
    P = np.stack([oracle.pack_rows_u64(c.A[s]) for s in range(c.B)])
    same(eliminate(L, P, c.b, c.n, True), [oracle.gf2_elimination_packed(c.A[s], c.b[s]) for s in range(c.B)], (name, "packed"))
    print(f"elim-domain {name}: {c.B} x {c.m} x {c.n}, {E.block_of(c.m)} threads, {c.lds} bytes of LDS scratch, ranks {c.expect['rank']}")


def test_three_row_words_for_70_columns(L, oracle):
    """nwords = 3 where n = 70 needs 2, random bits beyond column 70: they never pivot and are XOR-ed like any other"""
    P, b, n = E.packed3()
    same(eliminate(L, P, b, n, True), [oracle.gf2_elimination_packed_words(P[0], b[0], n)], (E.PACKED3,))


def test_refused_above_150_kib(L):
    """m = 30711: QLDPC_ERR_UNSUPPORTED from both entry points, nothing written"""
    c = E.case("lds_30711")
    for packed in (False, True):
        A = np.zeros((1, c.m, 1), np.uint64) if packed else c.A
        rc, A2, b2, pr, pc, k = eliminate(L, A, c.b, c.n, packed)
        assert rc == E.ERR_UNSUPPORTED and E.LDS_TEXT in L.lib().qldpc_last_error().decode(), (packed, rc)
        assert np.array_equal(A2, A) and np.array_equal(b2, c.b) and (pr == -1).all() and (k == -1).all()
