"""The layered decoder on the MI355X over its domain (tests/layered_shapes.py): on every family qldpc_layered_decoder_info equals the restated rules
field by field (the exact LDS bytes, the storage form, the workgroup size) and every output equals the numpy model bit for bit; the refusal beyond
the last accepted row count; a workgroup that takes a second shot from the queue, with the posteriors in LDS and in the slab; convergence found
after the last layer of the last iteration.  tests/test_layered_domain_cpu.py has compared the model with the serial loop on the same families."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import layered_model as LM  # noqa: E402
import layered_shapes as LSH  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("err", "conv", "llr", "iters")
CASES = LSH.all_cases()
BY_NAME = {c.name: c for c in CASES}
ACCEPTED = [c.name for c in CASES if c.claims["form"] is not None]


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


def assert_same(got, ref, what):
    """bytes; for llr equal values, NaN where NaN and the zeros of one sign (as tests/test_shot_prior_gpu.py compares)"""
    for a, b, name in zip(got, ref, NAMES):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {name} has another type or shape"
        if name == "llr":
            bad = np.flatnonzero(~(((a == b) & (np.signbit(a) == np.signbit(b))) | ((a != a) & (b != b))).reshape(len(a), -1).all(axis=1))
        else:
            bad = np.flatnonzero(~(a == b).reshape(len(a), -1).all(axis=1))
        assert bad.size == 0, f"{what}: {name} differs on shots {bad[:8].tolist()} ({bad.size} of {len(a)})"


def flags_of(L, c, extra=()):
    out = 0
    for f in tuple(c.flags) + tuple(extra):
        out |= getattr(L, "FLAG_LAYERED_" + f)
    return out


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("name", ACCEPTED)
def test_every_family_against_the_rules_and_the_model(L, name):
    c = BY_NAME[name]
    e = LSH.expected(c)
    g = L.Graph(c.indptr, c.indices, c.n)
    synd = LSH.shots(c)
    for pn, prior in c.priors.items():
        dec = L.LayeredDecoder(g, prior, max_iter=c.max_iter, layers=c.row_layer, flags=flags_of(L, c))
        info = dec.info()
        got = dec.decode(synd)
        dec.close()
        print(name, pn, info)
        for key in ("layers", "max_layer_rows", "max_layer_edges", "lds_bytes", "block", "v_global", "lds_indices"):
            assert info[key] == e[key], (name, key, info, e)
        assert_same(got, LSH.reference(c, pn), f"{name} / {pn}")


def test_the_first_refused_row_count(L):
    """one row with entries beyond rows_vg_last: QLDPC_ERR_UNSUPPORTED, the message names the LDS count, no handle; a call without a handle touches nothing"""
    c = BY_NAME["rows_refused"]
    e = LSH.expected(c)
    assert not e["accepted"] and LSH.expected(BY_NAME["rows_vg_last"])["accepted"]
    g = L.Graph(c.indptr, c.indices, c.n)
    lib = L.lib()
    prior = np.ascontiguousarray(c.priors["normal"])
    for flags in (0, L.FLAG_LAYERED_VGLOBAL | L.FLAG_LAYERED_GLOBAL_IDX):
        h = C.c_void_p(12345)
        rc = lib.qldpc_layered_decoder_create(g.handle, None, L.ptr(prior, C.c_double), 3, 1, 1.0, None, 0, 20.0, flags, C.byref(h))
        msg = lib.qldpc_last_error().decode()
        assert rc == -4 and h.value is None and "LDS" in msg and f"{e['nslots']} rows in {e['layers']} layers need {e['lds_bytes']} bytes" in msg, msg
    with pytest.raises(L.QldpcError, match="error -4"):
        L.LayeredDecoder(g, prior, max_iter=3)
    synd = LSH.shots(c)
    err, llr = np.full((LSH.B, c.n), 9, np.int8), np.full((LSH.B, c.n), 9.0)
    conv, it = np.full(LSH.B, 9, np.uint8), np.full(LSH.B, -7, np.int32)
    rc = lib.qldpc_layered_decode_batch(None, LSH.B, L.ptr(synd, C.c_int8), L.ptr(err, C.c_int8), L.ptr(llr, C.c_double), L.ptr(conv, C.c_uint8), L.ptr(it, C.c_int32))
    assert rc == -1 and (err == 9).all() and (llr == 9.0).all() and (conv == 9).all() and (it == -7).all()


@pytest.mark.parametrize("extra", [(), ("VGLOBAL",)], ids=["lds", "slab"])
def test_the_queue_hands_out_a_second_shot(L, extra):
    """Eight shots for every workgroup of the grid and eight more, B = 8 (cap + 1): each of the eight kinds of shot -- five that converge (in
    iterations 0, 0, 0, 1 and 2 by the model), three that run all nine iterations, one of these with a 1 on the row without entries -- occurs
    cap + 1 times, and a workgroup ends on one shot only, so whichever way the atomic queue deals them, every kind is followed by another shot in
    some workgroup.  That workgroup must refill V (in LDS, or its slab) and reset the records and the syndrome bytes, whatever the shot before
    left in them; after the shot with the 1 on the empty row it must also clear the empty-row flag, or a successor that converges (5 of the 8
    kinds) reports conv = 0.  Every block of eight is another order of the eight shots, so every row of the big call has a row of the B = 8 call
    to equal, and that call equals the model.  What the run cannot tell: WHICH shot follows which (the queue decides).  That the empty-row shot has
    a successor is certain; that one of its successors converges is not, only as good as certain (some 7/8 of its cap + 1 occurrences have a
    successor, each of a converging kind with probability 5/8)."""
    c = LSH.queue_graph()
    g = L.Graph(c.indptr, c.indices, c.n)
    synd = LSH.shots(c)
    assert (np.diff(c.indptr) == 0).any() and synd[5, np.diff(c.indptr) == 0].any()
    dec = L.LayeredDecoder(g, c.priors["normal"], max_iter=c.max_iter, flags=flags_of(L, c, ("BLOCK_1024",) + extra))
    info = dec.info()
    assert info["block"] == 1024 and info["v_global"] == bool(extra)
    small = dec.decode(synd)
    ref = LSH.reference(c, "normal")
    assert 0 < ref[1].sum() < LSH.B and ref[1][5] == 0
    assert_same(small, ref, "B = 8 against the model")
    cap = cu_count() * LSH.grid_per_cu(info["lds_bytes"], 1024)
    B = 8 * (cap + 1)
    assert B > cap and LSH.grid_per_cu(info["lds_bytes"], 1024) == 2
    assert sorted(ref[3][ref[1] == 1].tolist()) == [0, 0, 0, 1, 2] and np.all(ref[3][ref[1] == 0] == c.max_iter - 1)
    rng = np.random.default_rng([LSH.SEED, 2])
    order = np.concatenate([rng.permutation(8) for _ in range(B // 8)])
    big = dec.decode(synd[order])
    dec.close()
    print("grid", cap, "shots", B)
    assert_same(big, [a[order] for a in small], f"B = {B} against B = 8")


def test_convergence_in_the_last_pass(L):
    """eight shots of the pool, among them those the model finds converging after the last layer of the last iteration (conv 1, iter max_iter - 1) and
    those one iteration short (conv 0, the same iter; conv 1 with one iteration more)"""
    c, T = LSH.queue_graph(), LSH.LAST_PASS["max_iter"]
    pool = LSH.last_pass_pool(c, LSH.LAST_PASS["weight"], LSH.LAST_PASS["pool"])
    model = LM.LayeredModel(c.indptr, c.indices, c.n, c.priors["normal"])
    hit, short = LSH.last_pass_pair(lambda s, t: model.decode(s, max_iter=t), pool, T)
    assert hit.size and short.size
    pick, hit, short = LSH.last_pass_batch(hit, short, len(pool))
    pool = pool[pick]
    assert len(pool) == LSH.B
    g = L.Graph(c.indptr, c.indices, c.n)
    for t in (T, T + 1):
        dec = L.LayeredDecoder(g, c.priors["normal"], max_iter=t)
        got = dec.decode(pool)
        dec.close()
        assert_same(got, model.decode(pool, max_iter=t), f"max_iter {t}")
        if t == T:
            assert np.all(got[1][hit] == 1) and np.all(got[3][hit] == T - 1) and np.all(got[1][short] == 0) and np.all(got[3][short] == T - 1)
        else:
            assert np.all(got[1][short] == 1) and np.all(got[3][short] == T)
