"""The f32 decoder on the MI355X over its domain (tests/minsum32_shapes.py): on every family qldpc_minsum32_decoder_info equals the restated rules (the
exact LDS bytes, the clean form, the workgroup size up to what the occupancy query may lower) and every output equals the numpy model bit for bit, in
both kernel forms where both exist; the first refused size on the column and on the row side; a workgroup that takes a second shot from the queue;
convergence found in the pass that only tests.  tests/test_minsum32_domain_cpu.py has compared the model with the scalar loop on the same families."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401  (first: the HIP runtime torch loads is the one libqldpc_hip.so then binds to)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import minsum32_shapes as MS  # noqa: E402
from test_layered_domain_gpu import assert_same, cu_count  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = MS.all_cases()
BY_NAME = {c.name: c for c in CASES}
ACCEPTED = [c.name for c in CASES if c.claims["accepted"]]
MODE = {"dynamical": "dynamical", "const": "alvarado"}


@pytest.fixture(scope="module")
def L():
    import qldpc_amd  # noqa: F401
    from qldpc_amd import _lib
    _lib.require_device()
    return _lib


def decoder(L, g, c, flags=(), max_iter=None):
    bits = 0
    for f in flags:
        bits |= getattr(L, "FLAG_F32_" + f)
    return L.Minsum32Decoder(g, c.prior, max_iter=max_iter or c.max_iter, alpha_mode=MODE[c.alpha[0]], alpha=c.alpha[1], clip_llr=c.clip, flags=bits)


def check_info(info, e, what):
    assert info["lds_bytes"] == e["lds_bytes"] and info["clean"] == e["clean"] and info["wg_per_cu"] >= 1, (what, info, e)
    if e["forced"]:
        assert info["block"] == e["first_block"], (what, info)
    elif e["one_wg"]:
        assert info["block"] == 1024 and info["wg_per_cu"] == 1, (what, info)
    else:                                                                       # the occupancy query may lower the first choice
        assert info["block"] in [b for b in (256, 512, 1024) if b <= e["first_block"]], (what, info)


@pytest.mark.parametrize("name", ACCEPTED)
def test_every_family_against_the_rules_and_the_model(L, name):
    c = BY_NAME[name]
    g = L.Graph(c.indptr, c.indices, c.n)
    synd = MS.shots(c)
    seen = set()
    for flags in c.runs:
        dec = decoder(L, g, c, flags)
        info = dec.info()
        got = dec.decode(synd)
        dec.close()
        print(name, flags, info)
        check_info(info, MS.expected(c, flags), f"{name} {flags}")
        assert_same(got, MS.reference(c), f"{name} {flags}")
        seen.add(info["clean"])
    if c.claims["clean"] and len(c.runs) > 1:
        assert seen == {True, False}                                            # both kernel forms ran


@pytest.mark.parametrize("near,far", [("cols_last", "cols_refused"), ("rows_last", "rows_refused")])
def test_the_first_refused_size(L, near, far):
    """a column, or a row, beyond the last accepted size: QLDPC_ERR_UNSUPPORTED, the message names the LDS count, no handle; a call without a handle
    touches nothing"""
    c = BY_NAME[far]
    e = MS.expected(c)
    assert not e["accepted"] and MS.expected(BY_NAME[near])["accepted"] and c.n < 65534
    g = L.Graph(c.indptr, c.indices, c.n)
    lib = L.lib()
    prior = np.ascontiguousarray(c.prior, np.float64)
    for flags in (0, L.FLAG_F32_BLOCK_256, L.FLAG_F32_GENERIC):
        h = C.c_void_p(12345)
        rc = lib.qldpc_minsum32_decoder_create(g.handle, L.ptr(prior, C.c_double), 4, 1, 1.0, None, 0, 20.0, flags, C.byref(h))
        msg = lib.qldpc_last_error().decode()
        assert rc == -4 and h.value is None and "LDS" in msg and f"{c.n} columns and {c.m} rows need {e['lds_bytes']} bytes" in msg, msg
    synd = MS.shots(c)
    err, llr = np.full((MS.B, c.n), 9, np.int8), np.full((MS.B, c.n), 9.0)
    conv, it = np.full(MS.B, 9, np.uint8), np.full(MS.B, -7, np.int32)
    rc = lib.qldpc_minsum32_decode_batch(None, MS.B, L.ptr(synd, C.c_int8), L.ptr(err, C.c_int8), L.ptr(llr, C.c_double), L.ptr(conv, C.c_uint8), L.ptr(it, C.c_int32))
    assert rc == -1 and (err == 9).all() and (llr == 9.0).all() and (conv == 9).all() and (it == -7).all()


@pytest.mark.parametrize("form", [(), (MS.GENERIC,)], ids=["clean", "generic"])
def test_the_queue_hands_out_a_second_shot(L, form):
    """Eight shots for every workgroup of the grid and eight more, B = 8 (cap + 1): each of the eight kinds of shot -- five that converge (in
    iterations 0, 0, 0, 1 and 4 by the model), three that run all nine iterations and leave an unsat flag set, one of these with a 1 on the row
    without entries -- occurs cap + 1 times, and a workgroup ends on one shot only, so whichever way the atomic queue deals them, every kind is
    followed by another shot in some workgroup.  That workgroup must rewrite V and the syndrome bytes, must not overwrite them or the flags before
    every thread is done with the shot before (the trailing barrier), and must write its outputs to the rows of the shot it drew.  Every block
    of eight is another order of the eight shots, so every row of the big call has a row of the B = 8 call to equal, and that call equals the
    model.  What the run cannot tell: WHICH shot follows which (the queue decides); a missing barrier shows only if the race is lost in this run.
    Two things the kernel does per shot that no run can show, by its own code: the reset of the two unsat flags at the head of a shot (pass `it`
    clears the flag of pass `it + 1` before that pass sets and reads it, and pass 0 reads none, so the flags an unconverged shot leaves set --
    both, at max_iter = 9 -- are cleared before they are read whether or not they are reset), and the it > 0 guard on loading the records of the
    shot before (what is loaded is used only under it > 0 again)."""
    c = MS.queue_case()
    g = L.Graph(c.indptr, c.indices, c.n)
    synd = MS.shots(c)
    assert (c.row_deg == 0).any() and synd[5, c.row_deg == 0].any()
    dec = decoder(L, g, c, form + (MS.BLOCK_1024,))
    info = dec.info()
    assert info["block"] == 1024 and info["clean"] == (not form)
    small = dec.decode(synd)
    ref = MS.reference(c)
    assert 0 < ref[1].sum() < MS.B and ref[1][5] == 0
    assert_same(small, ref, "B = 8 against the model")
    cap = cu_count() * info["wg_per_cu"]
    B = 8 * (cap + 1)
    assert B > cap
    assert sorted(ref[3][ref[1] == 1].tolist()) == [0, 0, 0, 1, 4] and np.all(ref[3][ref[1] == 0] == c.max_iter - 1)
    rng = np.random.default_rng([MS.SEED, 2])
    order = np.concatenate([rng.permutation(8) for _ in range(B // 8)])
    big = dec.decode(synd[order])
    dec.close()
    print("grid", cap, "shots", B)
    assert_same(big, [a[order] for a in small], f"B = {B} against B = 8")


@pytest.mark.parametrize("form", [(), (MS.GENERIC,)], ids=["clean", "generic"])
def test_convergence_in_the_last_pass(L, form):
    """eight shots of the pool, among them those the model finds converging in the pass that only tests (conv 1, iter max_iter - 1) and those one
    iteration short (conv 0, the same iter; conv 1 with one iteration more)"""
    c, T = MS.queue_case(), MS.LAST_PASS["max_iter"]
    pool = MS.last_pass_pool(c, MS.LAST_PASS["weight"], MS.LAST_PASS["pool"])
    hit, short = MS.LSH.last_pass_pair(lambda s, t: MS.model_decode(c, s, max_iter=t), pool, T)
    assert hit.size and short.size
    pick, hit, short = MS.LSH.last_pass_batch(hit, short, len(pool))
    pool = pool[pick]
    assert len(pool) == MS.B
    g = L.Graph(c.indptr, c.indices, c.n)
    for t in (T, T + 1):
        dec = decoder(L, g, c, form, max_iter=t)
        assert dec.info()["clean"] == (not form)
        got = dec.decode(pool)
        dec.close()
        assert_same(got, MS.model_decode(c, pool, max_iter=t), f"max_iter {t}")
        if t == T:
            assert np.all(got[1][hit] == 1) and np.all(got[3][hit] == T - 1) and np.all(got[1][short] == 0) and np.all(got[3][short] == T - 1)
        else:
            assert np.all(got[1][short] == 1) and np.all(got[3][short] == T)
