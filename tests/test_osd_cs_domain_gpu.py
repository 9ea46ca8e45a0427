"""OSD-CS (qldpc_osdcs_batch, qldpc_osdcs_batch_dev) over every shape, sort form and order it accepts, on the families, shots and weights of
tests/osd_cs_shapes.py.  Every shot of every call is compared with the numpy model (tests/osd_cs_model.py, itself held to a brute-force enumeration by
test_osd_cs_cpu.py): solution and flips bit for bit inside the column space, qldpc_osd0_batch's answer with flips (-1, -1) outside it.
tests/test_osd_cs_domain_cpu.py checks the cases themselves, and the layout rule that labels them, without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

try:            # two HIP runtimes in this image: torch first (see test_gpu_parity.py)
    import torch  # noqa: F401
except ImportError:
    torch = None

import osd_cs_model as M
import osd_cs_shapes as CS
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
        f = CS.family(name)
        _GRAPHS[name] = L.Graph(f.indptr, f.indices, f.n)
    return _GRAPHS[name]


def cost(x, w):
    return (x.astype(np.int64) * M.quantise(w)[None, :]).sum(axis=1)


def held_to_the_model(f, s, w, got, want, o0, what):
    """(solution, flips) of a call on the shots s against the model's `want` (CS.scored) and qldpc_osd0_batch's o0 -> the number of shots compared"""
    sol, fl = got
    msol, mfl, outside, mosd0, mcost = want
    ins = ~outside
    bad = np.flatnonzero(ins & ((sol != msol).any(axis=1) | (fl != mfl).any(axis=1)))
    assert bad.size == 0, (what, "differs from the model", [(int(b), str(s.cls[b]), fl[b].tolist(), mfl[b].tolist()) for b in bad[:8]])
    bad = np.flatnonzero(outside & ((sol != o0).any(axis=1) | (fl != -1).any(axis=1)))
    assert bad.size == 0, (what, "outside the column space: not OSD-0's answer", bad[:8].tolist())
    assert np.array_equal(OS._syndromes(f, sol[ins]), s.synd[ins] & 1), (what, "H x != s")
    c = cost(sol[ins], w)
    assert np.array_equal(c, mcost[ins]) and (c <= cost(o0[ins], w)).all(), (what, "cost")
    return int(ins.sum() + outside.sum())


@pytest.mark.parametrize("name", CS.RUN)
def test_family(L, name):
    """every class of the family in one call, under every weight set, at every order of the family"""
    f, g, s = CS.family(name), graph_of(L, name), CS.batch(name)
    o0 = L.osd0_batch(g, s.synd, s.llr, s.hard)
    B = len(s.cls)
    compared = calls = 0
    seen = {"osd0": 0, "single": 0, "pair": 0}
    for wset in CS.WEIGHT_SETS:
        w = CS.weights(f, wset)
        for order, want in CS.answers(name, wset).items():
            got = L.osdcs_batch(g, s.synd, s.llr, s.hard, w, order)
            compared += held_to_the_model(f, s, w, got, want, o0, (name, wset, order))
            calls += 1
            for k, v in CS.winners(got[1], want[2]).items():
                seen[k] += v
    assert calls == len(CS.WEIGHT_SETS) * len(f.orders) and compared == calls * B          # no shot left out: the share of skipped shots is zero
    forms = ", ".join(f"order {o}: {'global' if CS.cs_layout(f.m, f.n, o)[1] else 'LDS'} sort" for o in f.orders)
    print(f"osd-cs-domain {name}: {f.m} x {f.n}, {f.mw} row words, rank {f.rank}, {f.nonpivot} non-pivot columns, {f.block} threads, {forms}; "
          f"{B} shots x {calls} calls, winners {seen}")


@pytest.mark.parametrize("first", [0, 64])
def test_both_sort_forms_on_one_handle_in_both_call_orders(L, first):
    """m = 1024 with n between the edges: order 0 sorts in LDS, order 64 in global memory.  A fresh handle takes one, then the other (whose workspace is
    larger or smaller), then the first again"""
    name = "cs1024_mid"
    f, s = CS.family(name), CS.batch(name)
    assert (CS.cs_layout(f.m, f.n, 0)[1], CS.cs_layout(f.m, f.n, 64)[1]) == (False, True)
    g = L.Graph(f.indptr, f.indices, f.n)
    o0 = L.osd0_batch(g, s.synd, s.llr, s.hard)
    w = CS.weights(f, "priors")
    want = CS.answers(name, "priors")
    for order in (first, 64 - first, first):
        held_to_the_model(f, s, w, L.osdcs_batch(g, s.synd, s.llr, s.hard, w, order), want[order], o0, (name, "first", first, "order", order))


# ---- 600 shots on 512 workgroups, and the device entry point ----
_BIG = {}


def big(L, kind, wset="mixed", order=7):
    """the 600 shots of CS.big_batch(kind) with the model's answers and OSD-0's, computed once"""
    if kind not in _BIG:
        f, s = CS.family(CS.BIG_FAMILY), CS.big_batch(kind)
        w = CS.weights(f, wset)
        want = CS.scored(f, CS.eliminate_all(f, s.synd, s.llr, s.hard), w, order)
        if not hasattr(s, "cls"):
            s.cls = np.repeat(["random syndrome"], len(s.synd))
        _BIG[kind] = (f, s, w, order, want, L.osd0_batch(graph_of(L, CS.BIG_FAMILY), s.synd, s.llr, s.hard))
    return _BIG[kind]


def dev_call(L, g, s, w, order, select=None, alias=False, fill=5):
    """qldpc_osdcs_batch_dev on the null stream -> (solution, flips); rows not listed keep `fill` / -7 (hard itself under alias)"""
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)        # noqa: E731
    p = lambda x: C.c_void_p(x.data_ptr())                                # noqa: E731
    B = s.synd.shape[0]
    ds, dl, dh, dw = t(s.synd), t(s.llr), t(s.hard), t(np.asarray(w, np.float64))
    dsol = dh if alias else torch.full((B, g.n), fill, dtype=torch.int8, device=dev)
    dfl = torch.full((B, 2), -7, dtype=torch.int32, device=dev)
    sel = cnt = None
    if select is not None:
        sel, cnt = t(np.asarray(select, np.int32).reshape(-1) if len(select) else np.zeros(1, np.int32)), t(np.array([len(select)], np.int32))
    torch.cuda.synchronize()
    L.check(L.lib().qldpc_osdcs_batch_dev(g.handle, C.c_int64(B), p(ds), p(dl), p(dh), p(dw), int(order), p(sel) if sel is not None else None,
                                          p(cnt) if cnt is not None else None, p(dsol), p(dfl), C.c_void_p(0)))
    torch.cuda.synchronize()
    return dsol.cpu().numpy(), dfl.cpu().numpy()


def test_batch_larger_than_the_grid(L):
    """every class side by side: the work queue hands a second shot to some workgroups, and the redo list holds a tenth of the batch"""
    f, s, w, order, want, o0 = big(L, "classes")
    assert want[2].sum() == CS.BIG_BATCH // len(CS.classes_of(f))
    got = L.osdcs_batch(graph_of(L, CS.BIG_FAMILY), s.synd, s.llr, s.hard, w, order)
    assert held_to_the_model(f, s, w, got, want, o0, "600 shots") == CS.BIG_BATCH


def test_redo_list_holds_every_shot(L):
    f, s, w, order, want, o0 = big(L, "outside")
    assert want[2].all()
    got = L.osdcs_batch(graph_of(L, CS.BIG_FAMILY), s.synd, s.llr, s.hard, w, order)
    assert held_to_the_model(f, s, w, got, want, o0, "600 shots outside") == CS.BIG_BATCH


def test_device_entry_with_a_permuted_select_list(L):
    """560 of the 600 shots (still more than the grid) listed in a seeded random order: the listed rows are the model's, the others keep their sentinels"""
    f, s, w, order, want, o0 = big(L, "classes")
    g = graph_of(L, CS.BIG_FAMILY)
    select = np.random.default_rng(OS.SEED).permutation(CS.BIG_BATCH)[:560]
    sol, fl = dev_call(L, g, s, w, order, select=select)
    rest = np.setdiff1d(np.arange(CS.BIG_BATCH), select)
    assert (sol[rest] == 5).all() and (fl[rest] == -7).all()
    pick = lambda a: a[np.sort(select)]                                   # noqa: E731
    sub = type(s)(cls=pick(s.cls), synd=pick(s.synd), llr=pick(s.llr), hard=pick(s.hard))
    assert held_to_the_model(f, sub, w, (pick(sol), pick(fl)), tuple(pick(a) for a in want), pick(o0), "select list") == select.size


def test_device_entry_with_an_empty_select_list(L):
    f, s, w, order, want, o0 = big(L, "classes")
    sol, fl = dev_call(L, graph_of(L, CS.BIG_FAMILY), s, w, order, select=[])
    assert (sol == 5).all() and (fl == -7).all()


@pytest.mark.parametrize("form", ["L", "G"])
def test_solution_may_alias_hard(L, form):
    """d_solution == d_hard on the device entry: the same answers as with a buffer of its own, which is held to the model first"""
    name = CS.ALIAS_FAMILIES[form]
    f, g, s = CS.family(name), graph_of(L, name), CS.batch(name)
    order, wset = 7, "mixed"
    assert CS.cs_layout(f.m, f.n, order)[1] == (form == "G")
    w, want = CS.weights(f, wset), CS.answers(name, wset)[order]
    o0 = L.osd0_batch(g, s.synd, s.llr, s.hard)
    own = dev_call(L, g, s, w, order)
    assert held_to_the_model(f, s, w, own, want, o0, (name, "own buffer")) == len(s.cls)
    assert want[2].any() and (~want[2]).any()          # both kinds of shot: the sweep's own answer and OSD-0's behind the redo list
    aliased = dev_call(L, g, s, w, order, alias=True)
    assert np.array_equal(aliased[0], own[0]) and np.array_equal(aliased[1], own[1])


@pytest.mark.parametrize("name", [n for n in CS.TABLE if CS.TABLE[n][5] is None])
def test_refused_shapes(L, name):
    """n = 65536 and m = 1025: QLDPC_ERR_UNSUPPORTED with the documented text, from both entry points"""
    f = CS.family(name)
    g = L.Graph(f.indptr, f.indices, f.n)
    synd, llr, hard, w = np.zeros((1, f.m), np.int8), np.ones((1, f.n)), np.zeros((1, f.n), np.int8), np.ones(f.n)
    with pytest.raises(L.QldpcError) as e:
        L.osdcs_batch(g, synd, llr, hard, w, 7)
    assert "error -4" in str(e.value) and CS.UNSUPPORTED_TEXT in str(e.value) and f"{f.m} x {f.n}" in str(e.value), str(e.value)
    rc = L.lib().qldpc_osdcs_batch_dev(g.handle, C.c_int64(1), None, None, None, None, 0, None, None, None, None, C.c_void_p(0))
    assert rc == -4 and CS.UNSUPPORTED_TEXT in L.lib().qldpc_last_error().decode()          # (refused before any buffer is looked at)
